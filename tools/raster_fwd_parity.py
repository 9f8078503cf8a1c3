"""Groups the JSON lines that tests/test_raster_fwd_stages_gpu.py writes with SIU3R_RASTER_FWD_PARITY_LOG=parity.jsonl into
profiles/raster_fwd_parity.json: per comparison (one output map of one case, or the record of one projection case) and per stage the
worst element as a fraction of its tolerance, the tolerance itself as a multiple of S (S: the sum of the absolute terms of the element,
tests/dense_raster_fwd64.py) in units of u = 2^-24, median and largest element, and the share of undecided rows / margin pixels.

    SIU3R_RASTER_FWD_PARITY_LOG=parity.jsonl python -m pytest tests/test_raster_fwd_stages_gpu.py
    python tools/raster_fwd_parity.py parity.jsonl profiles/raster_fwd_parity.json
"""
import collections
import json
import sys

U24 = 2.0 ** -24
WHAT = ("tests/test_raster_fwd_stages_gpu.py on one MI355X.  Per comparison and per stage: worst_ratio_to_bound = the worst element as a fraction of "
        "its tolerance (below 1 everywhere; headroom = 1 - that); bound_over_S_u = the tolerance as a multiple of S in units of u = 2^-24 = 5.96e-08, "
        "median and largest element (projection: PROJ_MEAN_BOUND 26 u for mean and depth, PROJ_FWD_BOUND 74 u for the conic, SH_FWD_BOUND 80 u for "
        "SH colours, S weighted by the conditions of the slot's chain; composites: sum_j |f_j| w_j (e_w(j) + (2 + entries blended behind j) u) + "
        "|bg| T (e_T + u) over S = sum_j |f_j| w_j + |bg| T); undecided_share = rows (projection) or pixels (composites) within MARGIN = 4 "
        "derived errors of a threshold, capped at 0.01.  Records: the bounds do not come from them.")


def stage(name):
    if name.startswith("proj pose"):
        return "pose_kernels_and_projection"
    if name.startswith("proj "):
        return "project_kernel"
    if name.startswith("forward_"):
        return "composites_on_a_real_projection"
    if " feat_ws " in name or " np=" in name:
        return "composite_feat5_kernel"
    if " feat " in name:
        return "composite_feat_kernel"
    return "composite_rgb_kernel"


def main(src, dst):
    r4 = lambda x: float("%.4g" % x)
    cases, stages = collections.OrderedDict(), collections.OrderedDict()
    for line in open(src):
        d = json.loads(line)
        c = dict(worst_ratio_to_bound=r4(d["worst_ratio_to_bound"]), bound_over_S_u=[round(d["bound_over_S_median"] / U24), round(d["bound_over_S_max"] / U24)],
                 undecided_share=r4(d["undecided_share"]))
        cases[d["case"]] = c
        s = stages.setdefault(stage(d["case"]), dict(comparisons=0, worst_ratio_to_bound=0.0, headroom=1.0, bound_over_S_u=[0, 0], undecided_share=0.0))
        s["comparisons"] += 1
        s["worst_ratio_to_bound"] = max(s["worst_ratio_to_bound"], c["worst_ratio_to_bound"])
        s["headroom"] = r4(1.0 - s["worst_ratio_to_bound"])
        s["bound_over_S_u"] = [max(s["bound_over_S_u"][0], c["bound_over_S_u"][0]), max(s["bound_over_S_u"][1], c["bound_over_S_u"][1])]
        s["undecided_share"] = max(s["undecided_share"], c["undecided_share"])
    with open(dst, "w") as f:
        json.dump(dict(what=WHAT, stages=stages, cases=cases), f, indent=0)
    print(json.dumps(stages, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
