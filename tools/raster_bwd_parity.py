"""Groups the JSON lines that tests/test_raster_bwd_stages_gpu.py writes with SIU3R_RASTER_BWD_PARITY_LOG=parity.jsonl into
profiles/raster_bwd_parity.json: per comparison and per stage the largest |got - ref| / S (S: the sum of the absolute terms of the
element, tests/dense_raster_bwd64.py), the worst element as a fraction of its tolerance, and the tolerance itself as a multiple of S.

    SIU3R_RASTER_BWD_PARITY_LOG=parity.jsonl python -m pytest tests/test_raster_bwd_stages_gpu.py
    python tools/raster_bwd_parity.py parity.jsonl profiles/raster_bwd_parity.json
"""
import collections
import json
import re
import sys

U24 = 2.0 ** -24
WHAT = ("tests/test_raster_bwd_stages_gpu.py on one MI355X.  Per comparison (one output tensor of one case) and per stage: max_err_over_S = the "
        "largest |got - ref| / S over the elements, S = the sum of the absolute values of the element's terms (projection: weighted by the "
        "condition of the slot's chain, at most 12.7); worst_ratio_to_bound = the worst element as a fraction of its tolerance; bound_over_S_u = "
        "the tolerance as a multiple of S in units of u = 2^-24 = 5.96e-08, median and largest element: PROJ_BOUND 164 u, SH_BOUND 72 u, "
        "QUAT_BOUND 64 u, rows (ceil(n / 256) + 9) u, composite (64 + channels + addends) u plus the derived error of the element's alpha / "
        "transmittance chains (tests/dense_raster_bwd64.py, header).  Records: the bounds do not come from them.")


def stage(name):
    if re.match(r"k[23]_(deg|pre|one|rgb|views|two)", name):
        return "projection"
    if name.startswith("siu3r_raster_"):
        return "rows_reduce"
    if name.startswith("quat"):
        return "quat_scale_to_cov6_bwd"
    if name.startswith("sh_eval"):
        return "sh_eval_bwd"
    return "composite_on_the_forward_state" if name.startswith("forward_") else "composite"


def main(src, dst):
    r4 = lambda x: float("%.4g" % x)
    cases, stages = collections.OrderedDict(), collections.OrderedDict()
    for line in open(src):
        d = json.loads(line)
        c = dict(max_err_over_S=r4(d["max_err_over_S"]), worst_ratio_to_bound=r4(d["worst_ratio_to_bound"]),
                 bound_over_S_u=[round(d["bound_over_S_median"] / U24), round(d["bound_over_S_max"] / U24)])
        cases[d["case"]] = c
        s = stages.setdefault(stage(d["case"]), dict(max_err_over_S=0.0, worst_ratio_to_bound=0.0, bound_over_S_u=[0, 0]))
        s["max_err_over_S"] = max(s["max_err_over_S"], c["max_err_over_S"])
        s["worst_ratio_to_bound"] = max(s["worst_ratio_to_bound"], c["worst_ratio_to_bound"])
        s["bound_over_S_u"] = [max(s["bound_over_S_u"][0], c["bound_over_S_u"][0]), max(s["bound_over_S_u"][1], c["bound_over_S_u"][1])]
    with open(dst, "w") as f:
        json.dump(dict(what=WHAT, stages=stages, cases=cases), f, indent=0)
    print(json.dumps(stages, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
