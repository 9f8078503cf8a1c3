"""Groups the JSON lines that tests/test_absgrad_gpu.py writes with SIU3R_ABSGRAD_PARITY_LOG=parity.jsonl into profiles/absgrad_parity.json:
per comparison of abs_mean2d (one view of one case) the largest |got - ref| / S, the worst element as a fraction of its tolerance, and the
tolerance itself as a multiple of S.

    SIU3R_ABSGRAD_PARITY_LOG=parity.jsonl python -m pytest tests/test_absgrad_gpu.py
    python tools/absgrad_parity.py parity.jsonl profiles/absgrad_parity.json
"""
import collections
import json
import sys

U24 = 2.0 ** -24
WHAT = ("tests/test_absgrad_gpu.py on one MI355X: abs_mean2d of siu3r_raster_composite_rgb_bwd_abs against tests/dense_absgrad64.py.  Per comparison: "
        "max_err_over_S = the largest |got - ref| / S over the elements, S = composite_bwd64's sum of the absolute terms of the signed mean element; "
        "worst_ratio_to_bound = the worst element as a fraction of its tolerance (64 + 3 + addends) u S + chain, the signed element's; bound_over_S_u = "
        "that tolerance as a multiple of S in units of u = 2^-24, median and largest element.  Records: the bound does not come from them.")


def main(src, dst):
    r4 = lambda x: float("%.4g" % x)
    cases = collections.OrderedDict()
    for line in open(src):
        d = json.loads(line)
        cases[d["case"]] = dict(max_err_over_S=r4(d["max_err_over_S"]), worst_ratio_to_bound=r4(d["worst_ratio_to_bound"]),
                                bound_over_S_u=[round(d["bound_over_S_median"] / U24), round(d["bound_over_S_max"] / U24)])
    worst = dict(max_err_over_S=max(c["max_err_over_S"] for c in cases.values()), worst_ratio_to_bound=max(c["worst_ratio_to_bound"] for c in cases.values()))
    with open(dst, "w") as f:
        json.dump(dict(what=WHAT, all_cases=worst, cases=cases), f, indent=0)
        f.write("\n")
    print(json.dumps(worst))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
