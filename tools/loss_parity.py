"""Groups the JSON lines that tests/test_loss_stages_gpu.py writes with SIU3R_LOSS_PARITY_LOG=parity.jsonl into profiles/loss_parity.json:
per comparison and per kernel the worst element as a fraction of its tolerance, and the tolerance itself as a multiple of the element's
scale (tests/dense_photo64.py, tests/dense_depth64.py).

    SIU3R_LOSS_PARITY_LOG=parity.jsonl python -m pytest tests/test_loss_stages_gpu.py
    python tools/loss_parity.py parity.jsonl profiles/loss_parity.json
"""
import collections
import json
import sys

U24 = 2.0 ** -24
WHAT = ("tests/test_loss_stages_gpu.py on one MI355X.  Per comparison (one output of one crafted case) and per kernel: worst_ratio_to_bound = "
        "the worst element as a fraction of its tolerance; bound_over_S_u = the tolerance as a multiple of the element's scale S in units of "
        "u = 2^-24 = 5.96e-08, median and largest element; bound_over_ref_u = the median tolerance as a multiple of |ref|, in u.  Photo: S is the first-order count of the kernel's roundings on the float64 "
        "intermediates of the element (shifted units), tolerance 2 u S + the allowance of undecided windows.  Depth: S = |ref|, tolerance "
        "(u + 32 * 2^-53) S + the fp64 error of the view's statistics + 2^-149.  Records: the bounds do not come from them.")


def main(src, dst):
    r4 = lambda x: float("%.4g" % x)
    cases, kernels = collections.OrderedDict(), collections.OrderedDict()
    for line in open(src):
        d = json.loads(line)
        c = dict(kernel=d["kernel"], worst_ratio_to_bound=r4(d["worst_ratio_to_bound"]),
                 bound_over_S_u=[r4(d["bound_over_S_median"] / U24), r4(d["bound_over_S_max"] / U24)], bound_over_ref_u=r4(d["bound_over_ref_median"] / U24))
        cases[d["case"]] = c
        k = kernels.setdefault(d["kernel"], dict(worst_ratio_to_bound=0.0, worst_case="", comparisons=0))
        k["comparisons"] += 1
        if c["worst_ratio_to_bound"] >= k["worst_ratio_to_bound"]:
            k["worst_ratio_to_bound"], k["worst_case"] = c["worst_ratio_to_bound"], d["case"]
    with open(dst, "w") as f:
        json.dump(dict(what=WHAT, kernels=kernels, cases=cases), f, indent=0)
    print(json.dumps(kernels, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
