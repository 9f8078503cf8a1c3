"""The JSON lines tests/test_panoptic_stages_gpu.py appends under SIU3R_PANOPTIC_PARITY_LOG -> profiles/panoptic_parity.json: per case and
per stage the worst element as a fraction of its derived bound (tests/dense_panoptic64.py) and the undecided share; the qcl calls of a
case (every item and nq) are folded into one entry with their number.

    SIU3R_PANOPTIC_PARITY_LOG=parity.jsonl python -m pytest tests/test_panoptic_stages_gpu.py
    python tools/panoptic_parity.py parity.jsonl profiles/panoptic_parity.json
"""
import json
import sys


def main(src, dst):
    cases = {}
    for line in open(src):
        r = json.loads(line)
        stage = r["stage"].split(" ")[0]
        e = cases.setdefault(r["case"], {}).setdefault(stage, {"worst_ratio": 0.0, "undecided_share": 0.0, "calls": 0})
        e["worst_ratio"] = round(max(e["worst_ratio"], r["worst_ratio_to_bound"]), 4)
        e["undecided_share"] = round(max(e["undecided_share"], r["undecided_share"]), 6)
        e["calls"] += 1
    what = ("tests/test_panoptic_stages_gpu.py on one MI355X: per case and stage of csrc/postprocess.hip the worst element's |out - ref| as a "
            "fraction of the bound derived in tests/dense_panoptic64.py (0 for the integer stages: exact on decided elements) and the share of "
            "undecided rows / pixels / (pixel, query) pairs (cap 0.005).  Records: the bounds do not come from them.")
    with open(dst, "w") as f:
        json.dump({"what": what, "cases": cases}, f, indent=0)
        f.write("\n")
    worst = max(s["worst_ratio"] for c in cases.values() for s in c.values())
    share = max(s["undecided_share"] for c in cases.values() for s in c.values())
    print(f"{len(cases)} cases, worst ratio {worst}, largest undecided share {share}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
