"""Launch trace of the forward: every call the Python side makes through the C ABI (include/siu3r_hip.h), in order, with its arguments --
the instrument for proving that a change to the Python files leaves what runs on the GPU alone (two trees, one built library).

  python tools/launch_trace.py --out new.json [--tree DIR] [--precision bf16x3] [--batch 1] [--views 2] [--size 128 128] [--time N]
  python tools/launch_trace.py --diff old.json new.json        (exit status 1 and the first difference when they are not equal)

Three forwards (eager, graph capture, graph replay; all eager under SIU3R_NO_GRAPH=1) on seeded input and oracle.weights.make_weights(0).
Per call: the function, every non-pointer argument, every non-zero non-pointer field of a by-reference struct, pointers as "ptr"
(null ones are left out with the zeros), the stream as "s<n>" = the n-th distinct stream of the process; a plan query also logs the
plan it got back.  Per forward: sha256 of the six Gaussian fields, the class and mask logits and the segments info.
--tree DIR imports DIR/siu3r_amd instead of this tree's package (DIR needs the Python files only: the library is this tree's).
--time N adds the device-event time of N replayed and N eager forwards, each between two synchronisations.
The SIU3R_* switches are read at import: one process per configuration."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    """stands in front of the loaded library (siu3r_amd._lib.lib()): logs each call into `log`, then makes it"""

    def __init__(self, real, signatures, log, torch):
        self._real, self._sig, self.log, self._torch, self._streams = real, signatures, log, torch, {}

    def _struct(self, s):
        out = {}
        for name, ct in s._fields_:
            v = getattr(s, name)
            if ct is C.c_void_p:
                v = "ptr" if v else None
            elif isinstance(v, C.Array):
                v = list(v)
            elif isinstance(v, bytes):
                v = v.decode()
            if v:  # (zeros and null pointers are the struct's defaults)
                out[name] = v
        return out

    def _arg(self, a, ct, last):
        if ct is C.c_void_p:
            if last and (a or 0) == self._torch.cuda.current_stream().cuda_stream:
                return "s%d" % self._streams.setdefault(a or 0, len(self._streams))
            return "ptr" if a else None
        if isinstance(a, C.Array):
            return list(a)
        if hasattr(a, "_obj"):  # ctypes.byref(struct)
            return self._struct(a._obj)
        return a

    def __getattr__(self, name):
        fn, sig = getattr(self._real, name), self._sig.get(name)
        if sig is None or name == "siu3r_last_error":
            return fn

        def call(*args):
            plan = next((a for a in args if type(getattr(a, "_obj", None)).__name__.endswith("Plan")), None)  # an output: logged behind the call
            entry = [name] + [self._arg(a, ct, i == len(args) - 1) for i, (a, ct) in enumerate(zip(args, sig)) if a is not plan]
            self.log.append(entry)
            rc = fn(*args)
            entry.append({"rc": rc, **({"plan": self._struct(plan._obj)} if plan is not None else {})})
            return rc

        return call


def _sha(t):
    import torch

    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run(a):
    if a.tree:
        os.environ.setdefault("SIU3R_LIB_OVERRIDE", os.path.join(ROOT, "siu3r_amd", "libsiu3r_hip.so"))
    sys.path[:0] = [os.path.abspath(a.tree)] if a.tree else [ROOT]
    if ROOT not in sys.path:
        sys.path.append(ROOT)  # oracle/
    import torch
    from oracle import weights as OW
    from siu3r_amd import _lib, model as M
    from siu3r_amd.gaussians_types import Gaussians

    assert os.path.dirname(os.path.abspath(M.__file__)) == os.path.join(os.path.abspath(a.tree or ROOT), "siu3r_amd"), M.__file__
    log = []
    _lib._lib = _Recorder(_lib.lib(), _lib.SIGNATURES, log, torch)
    B, V, (H, W) = a.batch, a.views, a.size
    img = torch.rand(B, V, 3, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    K = torch.tensor([[318 / 256, 0, 0.5], [0, 318 / 256, 0.5], [0, 0, 1]])[None, None].repeat(B, V, 1, 1).cuda()
    m = (M.SIU3RModel if V == 2 else M.SIU3RMultiViewModel)(OW.make_weights(0), image_size=(H, W), precision=a.precision)
    runs = []
    with torch.no_grad():
        for _ in range(3):
            del log[:]
            g, seg, masks, infos, _ = m(img, K, enable_query_class_logit_lift=True)
            torch.cuda.synchronize()
            h = {f: _sha(getattr(g, f)) for f in Gaussians.FIELDS}
            h.update(class_logits=_sha(seg.class_queries_logits), mask_logits=_sha(seg.masks_queries_logits),
                     segments_info=hashlib.sha256(json.dumps(infos, sort_keys=True, default=float).encode()).hexdigest())
            runs.append({"calls": list(log), "hashes": h})
        res = {"config": {**vars(a), "switches": {k: v for k, v in sorted(os.environ.items()) if k.startswith("SIU3R_") and k != "SIU3R_LIB_OVERRIDE"}}, "runs": runs}
        if a.time:
            _lib._lib = _lib._lib._real
            for mode in ("replay", "eager"):
                m.use_graph = m.use_graph and mode == "replay"
                ms = []
                for _ in range(a.time + 1):  # (the first one is a warm-up of this mode)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    m(img, K, enable_query_class_logit_lift=True)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                res["time_ms_" + mode] = {"median": statistics.median(ms[1:]), "min": min(ms[1:]), "max": max(ms[1:]), "board": torch.cuda.get_device_name(0)}
    json.dump(res, open(a.out, "w"))
    digest = hashlib.sha256(json.dumps(runs, sort_keys=True).encode()).hexdigest()
    print(f"{a.out}: {[len(r['calls']) for r in runs]} calls, trace+hashes sha256 {digest[:16]}", {k: v for k, v in res.items() if k.startswith("time")})


def diff(pa, pb):
    ra, rb = json.load(open(pa))["runs"], json.load(open(pb))["runs"]
    for i, (x, y) in enumerate(zip(ra, rb)):
        bad = [k for k in x["hashes"] if x["hashes"][k] != y["hashes"][k]]
        if bad:
            print(f"forward {i}: output hashes differ: {bad}")
        for j, (cx, cy) in enumerate(zip(x["calls"], y["calls"])):
            if cx != cy:
                print(f"forward {i}, call {j} differs:\n  {pa}: {cx}\n  {pb}: {cy}")
                return 1
        if bad or len(x["calls"]) != len(y["calls"]):
            print(f"forward {i}: {len(x['calls'])} vs {len(y['calls'])} calls")
            return 1
    print(f"equal: {[len(r['calls']) for r in ra]} calls, {len(ra[0]['hashes'])} output hashes per forward")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--diff", nargs=2, metavar="JSON")
    ap.add_argument("--out", default="launch_trace.json")
    ap.add_argument("--tree")
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[128, 128], metavar=("H", "W"))
    ap.add_argument("--time", type=int, default=0)
    args = ap.parse_args()
    sys.exit(diff(*args.diff) if args.diff else run(args))
