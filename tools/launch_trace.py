"""Launch trace: every call the Python side makes through the C ABI (include/siu3r_hip.h), in order, with its arguments --
the instrument for proving that a change to the Python files leaves what runs on the GPU alone (two trees, one built library).

  python tools/launch_trace.py --out new.json [--tree DIR] [--precision bf16x3] [--batch 1] [--views 2] [--size 128 128] [--time N]
  python tools/launch_trace.py --scenario raster --out new.json [--tree DIR]
  python tools/launch_trace.py --diff old.json new.json [--repeat old2.json]   (exit status 1 and the difference when they are not equal)

--scenario forward (the default): three forwards (eager, graph capture, graph replay; all eager under SIU3R_NO_GRAPH=1) on seeded input and oracle.weights.make_weights(0).
--scenario raster: the rasterizer front-end (siu3r_amd/raster.py) on a seeded scene of 300 Gaussians, two 64 x 48 views -- every pose form of
rasterize_views_k2 / _k3 / _k3_rgb, the 32-channel and the matrix-core N-channel composite, each without grad and with grad + a backward, then
an entry overflow that is repeated and a deferred check; one run per case, sha256 of every returned tensor, of the state buffers a backward
reads again and of every gradient; the gradients themselves go to <out>.grads.npz beside the trace.  The backward kernels accumulate with float
atomics, so the bits of a gradient change from one process to the next on ONE tree: with --repeat old2.json, a second trace of the old tree,
a hash on which old.json and old2.json disagree is compared by value instead -- the largest element-wise |old - new| must not exceed 8 x
the largest |old - old2| (_close) -- and everything the old tree reproduces (every call, every forward output, the state) must be equal.
Per call: the function, every non-pointer argument, every non-zero non-pointer field of a struct (by reference, or an array by value), pointers as "ptr"
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
            return [self._struct(x) if isinstance(x, C.Structure) else x for x in a]
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


def _start(a):
    """put the tree under test first on the path, load its package on this tree's library and stand the recorder in front of that"""
    if a.tree:
        os.environ.setdefault("SIU3R_LIB_OVERRIDE", os.path.join(ROOT, "siu3r_amd", "libsiu3r_hip.so"))
    sys.path[:0] = [os.path.abspath(a.tree)] if a.tree else [ROOT]
    if ROOT not in sys.path:
        sys.path.append(ROOT)  # oracle/
    import torch
    from siu3r_amd import _lib

    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(a.tree or ROOT), "siu3r_amd"), _lib.__file__
    log = []
    _lib._lib = _Recorder(_lib.lib(), _lib.SIGNATURES, log, torch)
    return torch, _lib, log


def _finish(a, res):
    json.dump(res, open(a.out, "w"))
    digest = hashlib.sha256(json.dumps(res["runs"], sort_keys=True).encode()).hexdigest()
    print(f"{a.out}: {[len(r['calls']) for r in res['runs']]} calls, trace+hashes sha256 {digest[:16]}", {k: v for k, v in res.items() if k.startswith("time")})


def run(a):
    torch, _lib, log = _start(a)
    from oracle import weights as OW
    from siu3r_amd import model as M
    from siu3r_amd.gaussians_types import Gaussians

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
    _finish(a, res)


def run_raster(a):
    torch, _lib, log = _start(a)
    from siu3r_amd import cuda_splatting as CS, density, raster

    G, V, W, H = 300, 2, 64, 48
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    A = 0.3 * (rnd(G, 3, 3) - 0.5)
    scene = dict(means=torch.cat((2.4 * rnd(G, 2) - 1.2, 2.0 + 3.0 * rnd(G, 1)), 1), cov6=raster.cov6_from_cov3x3(A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)),
                 opac=0.2 + 0.7 * rnd(G), shs=rnd(G, 9, 3) - 0.5, rgb=rnd(G, 3), feats8=rnd(G, 8) - 0.5, feats40=rnd(G, 40) - 0.5)
    ext = torch.eye(4).repeat(V, 1, 1)  # camera-to-world: view 1 stands 0.3 to the right and looks slightly inwards
    c, s = float(torch.cos(torch.tensor(0.08))), float(torch.sin(torch.tensor(0.08)))
    ext[1, :3, :3] = torch.tensor([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    ext[1, 0, 3] = 0.3
    intr = torch.tensor([[1.1, 0.0, 0.5], [0.0, 1.4, 0.5], [0.0, 0.0, 1.0]]).repeat(V, 1, 1)  # normalised by the frame size
    Kpix = intr * torch.tensor([float(W), float(H), 1.0])[:, None]
    near, far, bg = torch.full((V,), 0.1), torch.full((V,), 100.0), [0.1, 0.2, 0.3]
    w2c = torch.linalg.inv(ext)
    fov_x, fov_y = CS.get_fov(intr).unbind(-1)
    full = CS.get_projection_matrix(near, far, fov_x, fov_y) @ w2c
    k2_host = [raster.make_cam_k2(w2c[v], full[v], float((0.5 * fov_x[v]).tan()), float((0.5 * fov_y[v]).tan()), ext[v, :3, 3].tolist(), bg, W, H, sh_degree=2)
               for v in range(V)]
    k2_dev = [raster.make_cam_k2(None, None, None, None, None, bg, W, H, sh_degree=2, near=0.1, far=100.0) for v in range(V)]
    k3_host = [raster.make_cam_k3(w2c[v], Kpix[v, 0, 0], Kpix[v, 1, 1], Kpix[v, 0, 2], Kpix[v, 1, 2], W, H) for v in range(V)]
    k3_dev = [raster.make_cam_k3(torch.eye(4), 1.0, 1.0, 0.0, 0.0, W, H) for v in range(V)]

    def k2(t, cams, **kw):
        return raster.rasterize_views_k2(cams, t["means"], t["cov6"], t["shs"], t["opac"], **kw)

    def k3(t, cams, feats, **kw):
        return raster.rasterize_views_k3(cams, t["means"], t["cov6"], t["opac"], t[feats], **kw)

    def k3_rgb(t, cams, **kw):
        return raster.rasterize_views_k3_rgb(cams, t["means"], t["cov6"], t["opac"], t["rgb"], **kw)

    c2w = lambda t: (t["ext"], t["intr"], 1.0)
    dp = lambda t: (t["viewmats"], t["Kpix"])
    # name -> (the render, the tensors it takes a gradient for)
    cases = {
        "k2_host": (lambda t: k2(t, k2_host), ("means", "cov6", "shs", "opac")),
        "k2_c2w": (lambda t: k2(t, k2_dev, pose_c2w=c2w(t)), ("means", "cov6", "shs", "opac")),
        "k2_pose_delta_density_stats": (lambda t: k2(t, k2_host, pose_delta=t["pose_delta"], density_stats=t["density_stats"]),
                                        ("means", "cov6", "shs", "opac", "pose_delta")),
        "k3_c8": (lambda t: k3(t, k3_host, "feats8"), ("means", "cov6", "opac", "feats8")),
        "k3_c40": (lambda t: k3(t, k3_host, "feats40"), ("means", "cov6", "opac", "feats40")),
        "k3_c40_pose_dev": (lambda t: k3(t, k3_dev, "feats40", pose_dev=dp(t)), ("means", "cov6", "opac", "feats40", "viewmats")),
        "k3_c8_pose_c2w": (lambda t: k3(t, k3_dev, "feats8", pose_c2w=c2w(t)), ("means", "cov6", "opac", "feats8")),
        "k3_rgb_host": (lambda t: k3_rgb(t, k3_host), ("means", "cov6", "opac", "rgb")),
        "k3_rgb_pose_dev": (lambda t: k3_rgb(t, k3_dev, pose_dev=dp(t)), ("means", "cov6", "opac", "rgb", "viewmats")),
    }

    def tensors(leaves=()):
        t = {k: v.cuda() for k, v in scene.items()}
        t.update(ext=ext.cuda(), intr=intr.cuda(), viewmats=w2c.cuda(), Kpix=Kpix.cuda(), pose_delta=torch.zeros(V, 6).cuda(),
                 density_stats=density.DensityStats(G, "cuda"))
        for k in leaves:
            t[k].requires_grad_(True)
        return t

    def hashes(out):
        """the returned tensors, and of the state what a backward reads again (the valid part of each capacity-bounded buffer)"""
        h = {k: _sha(v) for k, v in out.items() if isinstance(v, torch.Tensor)}
        st = out["state"]
        h.update({"state_" + k: _sha(st[k]) for k in ("rect", "bin_start", "tiles_touched_all")})
        h["state_rec"] = _sha(st["rec"][..., :8])  # mean, depth, conic, opacity: written for every Gaussian
        h["state_totals"] = [st.totals(k) for k in range(4)]
        h["state_entries"] = [_sha(st["entries"][v, :e]) for v, e in enumerate(st.totals(2)) if e <= st["cap_e"]]
        if "colors" in out and out["colors"].shape[-1] != 3:  # the N-channel path: its tile lists exist (reading them builds none)
            h["state_tile_start"] = _sha(st["tile_start_all"])
            h["state_ids"] = [_sha(st["ids_all"][v, :d]) for v, d in enumerate(st.totals(1))]
        else:  # the colour travels in the record: the projection writes it for the Gaussians it keeps (csrc/raster.hip), no other row
            h["state_rec_colour"] = _sha(st["rec"][..., 8:][st["tiles_touched_all"] > 0])
        return h

    runs, values = [], {}  # values: "<run>/<hash key>" -> the gradient itself, for --repeat (written beside the trace, as <out>.grads.npz)

    def case(name, fn):
        del log[:]
        h = fn()
        torch.cuda.synchronize()
        runs.append({"name": name, "calls": list(log), "hashes": h})

    def keep(name, key, t):
        values[name + "/" + key] = t.detach().cpu().numpy()
        return _sha(t)

    def with_grad(name, render, leaves):
        t = tensors(leaves)
        out = render(t)
        h = hashes(out)
        maps = [v for v in out.values() if isinstance(v, torch.Tensor) and v.requires_grad]
        wgen = torch.Generator().manual_seed(5)
        torch.autograd.backward(maps, [torch.rand(m.shape, generator=wgen).cuda() for m in maps])
        h.update({"grad_" + k: keep(name, "grad_" + k, t[k].grad) for k in leaves})
        h.update({"density_" + f: keep(name, "density_" + f, getattr(t["density_stats"], f)) for f in ("grad_accum", "seen", "max_radius")})
        return h

    def retried():
        out = k2(tensors(), k2_host, entry_capacity=8)  # (far too few coarse-bin entries: detected, the call repeated with the exact count)
        return {**hashes(out), "cap_e": out["state"]["cap_e"], "E": out["state"].totals(2)}

    def deferred():
        with torch.no_grad():
            out = k2(tensors(), k2_host, check_overflow="deferred")
            raster.check_pending()
        return {**hashes(out), "call_id": out["call_id"], "pending": len(raster._PENDING)}

    for name, (render, leaves) in cases.items():
        with torch.no_grad():
            case(name, lambda: hashes(render(tensors())))
        case(name + "+grad", lambda: with_grad(name + "+grad", render, leaves))
    with torch.no_grad():
        case("k2_host_entry_overflow_retried", retried)
    case("k2_host_deferred", deferred)
    cams = []  # every distinct camera array once; a call names it as {"cams": index}

    def intern(x):
        if not (isinstance(x, list) and x and isinstance(x[0], dict)):
            return x
        if x not in cams:
            cams.append(x)
        return {"cams": cams.index(x)}

    for r in runs:
        r["calls"] = [[intern(x) for x in c] for c in r["calls"]]
    _finish(a, {"config": {"scenario": "raster", "scene": dict(G=G, V=V, W=W, H=H)}, "cams": cams, "runs": runs})
    import numpy

    numpy.savez_compressed(_grads_path(a.out), **values)


def _grads_path(trace_path):
    return os.path.splitext(trace_path)[0] + ".grads.npz"


def _load(path):
    """the runs of a trace, camera arrays back in their calls"""
    t = json.load(open(path))
    back = lambda x: t["cams"][x["cams"]] if isinstance(x, dict) and list(x) == ["cams"] else x
    return [{**r, "calls": [[back(x) for x in c] for c in r["calls"]]} for r in t["runs"]]


def _close(key, old, new, old2):
    """a value the old tree does not reproduce bit for bit (float atomics: the order of the additions changes from process to process): the new
    tree's must lie as close to the old one's as the old tree's second trace does.  Bound on the largest element-wise difference: 8 x the
    old / old2 one, and for that at least one unit in the last place of the tensor's largest magnitude (2^-23 max|old|), so that a single
    last-bit disagreement of the two old traces does not ask for bit equality.  Both differences are draws of the same reordering error, so
    they agree to a small factor; a gradient that is scaled, swapped with another, stale or left unwritten is off by the order of its own
    magnitude, 10^5 times the bound and more.  -> None, or what is wrong"""
    import numpy as np

    if key not in old.files or key not in new.files or key not in old2.files:
        return "no saved value to compare"
    o, n, o2 = (f[key].astype(np.float64) for f in (old, new, old2))
    if not (o.shape == n.shape == o2.shape):
        return f"shapes {o.shape} / {n.shape}"
    bound = 8.0 * max(np.abs(o - o2).max(initial=0.0), 2.0 ** -23 * np.abs(o).max(initial=0.0))
    d = np.abs(o - n).max(initial=0.0)
    return None if d <= bound else f"max |old - new| = {d:.3e} > {bound:.3e} = 8 x max(max |old - old2|, 2^-23 max |old|)"  # (NaN fails too)


def diff(pa, pb, repeat=None):
    ra, rb = _load(pa), _load(pb)
    rr = _load(repeat) if repeat else ra
    saved = None
    if not [x.get("name") for x in ra] == [y.get("name") for y in rb] == [z.get("name") for z in rr]:
        print(f"not the same runs: {len(ra)} vs {len(rb)}" + (f" vs {len(rr)}" if repeat else ""))
        return 1
    rc, excused = 0, 0
    for i, (x, y, z) in enumerate(zip(ra, rb, rr)):
        run = f"run {i}" + (f" ({x['name']})" if "name" in x else "")
        if repeat and x["calls"] != z["calls"]:
            print(f"{run}: {pa} and {repeat} do not make the same calls: not two traces of one tree")
            return 1
        differs = lambda u: [k for k in sorted(set(x["hashes"]) | set(u["hashes"])) if x["hashes"].get(k) != u["hashes"].get(k)]
        loose = differs(z)  # not reproducible between two traces of the old tree itself
        bad = [k for k in differs(y) if k not in loose]
        excused += len(loose)
        for k in loose:  # compared by value, within the bound of _close
            if saved is None:
                import numpy

                saved = [numpy.load(_grads_path(q)) for q in (pa, pb, repeat)]
            wrong = _close(f"{x['name']}/{k}", *saved)
            if wrong:
                print(f"{run}: {k}: {wrong}")
                rc = 1
        if bad:
            print(f"{run}: output hashes differ: {bad}")
        for j, (cx, cy) in enumerate(zip(x["calls"], y["calls"])):
            if cx != cy:
                print(f"{run}, call {j} differs:\n  {pa}: {cx}\n  {pb}: {cy}")
                return 1
        if len(x["calls"]) != len(y["calls"]):
            print(f"{run}: {len(x['calls'])} vs {len(y['calls'])} calls")
            return 1
        rc |= bool(bad)
    if not rc:
        print(f"equal: {[len(r['calls']) for r in ra]} calls, {sum(len(r['hashes']) for r in ra) - excused} output hashes in {len(ra)} runs"
              + (f"; {excused} values that the old tree does not reproduce bit for bit are within 8 x its own disagreement" if excused else ""))
    return rc


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--diff", nargs=2, metavar="JSON")
    ap.add_argument("--repeat", metavar="JSON", help="with --diff: a second trace of the old tree")
    ap.add_argument("--out", default="launch_trace.json")
    ap.add_argument("--tree")
    ap.add_argument("--scenario", default="forward", choices=["forward", "raster"])
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[128, 128], metavar=("H", "W"))
    ap.add_argument("--time", type=int, default=0)
    args = ap.parse_args()
    sys.exit(diff(*args.diff, repeat=args.repeat) if args.diff else run_raster(args) if args.scenario == "raster" else run(args))
