"""What the blend-contribution statistics cost, written to profiles/contrib_timing.json: microseconds per call of siu3r_raster_contrib (all
three statistics, and wmax alone) against siu3r_raster_composite_rgb with n_touched -- the same walk plus the colours: the yardstick --
on synthetic.pixel_aligned_scene (2 x 512^2 = 524,288 Gaussians) seen from six 512 x 512 views, on the state of ONE forward call.
Every call sits between its own pair of device events, warm; 40 calls per contender in five turns of eight, the contenders alternating
turn by turn inside one process; the record keeps every sample, the medians and the ratio of the medians.  With --parent the yardstick
is the PARENT commit's library, loaded next to this tree's and run in the same turns on the same buffers (`composite_rgb_nt`); without
it, this tree's (the same source file).
  python tools/mb_contrib.py [--parent PATH] [--out FILE]     PATH: a built checkout of the parent commit
The ratio is reported, not bounded: a pruning event runs a handful of times per refinement."""
import ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
parent = os.path.abspath(args[args.index("--parent") + 1]) if "--parent" in args else None
sys.path.insert(0, ROOT)
import torch
from siu3r_amd import _lib, cuda_splatting as cs, raster, synthetic
from siu3r_amd.ops import _p, _stream

assert torch.cuda.is_available(), "mb_contrib.py measures on the GPU"
props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} {props.uuid}")
record = {"device": props.name, "gpu_uuid": str(props.uuid)}

V, H, W = 6, 512, 512
means, cov, opac, sh = (t.cuda() for t in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
G = means.shape[0]
ext = synthetic.target_views(V)
Kn = synthetic.default_intrinsics()[None].repeat(V, 1, 1)
fov = cs.get_fov(Kn)
tan = (0.5 * fov).tan()
proj = cs.get_projection_matrix(torch.full((V,), 1.0), torch.full((V,), 1000.0), fov[:, 0], fov[:, 1])
cams = []
for v in range(V):
    e = ext[v].clone()
    e[:3, 3] *= 10.0
    w2c = torch.linalg.inv(e)
    cams.append(raster.make_cam_k2(w2c, proj[v] @ w2c, float(tan[v, 0]), float(tan[v, 1]), e[:3, 3].tolist(), [0, 0, 0], W, H, sh_degree=4))
with torch.no_grad():
    o = raster.rasterize_views_k2(cams, means * 10.0, cov * 100.0, sh, opac, sh_planar=sh.dim() == 3 and sh.shape[1] == 3 and sh.shape[-1] == 25)
st = o["state"]
state = (st.cams, V, _p(st.cams_dev), G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec))
image, depth, alpha, nt = (torch.empty_like(o[k]) for k in ("image", "depth", "opacity", "n_touched"))
wmax, count, wsum = torch.empty((V, G), device="cuda"), torch.empty((V, G), dtype=torch.int32, device="cuda"), torch.empty((V, G), dtype=torch.int64, device="cuda")
wmax_only = torch.empty((V, G), device="cuda")
lib = _lib.lib()
ylib = lib
if parent:
    ylib = ctypes.CDLL(os.path.join(parent, "siu3r_amd", "libsiu3r_hip.so"))
    assert not hasattr(ylib, "siu3r_raster_contrib"), "--parent names a tree that already has the statistics"
    ylib.siu3r_raster_composite_rgb.argtypes = _lib.SIGNATURES["siu3r_raster_composite_rgb"]
contenders = {"composite_rgb_nt": lambda: _lib.check(ylib.siu3r_raster_composite_rgb(*state, _p(image), _p(depth), _p(alpha), _p(nt), _stream())),
              "contrib": lambda: _lib.check(lib.siu3r_raster_contrib(*state, _p(wmax), _p(count), _p(wsum), _stream())),
              "contrib_wmax_only": lambda: _lib.check(lib.siu3r_raster_contrib(*state, _p(wmax_only), None, None, _stream()))}


def event_turns(fns, n=8, turns=5):
    """every call between its own pair of device events, warm: {name: [us per call, n per turn, the contenders alternating turn by turn]}"""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(turns):
        for k, fn in fns.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            ev[0].record()
            for i in range(n):
                fn()
                ev[i + 1].record()
            ev[n].synchronize()
            out[k] += [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(n)]
    return out


us = event_turns(contenders)
med = {k: statistics.median(v) for k, v in us.items()}
record["yardstick_library"] = "the parent commit's" if parent else "this tree's (csrc/raster.hip is the parent's file)"
record["us_per_call"] = {k: {"median": med[k], "min": min(v), "max": max(v), "samples": v} for k, v in us.items()}
record["ratio_of_medians"] = {"contrib / composite_rgb_nt": med["contrib"] / med["composite_rgb_nt"],
                              "contrib_wmax_only / composite_rgb_nt": med["contrib_wmax_only"] / med["composite_rgb_nt"]}
record["scene"] = (f"synthetic.pixel_aligned_scene(512, 512, 2, seed=0): {G} Gaussians, {V} views {W} x {H}, {sum(st.totals(1))} (tile, Gaussian) pairs; the clears of "
                   "the outputs are inside the calls; 40 calls per contender, each between its own device events, in 5 alternating turns of 8 after 5 warm calls each")
assert torch.equal(image, o["image"]) and torch.equal(nt, o["n_touched"]), "the yardstick reproduces the forward it was taken from"
assert torch.equal(wmax.view(torch.int32), wmax_only.view(torch.int32))
blended = count > 0
record["statistics"] = {"rows_that_blend_in_some_view": int(blended.any(0).sum()), "rows": G, "blended_pixel_entries": int(count.sum()),
                        "share_of_rows_with_wmax_below_0.01_in_every_view": float((wmax.amax(0) < 0.01).float().mean()),
                        "weight_sum_total": float(wsum.sum().double() * 2.0 ** -40),
                        "alpha_sum_of_the_render": float(o["opacity"].double().sum())}
for k, v in us.items():
    print(f"{k}: median {med[k]:.1f} us, min {min(v):.1f}, max {max(v):.1f} over {len(v)} calls")
print(record["ratio_of_medians"], record["statistics"])
path = os.path.abspath(args[args.index("--out") + 1]) if "--out" in args else os.path.join(ROOT, "profiles", "contrib_timing.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
print("wrote", path)
