"""What the anti-aliased projection costs, written to profiles/antialias_timing.json: microseconds per call of siu3r_raster_project against
siu3r_raster_project_aa and of siu3r_raster_project_bwd against siu3r_raster_project_bwd_aa on synthetic.pixel_aligned_scene (2 x 512^2 =
524,288 Gaussians) seen from six 512 x 512 views -- the scene of DESIGN.md sections 25 / 26.  Every call sits between its own pair of device
events, warm; 40 calls per contender in five turns of eight, the contenders alternating turn by turn inside one process; the record keeps
every sample, the medians and the ratios of the medians.  With --parent the classic contenders also run from the PARENT commit's library,
loaded next to this tree's, in the same turns on the same buffers.  Also timed: the three 3-D filter entry points on the same scene.
  python tools/mb_antialias.py [--parent PATH] [--out FILE]     PATH: a directory holding the parent commit's siu3r_amd/libsiu3r_hip.so
The ratios are reported, not bounded."""
import ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
parent = os.path.abspath(args[args.index("--parent") + 1]) if "--parent" in args else None
sys.path.insert(0, ROOT)
import torch
from siu3r_amd import _lib, cuda_splatting as cs, mip, raster, synthetic
from siu3r_amd.ops import _p, _stream

assert torch.cuda.is_available(), "mb_antialias.py measures on the GPU"
props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} {props.uuid}")
record = {"device": props.name, "gpu_uuid": str(props.uuid)}

V, H, W = 6, 512, 512
means, cov, opac, sh = (t.cuda() for t in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
means, cov = (means * 10.0).contiguous(), (cov * 100.0).contiguous()
G = means.shape[0]
ext = synthetic.target_views(V)
Kn = synthetic.default_intrinsics()[None].repeat(V, 1, 1)
fov = cs.get_fov(Kn)
tan = (0.5 * fov).tan()
proj = cs.get_projection_matrix(torch.full((V,), 1.0), torch.full((V,), 1000.0), fov[:, 0], fov[:, 1])
cams, c2w = [], []
for v in range(V):
    e = ext[v].clone()
    e[:3, 3] *= 10.0
    c2w.append(e)
    w2c = torch.linalg.inv(e)
    cams.append(raster.make_cam_k2(w2c, proj[v] @ w2c, float(tan[v, 0]), float(tan[v, 1]), e[:3, 3].tolist(), [0, 0, 0], W, H, sh_degree=4))
planar = sh.dim() == 3 and sh.shape[1] == 3 and sh.shape[-1] == 25
sh = sh.contiguous()
ncoef = sh.shape[2] if planar else sh.shape[1]
with torch.no_grad():
    o = raster.rasterize_views_k2(cams, means, cov, sh, opac, sh_planar=planar, antialiased=True)
st = o["state"]
stride = raster._cov_stride(cov)
f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
rec, radii, rect, tiles, keys, stats, comp = f32(V, G, 12), i32(V, G, 2), i32(V, G, 4), i32(V, G), i32(V, G), torch.empty((V, 4), dtype=torch.int64, device="cuda"), f32(V, G)
cams_dev = torch.empty_like(st.cams_dev)
fwd = (st.cams, V, _p(cams_dev), G, _p(means), _p(cov), stride, _p(opac), _p(sh), ncoef, int(planar), _p(rec), _p(radii), _p(rect), _p(tiles), _p(keys), _p(stats))
grad = torch.randn(V, G, raster.GR_N, device="cuda")
g_means, g_cov, g_op, g_sh = torch.empty_like(means), torch.empty_like(cov), torch.empty_like(opac), torch.empty_like(sh)
bwd = (st.cams, V, _p(st.cams_dev), G, _p(means), _p(cov), stride, _p(opac), _p(sh), ncoef, int(planar), _p(st.rect), _p(grad), _p(g_means), _p(g_cov), _p(g_op),
       _p(g_sh), None, None)
lib = _lib.lib()
contenders = {"project": lambda: _lib.check(lib.siu3r_raster_project(*fwd, _stream())),
              "project_aa": lambda: _lib.check(lib.siu3r_raster_project_aa(*fwd, _p(comp), _stream())),
              "project_aa_no_comp": lambda: _lib.check(lib.siu3r_raster_project_aa(*fwd, None, _stream())),
              "project_bwd": lambda: _lib.check(lib.siu3r_raster_project_bwd(*bwd, _stream())),
              "project_bwd_aa": lambda: _lib.check(lib.siu3r_raster_project_bwd_aa(*bwd, _stream()))}
if parent:
    plib = ctypes.CDLL(os.path.join(parent, "siu3r_amd", "libsiu3r_hip.so"))
    assert not hasattr(plib, "siu3r_raster_project_aa"), "--parent names a tree that already has the anti-aliased projection"
    for name in ("siu3r_raster_project", "siu3r_raster_project_bwd"):
        getattr(plib, name).argtypes = _lib.SIGNATURES[name]
    contenders["parent_project"] = lambda: _lib.check(plib.siu3r_raster_project(*fwd, _stream()))
    contenders["parent_project_bwd"] = lambda: _lib.check(plib.siu3r_raster_project_bwd(*bwd, _stream()))
c2w_d, Kn_d = torch.stack(c2w).cuda().contiguous(), Kn.cuda().contiguous()
scales, filt = torch.rand(G, 3, device="cuda") * 0.1 + 0.01, mip.compute_filter3d(means, c2w_d, Kn_d, W, H)
ws = f32(int(lib.siu3r_mip_filter3d_ws(V)) // 4)
sf, of, gs, go = f32(G, 3), f32(G), f32(G, 3), f32(G)
contenders["mip_filter3d"] = lambda: _lib.check(lib.siu3r_mip_filter3d(_p(c2w_d), _p(Kn_d), V, W, H, _p(means), G, 0.2, 0.15, 0.2, _p(filt), _p(ws), _stream()))
contenders["mip_apply"] = lambda: _lib.check(lib.siu3r_mip_apply(_p(scales), _p(opac), _p(filt), G, _p(sf), _p(of), _stream()))
contenders["mip_apply_bwd"] = lambda: _lib.check(lib.siu3r_mip_apply_bwd(_p(scales), _p(opac), _p(filt), _p(sf), _p(of), G, _p(gs), _p(go), _stream()))


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
record["us_per_call"] = {k: {"median": med[k], "min": min(v), "max": max(v), "samples": v} for k, v in us.items()}
ratios = {"project_aa / project": med["project_aa"] / med["project"], "project_aa_no_comp / project": med["project_aa_no_comp"] / med["project"],
          "project_bwd_aa / project_bwd": med["project_bwd_aa"] / med["project_bwd"]}
if parent:
    ratios.update({"project_aa / parent_project": med["project_aa"] / med["parent_project"], "project / parent_project": med["project"] / med["parent_project"],
                   "project_bwd_aa / parent_project_bwd": med["project_bwd_aa"] / med["parent_project_bwd"],
                   "project_bwd / parent_project_bwd": med["project_bwd"] / med["parent_project_bwd"]})
record["ratio_of_medians"] = ratios
record["parent_library"] = bool(parent)
record["scene"] = (f"synthetic.pixel_aligned_scene(512, 512, 2, seed=0): {G} Gaussians, SH [G,{'3,25' if planar else str(ncoef) + ',3'}], {V} views {W} x {H}, host poses; the projection "
                   "calls include their camera upload and counter reset; 40 calls per contender, each between its own device events, in 5 alternating turns of 8 "
                   "after 5 warm calls each")
# the last calls left the classic record in rec: the anti-aliased state of the render is st.rec
_lib.check(lib.siu3r_raster_project_aa(*fwd, _p(comp), _stream()))
torch.cuda.synchronize()
assert torch.equal(rec[..., :8].contiguous().view(torch.int32), st.rec[..., :8].contiguous().view(torch.int32)) and torch.equal(rect, st.rect), \
    "the timed call reproduces the projection of the render"  # (slots 8 .. 11 of a culled row are not written)
live = comp > 0
record["compensation"] = {"visible_pairs": int(live.sum()), "median": float(comp[live].median()), "min": float(comp[live].min()), "max": float(comp[live].max()),
                          "on_the_floor": int((comp[live] <= 0.0050001).sum())}
for k, v in us.items():
    print(f"{k}: median {med[k]:.1f} us, min {min(v):.1f}, max {max(v):.1f} over {len(v)} calls")
print(record["ratio_of_medians"], record["compensation"])
path = os.path.abspath(args[args.index("--out") + 1]) if "--out" in args else os.path.join(ROOT, "profiles", "antialias_timing.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
print("wrote", path)
