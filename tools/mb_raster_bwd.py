"""K2 rasterizer forward / backward micro-benchmark: milliseconds per frame of the no-grad forward, the grad forward and the backward
(composite backward + projection backward + pose reduction), with the float-atomic bytes of the composite backward against the chip-wide
atomic rate (~1.3 TB/s).
  python tools/mb_raster_bwd.py pair [views]   pixel-aligned 2 x 512^2 Gaussians (524,288) -> `views` 512^2 views, one call
  python tools/mb_raster_bwd.py stress         ~2.1 M random Gaussians, one 1080p frame (SH degree 4, band 4 off)
"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from siu3r_amd import cuda_splatting as cs, raster, synthetic

mode = sys.argv[1] if len(sys.argv) > 1 else "pair"


def timed(fn, n=10):
    for _ in range(2):
        o = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        o = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, o


if mode == "stress":
    G, W, H = 2_097_152, 1920, 1080
    means, cov, opac, sh = (t.cuda() for t in synthetic.random_scene(G, seed=1, spread=3.0, depth=(2.0, 9.0), scale=(0.004, 0.03)))
    c2w = synthetic.perturbed_camera(0, jitter=0.1)
    w2c = torch.linalg.inv(c2w)
    fx = 0.9 * W
    fovx, fovy = 2 * math.atan(W / (2 * fx)), 2 * math.atan(H / (2 * fx))
    proj = cs.get_projection_matrix(torch.tensor([0.1]), torch.tensor([100.0]), torch.tensor([fovx]), torch.tensor([fovy]))[0]
    cams = [raster.make_cam_k2(w2c, proj @ w2c, math.tan(fovx / 2), math.tan(fovy / 2), c2w[:3, 3], torch.zeros(3), W, H, sh_degree=4)]
    V, args = 1, (means, cov, sh, opac)
else:
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    H = W = 512
    means, cov, opac, sh = (t.cuda() for t in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
    G = means.shape[0]
    ext = synthetic.target_views(V)
    K = synthetic.default_intrinsics()[None].repeat(V, 1, 1)
    fov = cs.get_fov(K)
    tan = (0.5 * fov).tan()
    proj = cs.get_projection_matrix(torch.full((V,), 1.0), torch.full((V,), 1000.0), fov[:, 0], fov[:, 1])
    cams = []
    for v in range(V):
        e = ext[v].clone()
        e[:3, 3] *= 10.0
        w2c = torch.linalg.inv(e)
        cams.append(raster.make_cam_k2(w2c, proj[v] @ w2c, float(tan[v, 0]), float(tan[v, 1]), e[:3, 3].tolist(), [0, 0, 0], W, H, sh_degree=4))
    args = (means * 10.0, cov * 100.0, sh, opac)

kw = dict(sh_planar=sh.shape[-1] == 25 and sh.dim() == 3 and sh.shape[1] == 3)
ms_fwd, o = timed(lambda: raster.rasterize_views_k2(cams, *args, **kw))
leaves = [t.detach().clone().requires_grad_() for t in args]
xi = torch.zeros(V, 6, device="cuda", requires_grad=True)
ms_gfwd, og = timed(lambda: raster.rasterize_views_k2(cams, *leaves, pose_delta=xi, **kw))
gi, gd, go = torch.randn_like(og["image"]), torch.randn_like(og["depth"]), torch.randn_like(og["opacity"])


def fwd_bwd():
    out = raster.rasterize_views_k2(cams, *leaves, pose_delta=xi, **kw)
    return torch.autograd.grad((out["image"], out["depth"], out["opacity"]), leaves + [xi], (gi, gd, go))


ms_fb, _ = timed(fwd_bwd)
ms_bwd = ms_fb - ms_gfwd
D = og["state"].totals(1)
atomic_bytes = sum(D) * 10 * 4  # upper bound: ten fp32 terms per (tile, Gaussian) pair
print(f"{mode} G={G} views={V} {W}x{H}: forward (no grad) {ms_fwd / V:.3f} ms/frame, forward (grad) {ms_gfwd / V:.3f}, backward {ms_bwd / V:.3f} "
      f"ms/frame = {ms_bwd / ms_fwd:.2f} x forward; pairs {D}, atomic bytes <= {atomic_bytes / 1e6:.1f} MB = {atomic_bytes / 1.3e12 * 1e3:.3f} ms at 1.3 TB/s")
