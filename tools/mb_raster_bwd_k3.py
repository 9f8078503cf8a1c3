"""gsplat-family (K3) rasterizer forward / backward micro-benchmark: milliseconds per frame of the no-grad forward, the grad forward and
the backward, with an upper bound of the float-atomic bytes of the composite backward against the chip-wide atomic rate (~1.3 TB/s).
  python tools/mb_raster_bwd_k3.py pair [C] [views]  pixel-aligned 2 x 512^2 Gaussians -> `views` 512^2 views in one call, C channels (168)
  python tools/mb_raster_bwd_k3.py stress            ~2.1 M random Gaussians, one 1080p frame, C = 3 (the fused three-channel path)
  python tools/mb_raster_bwd_k3.py viewer            the stress scene through compat.gsplat.rasterization with SH degree 3 (quats, scales, SH)
"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from siu3r_amd import raster, synthetic
from siu3r_amd.compat.gsplat import rasterization

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


def report(name, V, ms_fwd, ms_gfwd, ms_fb, pairs, C):
    """pairs: the listed (quadrant, entry) pairs of the N-channel path, or the (tile, Gaussian) pairs of the three-channel path"""
    ms_bwd = ms_fb - ms_gfwd
    # upper bound: at most C feature gradients + six screen-space terms per listed (quadrant, entry) pair (N channels), at most ten terms per
    # (tile, Gaussian) pair (three channels), 4 B each
    ab = pairs * 4 * (C + 6) if C > 3 else pairs * 10 * 4
    kind = "quadrant pairs" if C > 3 else "tile pairs"
    print(f"{name} views={V} C={C}: forward (no grad) {ms_fwd / V:.3f} ms/frame, forward (grad) {ms_gfwd / V:.3f}, backward {ms_bwd / V:.3f} ms/frame "
          f"= {ms_bwd / ms_fwd:.2f} x forward; {kind} {pairs}, atomic bytes <= {ab / 1e6 / V:.1f} MB/frame = {ab / V / 1.3e12 * 1e3:.3f} ms/frame at 1.3 TB/s",
          flush=True)


if mode == "pair":
    C = int(sys.argv[2]) if len(sys.argv) > 2 else 168
    V = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    H = W = 512
    means, cov, opac, _ = (t.cuda() for t in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
    ext = synthetic.target_views(V)
    ext[:, :3, 3] *= 10.0
    Kt = synthetic.default_intrinsics()
    cams = []
    for j in range(V):
        Kp = Kt.clone(); Kp[0, :] *= W; Kp[1, :] *= H
        cams.append(raster.make_cam_k3(torch.linalg.inv(ext[j]), Kp[0, 0], Kp[1, 1], Kp[0, 2], Kp[1, 2], W, H, near_plane=1.0, far_plane=1000.0))
    feats = torch.randn(means.shape[0], C, generator=torch.Generator().manual_seed(5)).cuda()
    args = [(means * 10.0).contiguous(), (cov * 100.0).contiguous(), opac, feats]
    ms_fwd, o = timed(lambda: raster.rasterize_views_k3(cams, *args))
    leaves = [t.detach().clone().requires_grad_() for t in args]
    ms_gfwd, og = timed(lambda: raster.rasterize_views_k3(cams, *leaves))
    gc, ga = torch.randn_like(og["colors"]), torch.randn_like(og["alphas"])

    def fwd_bwd():
        out = raster.rasterize_views_k3(cams, *leaves)
        return torch.autograd.grad((out["colors"], out["alphas"]), leaves, (gc, ga))

    ms_fb, _ = timed(fwd_bwd)
    st = og["state"]
    # the listed (quadrant, entry) pairs: qcnt [V, T, 4] behind the V * 4 * cap_d ids of the workspace (C >= 32: the forward's lists)
    assert st["feat_ws_lists"]
    nq = st["V"] * 4 * st["cap_d"]
    pairs = int(st["feat_ws"][nq:nq + st["V"] * st["T"] * 4].long().sum())
    tile_pairs = int(st["tile_start_all"][:, st["T"]].sum())
    print(f"tile pairs {tile_pairs}, quadrant pairs {pairs} = {pairs / tile_pairs:.2f} per tile pair")
    report("pair", V, ms_fwd, ms_gfwd, ms_fb, pairs, C)
else:
    G, W, H = 2_097_152, 1920, 1080
    means, cov, opac, sh = (t.cuda() for t in synthetic.random_scene(G, seed=1, spread=3.0, depth=(2.0, 9.0), scale=(0.004, 0.03)))
    c2w = synthetic.perturbed_camera(0, jitter=0.1)
    fx = 0.9 * W
    vm = torch.linalg.inv(c2w)[None].cuda()
    Ks = torch.tensor([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=torch.float32)[None].cuda()
    cov6 = raster.cov6_from_cov3x3(cov)
    if mode == "stress":
        rgb = torch.rand(G, 3, generator=torch.Generator().manual_seed(2)).cuda()
        args = [means, cov6, opac, rgb]
        cams = [raster.make_cam_k3(vm[0].cpu(), fx, fx, W / 2, H / 2, W, H)]
        run = lambda a: raster.rasterize_views_k3_rgb(cams, *a, pose_dev=(vm, Ks))
        outs = lambda o: (o["colors"], o["alphas"])
    else:
        quats = torch.randn(G, 4, generator=torch.Generator().manual_seed(3)).cuda()
        scales = (0.004 + 0.026 * torch.rand(G, 3, generator=torch.Generator().manual_seed(4))).cuda()
        shc = sh.permute(0, 2, 1)[:, :16].contiguous()
        args = [means, quats, scales, opac, shc]
        bg = torch.ones(3, device="cuda")
        run = lambda a: rasterization(a[0], a[1], a[2], a[3], a[4], vm, Ks, W, H, sh_degree=3, backgrounds=bg)
        outs = lambda o: (o[0], o[1])
    ms_fwd, _ = timed(lambda: run(args))
    leaves = [t.detach().clone().requires_grad_() for t in args]
    ms_gfwd, og = timed(lambda: run(leaves))
    gouts = [torch.randn_like(t) for t in outs(og)]

    def fwd_bwd():
        return torch.autograd.grad(outs(run(leaves)), leaves, gouts)

    ms_fb, _ = timed(fwd_bwd)
    with torch.no_grad():
        st = raster.rasterize_views_k3_rgb([raster.make_cam_k3(vm[0].cpu(), fx, fx, W / 2, H / 2, W, H)], means, cov6, opac,
                                           torch.zeros(G, 3, device="cuda"), pose_dev=(vm, Ks))["state"]
    report(mode, 1, ms_fwd, ms_gfwd, ms_fb, sum(st.totals(1)), 3)
