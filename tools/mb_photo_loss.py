"""Fused photometric loss (csrc/photo_loss.hip) against the composed torch loss (tests/dense_photo64.py in float32) on the same board in the
same call: milliseconds of value + gradient, alternating the two, with the algorithmic bytes (read pred, read target, write grad) as a
fraction of the 8 TB/s HBM peak; then the share of one refine_gaussians iteration that the loss takes with each.
  python tools/mb_photo_loss.py              6 x 3 x 512 x 512, 1 x 3 x 1080 x 1920 and the refinement iteration
  python tools/mb_photo_loss.py V H W        one size, no refinement
The refinement scene is synthetic.pixel_aligned_scene (2 x 512^2 = 524,288 Gaussians, SH degree 4) seen from 6 views at 512^2; the scene
generator emits covariances, so scales are the square roots of their diagonals and the quaternions seeded random (the same footprints)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import dense_photo64 as D
from siu3r_amd import losses, refine, synthetic

assert torch.cuda.is_available(), "mb_photo_loss.py measures on the GPU"
LAM = 0.2
props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} uuid {getattr(props, 'uuid', 'n/a')}")


def fused(p, t):
    p.grad = None
    losses.photometric_loss(p, t, LAM).backward()
    return p.grad


def composed(p, t):
    p.grad = None
    D.photo_loss(p, t, LAM)[0].backward()
    return p.grad


def alternate(fns, args, n, rounds=5):
    """event time per call of each function, the functions taking turns `rounds` times (n calls each turn); returns the per-turn means"""
    for f in fns:
        for _ in range(3):
            f(*args)
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                f(*args)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / n)
    return ms


def loss_size(V, H, W):
    g = torch.Generator().manual_seed(0)
    p = torch.rand(V, 3, H, W, generator=g).cuda().requires_grad_(True)
    t = torch.rand(V, 3, H, W, generator=g).cuda()
    gf, gc = fused(p, t).clone(), composed(p, t).clone()
    err = float((gf - gc).abs().max() / gc.abs().max())
    ms_f, ms_c = alternate((fused, composed), (p, t), n=40)
    byt = 3 * p.numel() * 4
    f, c = min(ms_f), min(ms_c)
    print(f"{V} x 3 x {H} x {W}: fused {f:.4f} ms (turns {' '.join(f'{x:.4f}' for x in ms_f)}), composed torch {c:.4f} ms "
          f"(turns {' '.join(f'{x:.4f}' for x in ms_c)}) = {c / f:.1f} x; algorithmic bytes {byt / 1e6:.1f} MB = {byt / 8e12 * 1e3:.4f} ms at 8 TB/s "
          f"-> fused at {byt / 8e12 * 1e3 / f * 100:.1f} % of the HBM peak; gradients agree to {err:.1e} (max-normalised)")
    return f, c


def refine_iteration():
    H = W = 512
    V = 6
    means, cov, opac, sh = (x.cuda() for x in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
    G = means.shape[0]
    g = torch.Generator().manual_seed(1)
    scales = torch.diagonal(cov, dim1=1, dim2=2).sqrt().contiguous()
    rot = torch.randn(G, 4, generator=g).cuda()
    c2w = synthetic.target_views(V).cuda()
    K = synthetic.default_intrinsics()[None].repeat(V, 1, 1).cuda()
    targets = torch.rand(V, 3, H, W, generator=g).cuda()
    real = refine.photometric_loss

    def run(loss_fn, iters):
        refine.photometric_loss = loss_fn
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            refine.refine_gaussians(means, scales, rot, opac, sh, targets, c2w, K, 0.5, 100.0, (0, 0, 0), iters=iters, lambda_dssim=LAM, log_every=0)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e3
        finally:
            refine.photometric_loss = real

    comp = lambda img, tgt, lam: D.photo_loss(img, tgt, lam)[0]
    run(real, 3), run(comp, 3)
    ms = {"fused": [], "composed": []}
    for _ in range(3):
        ms["fused"].append(run(real, 20))
        ms["composed"].append(run(comp, 20))
    return min(ms["fused"]), min(ms["composed"]), ms


if len(sys.argv) > 3:
    loss_size(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
else:
    f, c = loss_size(6, 512, 512)
    loss_size(1, 1080, 1920)
    it_f, it_c, ms = refine_iteration()
    print(f"refine_gaussians iteration, pair scene (524,288 Gaussians, 6 views 512^2): {it_f:.2f} ms with the fused loss, {it_c:.2f} ms with the composed "
          f"loss (turns {ms}); the loss (value + gradient, 6 x 3 x 512 x 512 above) is {f / it_f * 100:.1f} % of the iteration fused, "
          f"{c / it_c * 100:.1f} % composed")
