"""Fused depth loss (csrc/depth_loss.hip) against the composed torch loss (tests/dense_depth64.py in float32) on the same board in the same
call: milliseconds of value + gradient, alternating the two, both modes, with the algorithmic bytes (every plane once per pass, two gradient
planes written) as a fraction of the 8 TB/s HBM peak; then one refine_gaussians iteration with and without a depth term.
  python tools/mb_depth_loss.py              6 x 512 x 512, 1 x 1080 x 1920 and the refinement iteration
  python tools/mb_depth_loss.py V H W        one size, no refinement
The refinement scene is synthetic.pixel_aligned_scene (2 x 512^2 = 524,288 Gaussians, SH degree 4) seen from 6 views at 512^2, as in
tools/mb_photo_loss.py; the depth target is the scene's own normalised depth before refinement."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import dense_depth64 as D
from siu3r_amd import losses, refine, synthetic

assert torch.cuda.is_available(), "mb_depth_loss.py measures on the GPU"
props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} uuid {getattr(props, 'uuid', 'n/a')}")


def fused(d, o, t, w, mode):
    d.grad = o.grad = None
    losses.depth_loss(d, o, t, w, mode).backward()
    return d.grad, o.grad


def composed(d, o, t, w, mode):
    """float32 torch: l1 as a caller would compose it without a host read (mask, where, sums); pearson through the restatement, whose
    per-view decision which views count reads the host, as a composed loss has to"""
    d.grad = o.grad = None
    if mode == "l1":
        m = D.valid_mask(d, o, t, w, 0.5)
        x, y, ww, _, _ = D._xyw(d, o, t, w, "depth", m)
        loss = (ww * (x - y).abs()).sum() / ww.sum().clamp_min(1e-30)
    else:
        loss = D.terms(d, o, t, w, mode)[0]
    loss.backward()
    return d.grad, o.grad


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
    d, o, t, w = (x.cuda() for x in D.make_inputs("smooth", V, H, W, seed=0, weights=True))
    d.requires_grad_(True), o.requires_grad_(True)
    for mode in ("l1", "pearson"):
        gf, gc = [x.clone() for x in fused(d, o, t, w, mode)], [x.clone() for x in composed(d, o, t, w, mode)]
        err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gf, gc))
        ms_f, ms_c = alternate((fused, composed), (d, o, t, w, mode), n=40)
        passes = 1 if mode == "l1" else 2
        byt = (4 * passes + 2) * d.numel() * 4
        f, c = min(ms_f), min(ms_c)
        print(f"{mode} {V} x {H} x {W}: fused {f:.4f} ms (turns {' '.join(f'{x:.4f}' for x in ms_f)}), composed torch {c:.4f} ms "
              f"(turns {' '.join(f'{x:.4f}' for x in ms_c)}) = {c / f:.1f} x; algorithmic bytes {byt / 1e6:.1f} MB = {byt / 8e12 * 1e3:.4f} ms at 8 TB/s "
              f"-> fused at {byt / 8e12 * 1e3 / f * 100:.1f} % of the HBM peak; gradients agree to {err:.1e} (max-normalised)")


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
    from siu3r_amd.cuda_splatting import render_cuda
    e = lambda x: x[None].expand(V, *x.shape)
    with torch.no_grad():
        _, dep, aux = render_cuda(c2w, K, torch.full((V,), 0.5), torch.full((V,), 100.0), (H, W), torch.zeros(V, 3), e(means),
                                  e(refine.covariances_from(rot, scales)), e(sh), e(opac), return_aux=True)
    opa = torch.cat([a["opacity"] for a in aux])
    depths = torch.where(opa > 0.5, dep / opa.clamp_min(1e-6), torch.zeros_like(dep))

    def run(iters, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refine.refine_gaussians(means, scales, rot, opac, sh, targets, c2w, K, 0.5, 100.0, (0, 0, 0), iters=iters, log_every=0, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    variants = {"photometric only": {}, "+ l1 depth": dict(depths=depths, lambda_depth=1.0),
                "+ pearson depth": dict(depths=depths, lambda_depth=1.0, depth_mode="pearson")}
    for kw in variants.values():
        run(3, **kw)
    ms = {k: [] for k in variants}
    for _ in range(3):
        for k, kw in variants.items():
            ms[k].append(run(20, **kw))
    return ms


if len(sys.argv) > 3:
    loss_size(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
else:
    loss_size(6, 512, 512)
    loss_size(1, 1080, 1920)
    ms = refine_iteration()
    print("refine_gaussians iteration, pair scene (524,288 Gaussians, 6 views 512^2), host clock around 20 iterations ending in a synchronise, "
          "three alternating turns: " + "; ".join(f"{k} {min(v):.2f} ms (turns {' '.join(f'{x:.2f}' for x in v)})" for k, v in ms.items()))
