"""Fused depth smoothness (csrc/depth_smooth.hip) against a composed float32 torch term on the same board in the same process: milliseconds
of a whole call, value + gradients, alternating the two, both orders and both spaces with a block-segment map, with the algorithmic bytes
(render space: depth and ids read, one gradient plane written; expected space: three planes read, two written) as a fraction of the 8 TB/s
HBM peak; then one refine_gaussians iteration with and without the term.  Results go to profiles/depth_smooth_timing.json.
  python tools/mb_depth_smooth.py              6 x 512 x 512, 1 x 1080 x 1920 and the refinement iteration
  python tools/mb_depth_smooth.py V H W        one size, no refinement, nothing written
The refinement scene is synthetic.pixel_aligned_scene (2 x 512^2 = 524,288 Gaussians, SH degree 4) seen from 6 views at 512^2, as in
tools/mb_depth_loss.py; the segments are 64 x 64 pixel blocks."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from siu3r_amd import losses, refine, synthetic
from siu3r_amd.smooth import DepthSmoothness

assert torch.cuda.is_available(), "mb_depth_smooth.py measures on the GPU"
props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} uuid {getattr(props, 'uuid', 'n/a')}")


def blocks(V, H, W, size=64):
    """int32 [V,H,W]: one id per size x size block, 2 % of the pixels void"""
    yy, xx = torch.arange(H, device="cuda")[:, None] // size, torch.arange(W, device="cuda")[None, :] // size
    s = (yy * ((W + size - 1) // size) + xx).int()[None].repeat(V, 1, 1)
    s[torch.rand(V, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) < 0.02] = -1
    return s


def fused(d, o, s, order, space):
    d.grad = o.grad = None
    losses.depth_smoothness(d, o, s, order, space).backward()
    return d.grad, o.grad


def composed(d, o, s, order, space):
    """float32 torch, as a caller would compose the term without a host read: x, the usable mask folded into the ids, one diff and one mask
    per axis, two abs().mean()"""
    d.grad = o.grad = None
    if space == "expected":
        ok = (o > 0.5) & (d > 0) & torch.isfinite(d) & torch.isfinite(o)
        x = torch.where(ok, d, torch.ones_like(d)) / torch.where(ok, o, torch.ones_like(o))
    else:
        ok = torch.isfinite(d)
        x = torch.where(ok, d, torch.zeros_like(d))
    ids = torch.where(ok, s, torch.full_like(s, -1))
    loss = 0.0
    for dim in (2, 1):
        n = x.shape[dim]
        sl = lambda a, lo: a.narrow(dim, lo, n - order)
        if order == 1:
            t, act = sl(x, 1) - sl(x, 0), (sl(ids, 0) >= 0) & (sl(ids, 1) == sl(ids, 0))
        else:
            t, act = sl(x, 0) - 2 * sl(x, 1) + sl(x, 2), (sl(ids, 1) >= 0) & (sl(ids, 0) == sl(ids, 1)) & (sl(ids, 2) == sl(ids, 1))
        loss = loss + (t * act).abs().mean()
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
    g = torch.Generator(device="cuda").manual_seed(1)
    yy, xx = torch.arange(H, device="cuda", dtype=torch.float32)[:, None], torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    dhat = 2.0 + 0.004 * xx + 0.003 * yy + 0.01 * torch.randn(V, H, W, device="cuda", generator=g)
    o = torch.where(torch.rand(V, H, W, device="cuda", generator=g) < 0.8, 0.9 + 0.1 * torch.rand(V, H, W, device="cuda", generator=g),
                    torch.rand(V, H, W, device="cuda", generator=g))
    d = (dhat * o).requires_grad_(True)
    o.requires_grad_(True)
    s = blocks(V, H, W)
    rows = []
    for order in (1, 2):
        for space in ("render", "expected"):
            o_ = o if space == "expected" else o.detach()  # (the render space does not read the opacity: nobody differentiates it there)
            n_g = 2 if space == "expected" else 1
            gf, gc = [x.clone() for x in fused(d, o_, s, order, space)[:n_g]], [x.clone() for x in composed(d, o_, s, order, space)[:n_g]]
            err = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(gf, gc))
            # the float32 composition rounds x = D / O, so the sign of a term within rounding of zero can differ from the kernel's float64 one:
            # such an element is off by a whole c / n, and the share of elements that differ at all is the telling figure
            share = max(float(((a - b).abs() > 1e-6 * b.abs().max()).float().mean()) for a, b in zip(gf, gc))
            ms_f, ms_c = alternate((fused, composed), (d, o_, s, order, space), n=40)
            planes = 5 if space == "expected" else 3
            byt = planes * d.numel() * 4
            f, c = min(ms_f), min(ms_c)
            print(f"order {order} {space} {V} x {H} x {W}: fused {f:.4f} ms (turns {' '.join(f'{x:.4f}' for x in ms_f)}), composed torch {c:.4f} ms "
                  f"(turns {' '.join(f'{x:.4f}' for x in ms_c)}) = {c / f:.1f} x; algorithmic bytes {byt / 1e6:.1f} MB = {byt / 8e12 * 1e3:.4f} ms at 8 TB/s "
                  f"-> fused at {byt / 8e12 * 1e3 / f * 100:.1f} % of the HBM peak; gradients against the float32 composition: largest difference {err:.1e} (max-normalised), "
                  f"{share * 100:.4f} % of the elements differ by more than 1e-6")
            rows.append(dict(shape=[V, H, W], order=order, space=space, fused_ms=f, fused_turns_ms=ms_f, composed_ms=c, composed_turns_ms=ms_c, ratio=c / f,
                             algorithmic_bytes=byt, hbm_peak_fraction=byt / 8e12 * 1e3 / f, gradient_max_difference=err, gradient_share_differing=share))
    return rows


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
    segments = blocks(V, H, W)

    def run(iters, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refine.refine_gaussians(means, scales, rot, opac, sh, targets, c2w, K, 0.5, 100.0, (0, 0, 0), iters=iters, log_every=0, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    variants = {"photometric only": {}, "+ smoothness order 1 render": dict(smooth=DepthSmoothness(), segments=segments),
                "+ smoothness order 2 expected": dict(smooth=DepthSmoothness(order=2, space="expected"), segments=segments)}
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
    rows = loss_size(6, 512, 512) + loss_size(1, 1080, 1920)
    ms = refine_iteration()
    print("refine_gaussians iteration, pair scene (524,288 Gaussians, 6 views 512^2), host clock around 20 iterations ending in a synchronise, "
          "three alternating turns: " + "; ".join(f"{k} {min(v):.2f} ms (turns {' '.join(f'{x:.2f}' for x in v)})" for k, v in ms.items()))
    out = dict(device=props.name, uuid=str(getattr(props, "uuid", "n/a")), torch=torch.__version__, calls=rows,
               refine_iteration_ms={k: dict(best=min(v), turns=v) for k, v in ms.items()},
               method="device events around 40 warm calls per turn, 5 alternating turns, best turn; refinement: host clock around 20 iterations, 3 turns")
    path = os.path.join(ROOT, "profiles", "depth_smooth_timing.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {path}")
