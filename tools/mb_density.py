"""Density control (csrc/density.hip) timed on the board: device events, the candidates taking turns in one process.
  1. one siu3r_density_accumulate at V = 6, G = 524,288 (the pair scene of tools/mb_photo_loss.py), with its algorithmic bytes;
  2. one full event, density.densify_and_prune = plan + apply over the five fields and their ten Adam moment tensors (SH degree 4: rows of
     3, 3, 4, 1 and 75 floats), against the same event composed in torch the way 3DGS's densify does it (boolean masks, `cat`, `repeat`:
     survivors first, then the clone copies, then the split children -- it does NOT keep the memory order).  Both read their row count
     back once; both leave the same multiset of rows.
  python tools/mb_density.py [G]"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from siu3r_amd import density

assert torch.cuda.is_available(), "mb_density.py measures on the GPU"
G = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
V, N_SH = 6, 25
FIELDS = density.FIELDS
props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} uuid {getattr(props, 'uuid', 'n/a')}")


def alternate(fns, n, rounds=5):
    """event time per call of each function, the functions taking turns `rounds` times (n calls each turn); returns the per-turn means"""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / n)
    return ms


g = torch.Generator().manual_seed(0)
r = lambda *s: torch.rand(*s, generator=g)

# ---- 1. accumulate
g2d = (torch.randn(V, G, 2, generator=g) * 1e-5).cuda()
radii = torch.randint(0, 12, (V, G, 2), generator=g, dtype=torch.int32)
radii[r(V, G) < 0.4] = 0
radii = radii.cuda()
stats = density.DensityStats(G, "cuda")
acc = lambda: stats.accumulate(g2d, radii, V * 512 / 2, V * 512 / 2)


def acc_torch():
    vis = (radii > 0).any(-1)
    norm = torch.hypot(g2d[..., 0] * (V * 512 / 2), g2d[..., 1] * (V * 512 / 2))
    stats.grad_accum.add_(torch.where(vis, norm, torch.zeros_like(norm)).sum(0))
    stats.seen.add_(vis.sum(0, dtype=torch.int32))
    torch.maximum(stats.max_radius, torch.where(vis[..., None], radii, torch.zeros_like(radii)).amax((0, 2)), out=stats.max_radius)


ms_a, ms_t = alternate((acc, acc_torch), n=50)
byt = V * G * 16 + G * 24  # gradient + radii rows of every view, the three running arrays read and written
print(f"accumulate V={V} G={G}: kernel {min(ms_a) * 1e3:.1f} us (turns {' '.join(f'{x * 1e3:.1f}' for x in ms_a)}), composed torch {min(ms_t) * 1e3:.1f} us "
      f"(turns {' '.join(f'{x * 1e3:.1f}' for x in ms_t)}); algorithmic bytes {byt / 1e6:.1f} MB = {byt / 8e12 * 1e6:.1f} us at 8 TB/s "
      f"-> {byt / 8e12 * 1e3 / min(ms_a) * 100:.1f} % of the HBM peak (launch included)")

# ---- 2. one event
p = dict(means=torch.randn(G, 3, generator=g) * 2, scales=torch.log(0.005 + 0.05 * r(G, 3)), rotations=torch.randn(G, 4, generator=g),
         opacities=torch.randn(G, generator=g) * 3, harmonics=torch.randn(G, 3, N_SH, generator=g))
p = {k: v.cuda() for k, v in p.items()}
m = {k: (torch.randn(p[k].shape, generator=g).cuda(), r(*p[k].shape).cuda()) for k in FIELDS}
noise = torch.randn(G, 2, 3, generator=g).cuda()
stats.reset()
stats.seen.copy_(torch.randint(0, 7, (G,), generator=g, dtype=torch.int32))
stats.grad_accum.copy_(r(G) * 4e-4)
stats.grad_accum.mul_(stats.seen)
control = density.DensityControl()
EXTENT = 3.0
thr = control.thresholds(EXTENT)
fused = lambda: density.densify_and_prune(p, m, stats, control, EXTENT, noise)


def rotation(q):
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).view(-1, 3, 3)


def composed():
    avg = torch.where(stats.seen > 0, stats.grad_accum.double() / stats.seen.clamp(min=1), 0.0)  # (fp64 quotient, as the plan kernel)
    hot = avg >= thr["grad_threshold"]
    big = p["scales"].max(-1).values > thr["log_dense_scale"]
    alive = ~(p["opacities"] < thr["logit_min_opacity"])
    clone, split = hot & ~big & alive, hot & big & alive
    stay = alive & ~split
    kids = p["means"][split][:, None, :] + torch.einsum("gij,gcj->gci", rotation(p["rotations"][split]), p["scales"][split].exp()[:, None, :] * noise[split])
    new_p, new_m = {}, {}
    for k in FIELDS:
        if k == "means":
            children = kids.transpose(0, 1).reshape(-1, 3)
        else:
            children = p[k][split].repeat(2, *([1] * (p[k].dim() - 1)))
            if k == "scales":
                children = children - math.log(1.6)
        fresh = torch.cat((p[k][clone], children))
        new_p[k] = torch.cat((p[k][stay], fresh))
        new_m[k] = tuple(torch.cat((x[stay], torch.zeros_like(fresh))) for x in m[k])
    return new_p, new_m, new_p["means"].shape[0]


fp, fm, info = fused()
cp, cm, rows = composed()
assert info["rows_out"] == rows, (info, rows)
for k in FIELDS:  # the same multiset of rows: compare the column sums (the orders differ)
    a, b = fp[k].double().sum(0), cp[k].double().sum(0)
    assert torch.allclose(a, b, rtol=1e-6, atol=1e-3 * float(b.abs().max())), k
ms_f, ms_c = alternate((fused, composed), n=10)
row = sum(p[k][0].numel() for k in FIELDS)  # 86 floats
byt = 3 * row * 4 * (G + rows) + G * (12 + 12 + 4 + 8) + 5 * G * 8
f, c = min(ms_f), min(ms_c)
print(f"event G={G} -> {rows} rows ({info}): fused plan + apply {f:.3f} ms (turns {' '.join(f'{x:.3f}' for x in ms_f)}), composed torch {c:.3f} ms "
      f"(turns {' '.join(f'{x:.3f}' for x in ms_c)}) = {c / f:.1f} x; algorithmic bytes {byt / 1e6:.1f} MB = {byt / 8e12 * 1e3:.3f} ms at 8 TB/s "
      f"-> fused at {byt / 8e12 * 1e3 / f * 100:.1f} % of the HBM peak (eight launches, fifteen output allocations and one host read included)")
