"""Dense restatement of adaptive density control (Kerbl et al. 2023, section 5.2) in plain torch, float64 by default: accumulate, plan and
apply written from the rules, not from csrc/density.hip.  Runs on any device; `dtype=torch.float32` gives the same restatement in float32
(the yardstick of the float32 error bars)."""
import math

import torch

PRUNE, KEEP, CLONE, SPLIT = 0, 1, 2, 3
LOG_SPLIT = math.log(1.6)  # children have scale / (0.8 * 2)


def accumulate(g_mean2d, radii, sx, sy, grad_accum, seen, max_radius, dtype=torch.float64):
    """g_mean2d [V,G,2], radii [V,G,2] int, running grad_accum / seen / max_radius [G] -> the three new arrays; views in index order;
    a view counts when either radius is positive, whatever the gradient row holds"""
    acc, n, rmax = grad_accum.to(dtype).clone(), seen.long().clone(), max_radius.long().clone()
    sx, sy = torch.tensor(sx, dtype=dtype), torch.tensor(sy, dtype=dtype)
    for v in range(g_mean2d.shape[0]):
        vis = (radii[v, :, 0] > 0) | (radii[v, :, 1] > 0)
        g = g_mean2d[v].to(dtype)
        norm = torch.hypot(sx * g[:, 0], sy * g[:, 1])
        acc = torch.where(vis, acc + norm, acc)
        n = n + vis.long()
        rmax = torch.where(vis, torch.maximum(rmax, radii[v].long().max(-1).values), rmax)
    return acc, n, rmax


def plan(grad_accum, seen, max_radius, log_scales, logit_opacity, grad_threshold, log_dense_scale, logit_min_opacity, max_screen_radius=0,
         log_max_world_scale=math.inf, grow=True):
    """-> action [G], offset [G] (exclusive scan of the output rows), totals (rows out, pruned, cloned, split).  The thresholds are
    float32-representable numbers; every comparison is exact in float64"""
    ga, n = grad_accum.double(), seen.double()
    avg = torch.where(seen > 0, ga / n.clamp(min=1.0), torch.zeros_like(ga))
    hot = avg >= grad_threshold
    top = log_scales.double().max(-1).values
    big = top > log_dense_scale
    prune = logit_opacity.double() < logit_min_opacity
    if max_screen_radius > 0:
        prune = prune | (max_radius > max_screen_radius)
    prune = prune | (top > log_max_world_scale)
    action = torch.full_like(seen, KEEP, dtype=torch.long)
    if grow:
        action[hot] = CLONE
        action[hot & big] = SPLIT
    action[prune] = PRUNE
    count = action.clamp(max=2)
    offset = torch.cumsum(count, 0) - count
    totals = (int(count.sum()), int((action == PRUNE).sum()), int((action == CLONE).sum()), int((action == SPLIT).sum()))
    return action, offset, totals


def rotation(q_xyzw):
    """R(q / |q|) of raw (x, y, z, w) quaternions -> [G,3,3]"""
    q = q_xyzw / q_xyzw.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).view(-1, 3, 3)


def apply(params, moments, action, offset, rows_out, noise, dtype=torch.float64):
    """params {field: [G,...]} with "means", "scales" (log), "rotations" (x, y, z, w) among them, moments {field: (m1, m2)} ->
    (new params, new moments) of rows_out rows, in `dtype`"""
    src = torch.arange(action.shape[0], device=action.device)
    first, second = action >= KEEP, action >= CLONE
    split = action == SPLIT
    kids = params["means"].to(dtype)[:, None, :] + torch.einsum("gij,gcj->gci", rotation(params["rotations"].to(dtype)),
                                                                params["scales"].to(dtype).exp()[:, None, :] * noise.to(dtype))
    new_p, new_m = {}, {}
    for k, v in params.items():
        v = v.to(dtype)
        out = torch.zeros((rows_out, *v.shape[1:]), dtype=dtype, device=v.device)
        a, b = v.clone(), v.clone()
        if k == "means":
            a[split], b[split] = kids[split, 0], kids[split, 1]
        elif k == "scales":
            a[split] = b[split] = v[split] - LOG_SPLIT
        out[offset[first]] = a[first]
        out[offset[second] + 1] = b[second]
        new_p[k] = out
        if k in moments:
            ms = []
            for m in moments[k]:
                m = m.to(dtype)
                mo = torch.zeros_like(out)
                carried = first & ~split
                mo[offset[carried]] = m[carried]
                ms.append(mo)
            new_m[k] = tuple(ms)
    return new_p, new_m
