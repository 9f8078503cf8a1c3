"""Dense restatement of the instance-aware depth smoothness (siu3r_amd/losses.py::depth_smoothness, csrc/depth_smooth.hip) in plain torch,
parametrised by dtype.  float64 is the reference of the GPU tests, float32 the 'composed torch loss' their tolerance is taken from.  Two
routes: `terms` is differentiable (autograd gives the gradient), `closed_form` is the derivative the HIP kernel implements;
tests/test_depth_smooth_ref.py checks one against the other on the CPU.

The term is the depth-smoothness loss of the SIU3R training objective (reference: src/pipeline.py:242-260, src/pipeline_multi.py:247-265):
the differences of the rendered depth of the context views along both image axes, switched off wherever two neighbouring pixels belong to
different panoptic segments or the right / lower one is void (-1), each axis averaged over ALL its difference positions.  Written here from
the definition, not from those lines:

  x = D (space "render", usable iff D is finite) or D / O (space "expected", usable iff O > min_opacity, D > 0, both finite).
  Along an axis, order 1: t = x[j+1] - x[j]; order 2: t = x[j-1] - 2 x[j] + x[j+1].  A term is active iff all its pixels are usable, none
  is void (a negative id) and all carry the same id.  loss = Sx / n_x + Sy / n_y, S = sum |t| over the active terms, n = the number of
  term positions of the axis over all views (an axis without a position adds 0, where the training objective would give NaN)."""
import numpy as np
import torch


def usable_mask(D, O, space, min_opacity):
    if space == "render":
        return torch.isfinite(D)
    if space != "expected":
        raise ValueError(space)
    mo = float(np.float32(min_opacity))  # the kernel compares float32 values
    return (O > mo) & (D > 0) & torch.isfinite(D) & torch.isfinite(O)


def _x(D, O, space, ok):
    """x, dx/dD, dx/dO with harmless values at the unusable pixels"""
    one = torch.ones_like(D)
    Ds = torch.where(ok, D, one)
    if space == "render":
        return Ds, one, torch.zeros_like(D)
    Os = torch.where(ok, O, one)
    return Ds / Os, 1 / Os, -Ds / (Os * Os)


def _ids(ok, S):
    """segment id per pixel, -1 for an unusable or void pixel; no map: one segment"""
    ids = torch.zeros(ok.shape, dtype=torch.int64) if S is None else S.to(torch.int64)
    return torch.where(ok & (ids >= 0), ids, torch.full_like(ids, -1))


def _axis(x, ids, order, dim):
    """(t, active) of every term position along `dim` (an empty tensor when the axis is too short)"""
    n = x.shape[dim]
    if n <= order:
        shape = list(x.shape)
        shape[dim] = 0
        return x.new_zeros(shape), torch.zeros(shape, dtype=torch.bool)
    sl = lambda a, lo: a.narrow(dim, lo, n - order)
    if order == 1:
        t = sl(x, 1) - sl(x, 0)
        act = (sl(ids, 0) >= 0) & (sl(ids, 1) == sl(ids, 0))
    elif order == 2:
        t = sl(x, 0) - 2 * sl(x, 1) + sl(x, 2)
        act = (sl(ids, 1) >= 0) & (sl(ids, 0) == sl(ids, 1)) & (sl(ids, 2) == sl(ids, 1))
    else:
        raise ValueError(order)
    return t, act


def terms(D, O, S=None, order=1, space="render", min_opacity=0.5):
    """differentiable w.r.t. D and O, in their dtype -> (loss 0-d, (x part, y part), per_view [V], active [V,2] int64)"""
    ok = usable_mask(D, O, space, min_opacity)
    x, _, _ = _x(D, O, space, ok)
    ids = _ids(ok, S)
    V = D.shape[0]
    parts, per_view, active = [], torch.zeros(V, dtype=D.dtype), torch.zeros(V, 2, dtype=torch.int64)
    for a, dim in enumerate((2, 1)):
        t, act = _axis(x, ids, order, dim)
        e = torch.where(act, t.abs(), torch.zeros_like(t))
        n = t.numel()
        parts.append(e.sum() / n if n > 0 else (x * 0).sum())
        if n > 0:
            per_view = per_view + e.detach().flatten(1).sum(1) / (n // V)
        active[:, a] = act.flatten(1).sum(1)
    return parts[0] + parts[1], (parts[0].detach(), parts[1].detach()), per_view, active


def term_values(D, O, S=None, order=1, space="render", min_opacity=0.5):
    """[(t, active)] of the x and the y axis, for tests that look at single terms"""
    ok = usable_mask(D, O, space, min_opacity)
    x, _, _ = _x(D, O, space, ok)
    ids = _ids(ok, S)
    return [_axis(x, ids, order, dim) for dim in (2, 1)], x, ok


def closed_form(D, O, S=None, order=1, space="render", min_opacity=0.5):
    """(d loss / dD, d loss / dO) without autograd: the formulas of the kernel (c sign(t) / n_axis gathered per pixel, then the chain)"""
    with torch.no_grad():
        ok = usable_mask(D, O, space, min_opacity)
        x, dxdD, dxdO = _x(D, O, space, ok)
        ids = _ids(ok, S)
        gx = torch.zeros_like(D)
        coef = (-1.0, 1.0) if order == 1 else (1.0, -2.0, 1.0)
        for dim in (2, 1):
            t, act = _axis(x, ids, order, dim)
            if t.numel() == 0:
                continue
            s = torch.where(act, torch.sign(t), torch.zeros_like(t)) / t.numel()
            for k, c in enumerate(coef):
                gx.narrow(dim, k, t.shape[dim]).add_(c * s)
        zero = torch.zeros_like(D)
        live = ok & (ids >= 0)
        return torch.where(live, gx * dxdD, zero), torch.where(live, gx * dxdO, zero)


def loss_and_grad(D, O, S=None, order=1, space="render", min_opacity=0.5, dtype=torch.float64, route="closed"):
    """the inputs converted to `dtype` (an upcast of float32 inputs is exact) -> dict(loss, parts, per_view, active, g_depth, g_opacity);
    route "closed": the gradient by closed_form, "autograd": by torch autograd through `terms`.  O may be None in the render space."""
    auto = route == "autograd"
    Dd = D.detach().to(dtype).clone().requires_grad_(auto)
    Od = (torch.ones_like(D) if O is None else O).detach().to(dtype).clone().requires_grad_(auto)
    loss, parts, per_view, active = terms(Dd, Od, S, order, space, min_opacity)
    if auto:
        gD, gO = torch.autograd.grad(loss, (Dd, Od), allow_unused=True) if loss.requires_grad else (None, None)
        gD = torch.zeros_like(Dd) if gD is None else gD
        gO = torch.zeros_like(Od) if gO is None else gO
    else:
        gD, gO = closed_form(Dd.detach(), Od.detach(), S, order, space, min_opacity)
    return dict(loss=float(loss.detach()), parts=(float(parts[0]), float(parts[1])), per_view=per_view.detach(), active=active, g_depth=gD.detach(),
                g_opacity=gO.detach())


def block_segments(V, H, W, seed=0):
    """int32 [V,H,W] block-segment map whose boundaries fall exactly on the kernel's tile seams (columns 63|64, rows 15|16) and one pixel
    to either side of them, with void pixels on both sides of a seam and in the image corners"""
    yy, xx = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    S = torch.zeros(V, H, W, dtype=torch.int32)
    for v in range(V):
        cx, cy = (63, 64, 65)[v % 3], (15, 16, 17)[(v + 1) % 3]  # first boundary: column cx - 1 | cx, row cy - 1 | cy
        S[v] = (1 + (xx >= cx).int() + (xx >= cx + 64).int() + (xx >= cx + 129).int()) + 10 * ((yy >= cy).int() + (yy >= cy + 15).int() + (yy >= cy + 33).int())
    if H * W < 64:  # (a handful of pixels: the segments alone, so that the few terms there are stay)
        return S
    g = torch.Generator().manual_seed(seed + 900)
    S[torch.rand(V, H, W, generator=g) < 0.03] = -1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        S[:, y, x] = -1
    for y, x in ((15, 63), (16, 64), (15, 64), (16, 63), (3, 63), (3, 64), (15, 5), (16, 5)):
        if y < H and x < W:
            S[:, y, x] = -1
    return S


def make_inputs(kind, V, H, W, seed, segments=True):
    """Seeded float32 (D, O, S or None) on the CPU.  "smooth": the expected depth is a tilted plane per segment (so that second differences
    are near zero inside a segment) plus sigma-1e-3 noise; "noise": uniform in [0.5, 6].  From 12 x 18 pixels on, a 6 x 9 block at the image's
    origin and the rows H/2 .. H/2+2 hold a constant (depth, opacity) pair, for exactly-zero terms.  60 % of the pixels have O in [0.9, 1], the rest uniform
    in [0, 1] (crossing min_opacity = 0.5); D = expected depth * O."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(V, H, W, generator=g)
    S = block_segments(V, H, W, seed) if segments else None
    yy, xx = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W), torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    if kind == "smooth":
        ids = (S if S is not None else torch.zeros(V, H, W, dtype=torch.int32)).clamp_min(0).float()
        dhat = 2.0 + 0.13 * (ids % 7) + (0.011 + 0.003 * (ids % 5)) * xx + (0.017 - 0.002 * (ids % 3)) * yy + 1e-3 * torch.randn(V, H, W, generator=g)
    elif kind == "noise":
        dhat = 0.5 + 5.5 * r()
    else:
        raise ValueError(kind)
    O = torch.where(r() < 0.6, 0.9 + 0.1 * r(), r()) if H * W >= 64 else 0.9 + 0.1 * r()  # (a handful of pixels: all usable)
    if H >= 12 and W >= 18:
        dhat[:, :6, :9], O[:, :6, :9] = 2.5, 0.75
        dhat[:, H // 2:H // 2 + 3, :], O[:, H // 2:H // 2 + 3, :] = 3.0, 1.0
    return (dhat * O).float(), O.float(), S


def excluded(D, O, S, order, space, min_opacity=0.5, rel=1e-9):
    """bool [V,H,W]: gradient elements one of whose terms has |t| < rel * max|x| without being exactly 0 (its sign depends on the precision)"""
    (tx, ty), x, ok = term_values(D.double(), (torch.ones_like(D) if O is None else O).double(), S, order, space, min_opacity)
    bar = rel * float(torch.where(ok, x.abs(), torch.zeros_like(x)).max()) if bool(ok.any()) else 0.0
    out = torch.zeros(D.shape, dtype=torch.bool)
    for (t, act), dim in ((tx, 2), (ty, 1)):
        if t.numel() == 0:
            continue
        shaky = act & (t != 0) & (t.abs() < bar)
        for k in range(order + 1):
            out.narrow(dim, k, t.shape[dim]).logical_or_(shaky)
    return out
