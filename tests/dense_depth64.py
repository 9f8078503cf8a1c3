"""Dense restatement of the depth loss (siu3r_amd/losses.py::depth_loss, csrc/depth_loss.hip) in plain torch, parametrised by dtype.
float64 is the reference of the GPU tests, float32 the 'composed torch loss' their tolerance is taken from.  Two routes: `terms` is
differentiable (autograd gives the gradient), `closed_form` is the derivative the HIP kernel implements; tests/test_depth_loss_ref.py
checks one against the other on the CPU.

A pixel is valid iff O > min_opacity, D > 0, T > 0, Wt > 0 (when given) and all of them are finite; NaN fails every comparison.
space "depth": x = D / O, y = T; "inverse": x = O / D, y = 1 / T.  mode "l1": sum w |x - y| / sum w over all views; "pearson": the mean
of 1 - rho_v over the counted views (>= 2 valid pixels, max x > min x, max y > min y)."""
import numpy as np
import torch


def valid_mask(D, O, T, Wt, min_opacity):
    mo = float(np.float32(min_opacity))  # the kernel compares float32 values
    m = (O > mo) & (D > 0) & (T > 0) & torch.isfinite(D) & torch.isfinite(O) & torch.isfinite(T)
    if Wt is not None:
        m = m & (Wt > 0) & torch.isfinite(Wt)
    return m


def _xyw(D, O, T, Wt, space, m):
    """x, y, w, dx/dD, dx/dO with harmless values (w = 0) at the invalid pixels"""
    one = torch.ones_like(D)
    Ds, Os, Ts = torch.where(m, D, one), torch.where(m, O, one), torch.where(m, T, one)
    if space == "depth":
        x, y, dxdD, dxdO = Ds / Os, Ts, 1 / Os, -Ds / (Os * Os)
    elif space == "inverse":
        x, y, dxdD, dxdO = Os / Ds, 1 / Ts, -Os / (Ds * Ds), 1 / Ds
    else:
        raise ValueError(space)
    w = torch.where(m, one if Wt is None else Wt, torch.zeros_like(D))
    return x, y, w, dxdD, dxdO


def _counted(m_v, x_v, y_v):
    if int(m_v.sum()) < 2:
        return False
    xs, ys = x_v[m_v], y_v[m_v]
    return bool(xs.max() > xs.min()) and bool(ys.max() > ys.min())


def terms(D, O, T, Wt=None, mode="l1", space="depth", min_opacity=0.5):
    """differentiable w.r.t. D and O, in their dtype -> (loss 0-d, per_view [V], valid [V] int64, N (l1) or the number of counted views)"""
    m = valid_mask(D, O, T, Wt, min_opacity)
    x, y, w, _, _ = _xyw(D, O, T, Wt, space, m)
    V = D.shape[0]
    valid = m.flatten(1).sum(1)
    nan = torch.full((), float("nan"), dtype=D.dtype, device=D.device)
    if mode == "l1":
        e = w * (x - y).abs()
        N = w.sum()
        loss = e.sum() / N if float(N) > 0 else (x * 0).sum()
        per_view = torch.stack([e[v].sum() / w[v].sum() if int(valid[v]) > 0 else nan for v in range(V)])
        return loss, per_view.detach(), valid, float(N)
    if mode != "pearson":
        raise ValueError(mode)
    vals, per_view = [], []
    for v in range(V):
        if not _counted(m[v], x[v], y[v]):
            per_view.append(nan)
            continue
        p = w[v] / w[v].sum()
        mx, my = (p * x[v]).sum(), (p * y[v]).sum()
        sxx, syy, sxy = (p * (x[v] - mx) ** 2).sum(), (p * (y[v] - my) ** 2).sum(), (p * (x[v] - mx) * (y[v] - my)).sum()
        vals.append(1 - sxy / torch.sqrt(sxx * syy))
        per_view.append(vals[-1].detach())
    loss = torch.stack(vals).mean() if vals else (x * 0).sum()
    return loss, torch.stack(per_view), valid, float(len(vals))


def closed_form(D, O, T, Wt=None, mode="l1", space="depth", min_opacity=0.5):
    """(d loss / dD, d loss / dO) without autograd: the formulas of the kernel"""
    with torch.no_grad():
        m = valid_mask(D, O, T, Wt, min_opacity)
        x, y, w, dxdD, dxdO = _xyw(D, O, T, Wt, space, m)
        gx = torch.zeros_like(D)
        if mode == "l1":
            N = w.sum()
            if float(N) > 0:
                gx = w * torch.sign(x - y) / N
        else:
            counted = [v for v in range(D.shape[0]) if _counted(m[v], x[v], y[v])]
            for v in counted:
                p = w[v] / w[v].sum()
                mx, my = (p * x[v]).sum(), (p * y[v]).sum()
                sxx, syy, sxy = (p * (x[v] - mx) ** 2).sum(), (p * (y[v] - my) ** 2).sum(), (p * (x[v] - mx) * (y[v] - my)).sum()
                norm = torch.sqrt(sxx * syy)
                rho = sxy / norm
                gx[v] = -(1.0 / len(counted)) * p * ((y[v] - my) / norm - rho * (x[v] - mx) / sxx)
        zero = torch.zeros_like(D)
        return torch.where(m, gx * dxdD, zero), torch.where(m, gx * dxdO, zero)


def loss_and_grad(D, O, T, Wt=None, mode="l1", space="depth", min_opacity=0.5, dtype=torch.float64, route="closed"):
    """the inputs converted to `dtype` (an upcast of float32 inputs is exact) -> dict(loss, per_view, valid, count, g_depth, g_opacity);
    route "closed": the gradient by closed_form, "autograd": by torch autograd through `terms`"""
    c = lambda t: None if t is None else t.detach().to(dtype)
    Dd, Od, Td, Wd = c(D).clone().requires_grad_(route == "autograd"), c(O).clone().requires_grad_(route == "autograd"), c(T), c(Wt)
    loss, per_view, valid, count = terms(Dd, Od, Td, Wd, mode, space, min_opacity)
    if route == "autograd":
        gD, gO = torch.autograd.grad(loss, (Dd, Od), allow_unused=True)
        gD = torch.zeros_like(Dd) if gD is None else gD
        gO = torch.zeros_like(Od) if gO is None else gO
    else:
        gD, gO = closed_form(Dd.detach(), Od.detach(), Td, Wd, mode, space, min_opacity)
    return dict(loss=float(loss.detach()), per_view=per_view.detach(), valid=valid, count=count, g_depth=gD.detach(), g_opacity=gO.detach())


def make_inputs(kind, V, H, W, seed, weights=False):
    """Seeded float32 (D, O, T, Wt or None) on the CPU.  "noise": expected depth and target uniform in [0.5, 6]; "smooth": bilinear-upsampled
    4 x 4 noise in [1, 5] plus sigma-0.02 noise, target = 1.3 base + 0.4 + noise.  60 % of the pixels have O in [0.9, 1], the rest uniform
    in [0, 1]; D = expected depth * O; 15 % of the targets are 0 (holes); weights uniform with 10 % zeros.  A target within 1e-5 (relative,
    float64) of x in either space is moved by 1 %, so that the sign of the l1 subgradient cannot depend on the precision."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(V, H, W, generator=g)
    if kind == "noise":
        dhat, T = 0.5 + 5.5 * r(), 0.5 + 5.5 * r()
    elif kind == "smooth":
        base = 1.0 + 4.0 * F.interpolate(torch.rand(V, 1, 4, 4, generator=g), size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        dhat = base + 0.02 * torch.randn(V, H, W, generator=g)
        T = 1.3 * base + 0.4 + 0.02 * torch.randn(V, H, W, generator=g)
    else:
        raise ValueError(kind)
    O = torch.where(r() < 0.6, 0.9 + 0.1 * r(), r())
    D = (dhat * O).float()
    O, T = O.float(), T.float()
    T[r() < 0.15] = 0.0
    Wt = None
    if weights:
        Wt = r().float()
        Wt[r() < 0.1] = 0.0
    D64, O64, T64 = D.double(), O.double(), T.double()
    ok = (O64 > 0) & (D64 > 0) & (T64 > 0)
    one = torch.ones_like(D64)
    Ds, Os, Ts = torch.where(ok, D64, one), torch.where(ok, O64, one), torch.where(ok, T64, one)
    close = ok & (((Ds / Os - Ts).abs() <= 1e-5 * Ts) | ((Os / Ds - 1 / Ts).abs() <= 1e-5 / Ts))
    T[close] = T[close] * 1.01
    return D, O, T, Wt
