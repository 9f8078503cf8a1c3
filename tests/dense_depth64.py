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


# ==== per-element parity of csrc/depth_loss.hip ===========================================================================================
"""(continued) The crafted cases, the float64 evaluation of everything siu3r_depth_loss writes with its per-element bound, and an
emulation of the kernels, shared by tests/test_depth_loss_ref.py (CPU) and tests/test_loss_stages_gpu.py (GPU).

THE COMPARISON is |got - ref| <= DEPTH_BOUND * |ref| + extra per element.  The kernels load float32 (the upcast is exact), compute in
fp64 from the pixel on and round once, at the float32 store: u = 2^-24 relative (round to nearest), plus a handful of fp64 roundings
(x = D * (1 / O) 2, the products with w and dx/dD 2, the sums below): DEPTH_BOUND = u + 32 * 2^-53.  extra is 2^-149 (a result in the
denormal range rounds to a multiple of it) plus, in the pearson mode, the propagated fp64 error of the view's four statistics:
  the six raw moments are sums of n_acc = 25 + ceil(records / 256) levels (4 pixels, 6 shuffle levels, 3 waves, the record loop, 6 + 3 again,
  the products 3); sxx = swxx / sw - mx^2 cancels: relative error r_xx = (6 n_acc + 8) E[x^2] / sxx in units of v = 2^-53, r_yy alike,
  r_xy = (3 n_acc + 4) (E[xy] + mx my) / |sxy|; rho: r_rho = r_xy + (r_xx + r_yy) / 2 + 4; c_y: (r_xx + r_yy) / 2 + n_acc + 6; c_x: r_rho +
  r_xx + n_acc + 6; mu_x, mu_y: (2 n_acc + 2) |mu| absolute.
  1 - rho: v (r_rho |rho| + 1) absolute (+ u (1 - rho) of the store);  a pixel: v [ |t1| (r_cy + 4) + |t2| (r_cx + 4) + w (|c_y| e_my +
  |c_x| e_mx) ] |dx/dD|, t1 = w (y - mu_y) c_y, t2 = w (x - mu_x) c_x.  On smooth depth around 3 with 1 - rho = 4e-4 that is ~1e-11
  relative: the float32 store dominates, three orders of magnitude below what float32 moments would give.
Nothing is undecided: validity is a chain of exact float32 comparisons, decided here on the same float32 values (counts are exact);
the sign of x - y and the min < max tests of a view are decided on the same fp64 expressions (x = D * (1 / O), as the kernel forms it), and
the cases keep x and y apart (>= 5 %) except where they are equal bit for bit on purpose (O = 1, D = T: the subgradient is exactly 0).
In the l1 mode the maps come WITHOUT 1 / N, which is out[2]."""
import functools
import zlib

U24, V53 = 2.0 ** -24, 2.0 ** -53
DEPTH_BOUND = U24 + 32 * V53
DENORM = 2.0 ** -149
CHUNK = 1024
MIN_OPACITY = 0.5
FMAX32 = float(np.finfo(np.float32).max)

# name: V, H, W, mode, space, weights, grad, content
DEPTH_CASES = {
    "p1": (1, 1, 1, "l1", "depth", False, True, "plain"),
    "p3_views3": (3, 1, 3, "pearson", "depth", True, True, "plain"),
    "p4": (1, 2, 2, "l1", "inverse", True, True, "plain"),
    "p5_views3": (3, 1, 5, "l1", "depth", False, True, "plain"),
    "p1023_views3": (3, 33, 31, "pearson", "inverse", False, True, "thresholds"),
    "p1024": (1, 32, 32, "pearson", "depth", True, False, "thresholds"),
    "p1025_views3": (3, 25, 41, "l1", "depth", True, True, "thresholds"),
    "p1025_l1_inverse_nograd": (3, 41, 25, "l1", "inverse", False, False, "thresholds"),
    "p2049_views3": (3, 3, 683, "pearson", "depth", True, True, "thresholds"),
    "p2049_l1_inverse": (1, 683, 3, "l1", "inverse", True, True, "thresholds"),
    "nonfinite": (3, 7, 37, "pearson", "inverse", True, True, "nonfinite"),
    "nonfinite_l1": (3, 37, 7, "l1", "depth", True, True, "nonfinite"),
    "views_none_one": (3, 9, 13, "pearson", "depth", False, True, "none_one"),
    "views_none_one_l1": (3, 9, 13, "l1", "inverse", False, True, "none_one"),
    "views_constant": (3, 13, 9, "pearson", "inverse", False, True, "constant"),
    "views_constant_l1": (3, 13, 9, "l1", "depth", False, True, "constant"),
    "equal_pixels": (1, 5, 11, "l1", "depth", False, True, "equal"),
    "equal_pixels_inverse": (3, 5, 11, "l1", "inverse", False, True, "equal"),
    "small_loss": (1, 45, 45, "pearson", "depth", False, True, "smooth"),
    "two_chunks_of_records": (1, 513, 512, "pearson", "depth", False, True, "smooth"),
}
DEPTH_FAULTS = ("valid_ge", "inverse_sign", "uncounted_in_mean", "tail_fill")


def _ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


@functools.lru_cache(maxsize=None)
def depth_case(name):
    V, H, W, mode, space, weights, grad, kind = DEPTH_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    P = H * W
    r = lambda: rng.random((V, P))
    if kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        dhat = (3.0 + 0.7 * np.sin(yy / (0.31 * H) + 0.2) * np.cos(xx / (0.23 * W)))[None].repeat(V, 0).reshape(V, P)
        T = 1.3 * dhat + 0.4 + 0.014 * rng.standard_normal((V, P))
        O = 0.9 + 0.1 * r()
    else:
        dhat = 0.5 + 5.5 * r()
        T = dhat * np.where(r() < 0.5, 0.6 + 0.35 * r(), 1.05 + 0.45 * r())  # x and y at least 5 % apart, in both spaces
        O = np.where(r() < 0.6, 0.9 + 0.1 * r(), r())
    D, O, T = (dhat * O).astype(np.float32), O.astype(np.float32), T.astype(np.float32)
    Wt = (0.05 + r()).astype(np.float32) if weights else None
    if P > 8 and kind != "smooth":
        T[r() < 0.1] = 0.0
        if weights:
            Wt[r() < 0.1] = 0.0
    marks = {}
    if kind == "thresholds":  # in every view: each threshold, and one float32 ulp either side of it
        tiny_ok = np.float32(2.0 ** -149) if space == "depth" else np.float32(2.0 ** -20)  # (inverse: O / D^2 of a denormal D leaves float32)
        rows = [("O", O, [_ulp(MIN_OPACITY, False), np.float32(MIN_OPACITY), _ulp(MIN_OPACITY, True)]),
                ("D", D, [np.float32(-2.0 ** -149), np.float32(0), tiny_ok]), ("T", T, [np.float32(-2.0 ** -149), np.float32(0), tiny_ok])]
        if weights:
            rows.append(("W", Wt, [np.float32(-2.0 ** -149), np.float32(0), np.float32(2.0 ** -149)]))
        at = 7
        for key, arr, vals in rows:
            for side, val in zip(("below", "on", "above"), vals):
                for rep in range(3):  # three pixels each, the last ones in the plane's tail
                    i = at if rep < 2 else P - 1 - (at % 37)
                    O[:, i], D[:, i] = 0.75, 1.5
                    T[:, i] = 2.25 if space == "depth" or key != "D" else 2.0 ** -18
                    if weights:
                        Wt[:, i] = 0.5
                    arr[:, i] = val
                    marks.setdefault(key + "_" + side, []).append(i)
                    at += 1
    if kind == "nonfinite":
        k = 3
        for arr in (D, O, T) + ((Wt,) if weights else ()):
            for val in (np.nan, np.inf, -np.inf):
                arr[:, k] = val
                arr[1, P - 1 - k] = val
                marks.setdefault("nonfinite", []).append(k)
                k += 2
    if kind == "none_one":
        O[0] = 0.25           # view 0: nothing valid
        T[1] = 0.0
        T[1, P - 2], O[1, P - 2] = 2.0, 0.875   # view 1: one valid pixel, in the scalar tail
    if kind == "constant":
        O[0], D[0] = 1.0, 2.5  # view 0: constant x (O = 1: exact)
        T[1] = 1.75           # view 1: constant y
    if kind == "equal":       # x == y bit for bit in both spaces
        O[:, ::3] = 1.0
        D[:, ::3] = T[:, ::3] = np.float32(1.0) + (np.arange(0, P, 3) % 7).astype(np.float32) * np.float32(0.25)
    sh = (V, H, W)
    return dict(name=name, V=V, H=H, W=W, mode=mode, space=space, grad=grad, marks=marks, D=D.reshape(sh), O=O.reshape(sh), T=T.reshape(sh),
                Wt=None if Wt is None else Wt.reshape(sh))


def _pixels64(c, fault=None):
    """valid [V,P] and the kernel's fp64 per-pixel quantities (harmless values at the invalid pixels)"""
    V, P = c["V"], c["H"] * c["W"]
    D, O, T = (c[k].reshape(V, P) for k in ("D", "O", "T"))
    Wt = np.ones((V, P), np.float32) if c["Wt"] is None else c["Wt"].reshape(V, P)
    mo = np.float32(MIN_OPACITY)
    with np.errstate(invalid="ignore"):
        ok = ((O >= mo) if fault == "valid_ge" else (O > mo)) & (O <= FMAX32) & (D > 0) & (D <= FMAX32) & (T > 0) & (T <= FMAX32) & (Wt > 0) & (Wt <= FMAX32)
    Dd, Od, Td = (np.where(ok, a, np.float32(1)).astype(np.float64) for a in (D, O, T))
    if c["space"] == "inverse":
        iD = 1.0 / Dd
        x, y = Od * iD, 1.0 / Td
        dxdD, dxdO = (x * iD if fault == "inverse_sign" else -x * iD), iD
    else:
        iO = 1.0 / Od
        x, y = Dd * iO, Td
        dxdD, dxdO = iO, -x * iO
    return ok, x, y, Wt.astype(np.float64), dxdD, dxdO


@functools.lru_cache(maxsize=None)
def depth_ref(name):
    """everything siu3r_depth_loss writes, in float64: out [4], per_view [V], valid [V], g_depth, g_opacity [V,H,W] (l1: without 1 / N), each
    with its absolute tolerance tol_* (= DEPTH_BOUND |ref| + extra), and the branch population"""
    c = depth_case(name)
    V, H, W, P = c["V"], c["H"], c["W"], c["H"] * c["W"]
    ok, x, y, w, dxdD, dxdO = _pixels64(c)
    w = np.where(ok, w, 0.0)
    valid = ok.sum(1)
    per_view, tol_pv = np.full(V, np.nan), np.zeros(V)
    gx, xg = np.zeros((V, P)), np.zeros((V, P))  # d loss / dx and its absolute fp64 allowance
    bpv = -(-P // CHUNK)
    n_acc = 25 + -(-bpv // 256)
    if c["mode"] == "l1":
        e = x - y
        N = w.sum()
        tot = (w * np.abs(e)).sum()
        for v in range(V):
            if valid[v]:
                per_view[v] = (w[v] * np.abs(e[v])).sum() / w[v].sum()
        gx = w * np.sign(e)
        out = np.array([tot / N if N > 0 else 0.0, N, 1.0 / N if N > 0 else 0.0, 0.0])
        tol_out = DEPTH_BOUND * np.abs(out) + np.array([DENORM, 0, DENORM, 0])
        counted = valid > 0
    else:
        counted = np.zeros(V, bool)
        stats = {}
        for v in range(V):
            m = ok[v]
            if m.sum() >= 2 and x[v][m].max() > x[v][m].min() and y[v][m].max() > y[v][m].min():
                counted[v] = True
                p = w[v] / w[v].sum()
                mx, my = (p * x[v]).sum(), (p * y[v]).sum()
                sxx, syy, sxy = (p * (x[v] - mx) ** 2).sum(), (p * (y[v] - my) ** 2).sum(), (p * (x[v] - mx) * (y[v] - my)).sum()
                rho = sxy / np.sqrt(sxx * syy)
                r_xx, r_yy = (6 * n_acc + 8) * (sxx + mx * mx) / sxx, (6 * n_acc + 8) * (syy + my * my) / syy
                r_xy = (3 * n_acc + 4) * ((p * x[v] * y[v]).sum() + abs(mx * my)) / abs(sxy)
                r_rho = r_xy + 0.5 * (r_xx + r_yy) + 4
                stats[v] = (p, mx, my, sxx, syy, rho, 0.5 * (r_xx + r_yy) + n_acc + 6, r_rho + r_xx + n_acc + 6, r_rho)
        nc = int(counted.sum())
        tot, t_tot = 0.0, 0.0
        for v, (p, mx, my, sxx, syy, rho, r_cy, r_cx, r_rho) in stats.items():
            per_view[v] = 1.0 - rho
            tol_pv[v] = V53 * (r_rho * abs(rho) + 1)
            tot += 1.0 - rho
            t_tot += tol_pv[v]
            cy, cx = -1.0 / np.sqrt(sxx * syy) / nc, rho / sxx / nc
            t1, t2 = p * (y[v] - my) * cy, p * (x[v] - mx) * cx
            gx[v] = t1 + t2
            xg[v] = V53 * (np.abs(t1) * (r_cy + 4) + np.abs(t2) * (r_cx + 4) + p * (abs(cy) * (2 * n_acc + 2) * abs(my) + abs(cx) * (2 * n_acc + 2) * abs(mx)))
        out = np.array([tot / nc if nc else 0.0, float(nc), 1.0, 0.0])
        tol_out = DEPTH_BOUND * np.abs(out) + np.array([t_tot / max(nc, 1) + DENORM, 0, 0, 0])
    tol_pv = tol_pv + DEPTH_BOUND * np.abs(np.nan_to_num(per_view)) + DENORM
    gD, gO = np.where(ok, gx * dxdD, 0.0), np.where(ok, gx * dxdO, 0.0)
    tol_gD = DEPTH_BOUND * np.abs(gD) + np.where(ok, xg * np.abs(dxdD) + DENORM, 0.0)
    tol_gO = DEPTH_BOUND * np.abs(gO) + np.where(ok, xg * np.abs(dxdO) + DENORM, 0.0)
    sh = (V, H, W)
    mk = c["marks"]
    pop = dict(valid=int(ok.sum()), invalid=int((~ok).sum()), uncounted_views=int((~counted).sum()), counted_views=int(counted.sum()),
               scalar_views=sum(1 for v in range(V) if (v * P) % 4), tail=P % 4, records=bpv, zero_subgradient=int((ok & (x == y)).sum()),
               threshold_valid=sum(int(ok[:, i].all()) for k, ii in mk.items() if k.endswith("above") for i in ii),
               threshold_invalid=sum(int((~ok[:, i]).all()) for k, ii in mk.items() if not k.endswith("above") and k != "nonfinite" for i in ii),
               nonfinite_invalid=sum(int((~ok[:, i]).all()) for i in mk.get("nonfinite", [])))
    return dict(out=out, tol_out=tol_out, per_view=per_view, tol_per_view=tol_pv, valid=valid.astype(np.int64), g_depth=gD.reshape(sh),
                tol_g_depth=tol_gD.reshape(sh), g_opacity=gO.reshape(sh), tol_g_opacity=tol_gO.reshape(sh), ok=ok.reshape(sh), pop=pop)


def depth_emulate(name, fault=None):
    """the three kernels in numpy: fp64 per pixel, RAW moments per 1,024-pixel record, the records added per view, float32 stores.
    fault: one of DEPTH_FAULTS, the kernel with that one line wrong"""
    c = depth_case(name)
    V, H, W, P = c["V"], c["H"], c["W"], c["H"] * c["W"]
    ok, x, y, w, dxdD, dxdO = _pixels64(c, fault)
    w = np.where(ok, w, 0.0)
    if fault == "tail_fill" and P % 4:  # the last thread's vector reads past the plane as data
        n = 4 - P % 4
        pad = lambda a, val: np.concatenate([a, np.full((V, n), val, a.dtype)], 1)
        ok, x, y, w, dxdD, dxdO = pad(ok, True), pad(x, 1.0), pad(y, 2.0), pad(w, 1.0), pad(dxdD, 1.0), pad(dxdO, -1.0)
    Pp = x.shape[1]
    bpv = -(-Pp // CHUNK)
    rec = lambda a: np.array([[np.where(ok[v, b * CHUNK:(b + 1) * CHUNK], a[v, b * CHUNK:(b + 1) * CHUNK], 0.0).sum() for b in range(bpv)] for v in range(V)])
    cnt, sw = rec(np.ones_like(x)).sum(1), rec(w).sum(1)
    nan = np.float32(np.nan)
    per_view, gx = np.full(V, nan, np.float32), np.zeros((V, Pp))
    if c["mode"] == "l1":
        e = x - y
        sa = rec(w * np.abs(e)).sum(1)
        denom, total = sw.sum(), sa.sum()
        for v in range(V):
            if cnt[v] > 0:
                per_view[v] = np.float32(sa[v] / sw[v])
        inv = 1.0 / denom if denom > 0 else 0.0
        out = np.array([total * inv, denom, inv, 0.0]).astype(np.float32)
        gx = w * np.sign(e)
    else:
        total = denom = 0.0
        st = np.zeros((V, 4))
        for v in range(V):
            m = ok[v]
            counted = cnt[v] >= 2 and x[v][m].max() > x[v][m].min() and y[v][m].max() > y[v][m].min()
            if counted:
                isw = 1.0 / sw[v]
                s2, s3, s4, s5, s6 = (rec(a)[v].sum() for a in (w * x, w * y, w * x * x, w * y * y, w * x * y))
                mx, my = s2 * isw, s3 * isw
                sxx, syy, sxy = s4 * isw - mx * mx, s5 * isw - my * my, s6 * isw - mx * my
                inorm = 1.0 / np.sqrt(sxx * syy)
                rho = sxy * inorm
                st[v] = mx, my, -inorm * isw, rho / sxx * isw
                per_view[v] = np.float32(1.0 - rho)
                total += 1.0 - rho
            if counted or fault == "uncounted_in_mean":
                denom += 1.0
        inv = 1.0 / denom if denom > 0 else 0.0
        out = np.array([total * inv, denom, 1.0, 0.0]).astype(np.float32)
        st[:, 2:] *= inv
        for v in range(V):
            if st[v, 2] != 0.0 or st[v, 3] != 0.0:
                gx[v] = w[v] * ((y[v] - st[v, 1]) * st[v, 2] + (x[v] - st[v, 0]) * st[v, 3])
    sh = (V, H, W)
    with np.errstate(over="ignore"):
        gD, gO = np.where(ok, gx * dxdD, 0.0).astype(np.float32)[:, :P], np.where(ok, gx * dxdO, 0.0).astype(np.float32)[:, :P]
    return dict(out=out, per_view=per_view, valid=cnt.astype(np.int64), g_depth=gD.reshape(sh) if c["grad"] else None,
                g_opacity=gO.reshape(sh) if c["grad"] else None)


def depth_worst(got, ref, grad=True):
    """-> {output: max |got - ref| / tolerance}; NaN must meet NaN, a tolerance of 0 must meet the exact value"""
    w = {}
    for k in ("out", "per_view") + (("g_depth", "g_opacity") if grad else ()):
        g, r, t = np.asarray(got[k], np.float64).ravel(), np.asarray(ref[k], np.float64).ravel(), np.asarray(ref["tol_" + k]).ravel()
        nan = np.isnan(r)
        d = np.abs(np.where(nan, 0.0, g) - np.where(nan, 0.0, r))
        ratio = np.where(t > 0, d / np.maximum(t, 1e-300), np.where(d == 0, 0.0, np.inf))
        ratio = np.where(np.isnan(g) != nan, np.inf, ratio)
        w[k] = float(ratio.max()) if ratio.size else 0.0
    w["valid"] = 0.0 if np.array_equal(np.asarray(got["valid"], np.int64), ref["valid"]) else float("inf")
    return w
