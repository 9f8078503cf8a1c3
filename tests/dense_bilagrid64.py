"""Float64 reference, float32 emulation, derived bounds and the case list of csrc/bilagrid.hip.

Two independent float64 forms.  `explicit` is the definition written out with numpy: coordinates, cell corners, nested a + t (b - a) steps,
the affine product, and the three gradients by their formulas.  `by_grid_sample` is torch.nn.functional.grid_sample (5-D, bilinear, border
padding, align_corners=True) with the clamped luminance as the z coordinate, and float64 autograd for every gradient.  Their agreement
(tests/test_bilagrid_ref.py) pins the convention.  With dtype=np.float32 `explicit` is the emulation: the kernels' operations in the kernels'
order (an fma is one rounding of the exact product-sum), the grid gradient gathered per vertex over the kernel's window, 256 interleaved
threads, fp32 per thread, fp64 across threads.

Bounds, per element, u = 2^-24, all magnitudes from the float64 reference.  Notation for one pixel: C the 8 corner matrices, Cmax[c,k] the
largest |corner entry|, mag[c] = sum_k Cmax[c,k] |p_k| + Cmax[c,3].
  coordinates   fx = ((x + 0.5) / W) (Gw - 1): x + 0.5 is exact, a division and a product round: |dfx| <= 2u fx; fy likewise; tx = fx - x0
                is exact.  lum: a product and two fmas: |dlum| <= 3u sum_k |lw_k p_k|; the clamp is exact, the product by L - 1 rounds:
                |dfz| <= 3u (L - 1) sum_k |lw_k p_k| + u fz.
  one lerp      fl(b - a) then one fma: |error| <= u t |b - a| + u |result| <= 3u max(|a|, |b|); errors of a and b pass through a convex
                combination, so after the x, y and z steps |dM[c,k]| <= 9u Cmax[c,k].  (The count is on the corners and not on |M|: a lerp
                of corners of opposite sign rounds relative to the corners.)
  forward       the affine product is three fmas: 3u (sum_k |M_ck p_k| + |M_c3|) <= 3u mag[c].  With the lerps: 12u mag[c], plus per axis
                |df| x (the interpolated |corner differences| along that axis applied to (|p|, 1)).  Along z the larger of the pixel's cell
                and its two neighbours is taken, so that a pixel on a level boundary, which fp32 may put in the other cell, is covered
                (the interpolant is continuous).  x and y cells agree between fp32 and float64 for every case (asserted).
  g_in          affine part: a product and two fmas on interpolated M: 12u sum_c Cmax[c,k] |g_c|, plus |df| x differences as above.
                Guidance part: D = A1 - A0 of two twice-interpolated levels: 2 x 6u Cmax + u |D| <= 14u Cmax; three dots D[c] . (p, 1)
                of three fmas (|D| <= 2 Cmax): 14u + 6u = 20u mag[c]; their sum with g: 3 x 2u; the product by L - 1 and the last fma: 2u
                each: 30u lw_k (L - 1) sum_c |g_c| mag[c], plus (|dfx| X_xz + |dfy| X_yz), X the interpolated |mixed second differences|
                applied to (|p|, 1) and to |g|.  D does not depend on tz inside a cell.
  g_grids       one term is w g_c p_k with w = (wy wx) wz: the four weights round once or twice (6u together with the two products), w g
                once, and the fma into the thread's sum once per add of at most n_t = ceil(window pixels / 256) terms; the fp64 tree adds
                nothing visible and the store rounds once: (n_t + 9) u sum |w g_c p_k|, plus sum (|dfx| wy wz + |dfy| wx wz + |dfz| wx wy)
                |g_c p_k| for the weights' coordinate error (a weight moves by at most |df| times the other two).
  tv            fp32 differences (u each, 2u on a square), fp64 sums, one rounding: 4u tv.  Gradient: 2u on each difference and the fp32
                add into g_grids: 3u x the sum of the absolute terms.
Every bound is multiplied by 1.001 for the second-order terms and carries 1e-37 for the subnormal range."""
import math

import numpy as np
import torch

U = 2.0 ** -24
LW = (0.299, 0.587, 0.114)
NT = 256
MUTATIONS = ("lum_perm", "align_false", "no_clamp", "no_guidance_grad", "guidance_grad_unclamped", "transposed", "stale_vertex")
TV_MUTATIONS = ("tv_drop_axis", "tv_wrong_count")


def identity_grids(V, Gh, Gw, L):
    g = np.zeros((V, 12, L, Gh, Gw), np.float32)
    g[:, (0, 5, 10)] = 1.0
    return g


def _fma(a, b, c, dt):
    """one rounding of a * b + c in dt (the product of two float32 is exact in float64)"""
    if dt == np.float64:
        return a * b + c
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def coords(n_pix, n_grid, dt, align_false=False):
    """(f, i0, t) of the n_pix pixel centres along an axis with n_grid vertices"""
    i = np.arange(n_pix).astype(dt)
    if align_false:
        f = np.clip((i + dt(0.5)) / dt(n_pix) * dt(n_grid) - dt(0.5), dt(0), dt(n_grid - 1))
    else:
        f = (i + dt(0.5)) / dt(n_pix) * dt(n_grid - 1)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_grid - 2)
    return f, i0, f - i0.astype(dt)


def luminance(img, dt, lw=LW):
    r, g, b = img[:, 0], img[:, 1], img[:, 2]
    return _fma(dt(lw[2]), b, _fma(dt(lw[1]), g, dt(lw[0]) * r, dt), dt)


def _lerp(a, b, t, dt):
    return _fma(t, b - a, a, dt)


def explicit(img, grids, g_out=None, dtype=np.float64, mut=None, want_grids=True):
    """img [V,3,H,W], grids [V,12,L,Gh,Gw], g_out [V,3,H,W] or None -> dict(out, g_in, g_grids and what the bounds need).  dtype float64: the
    reference; float32: the emulation.  mut: one of MUTATIONS, a deliberately wrong variant."""
    dt = dtype
    img, grids = np.asarray(img).astype(dt), np.asarray(grids).astype(dt)
    V, _, H, W = img.shape
    _, _, L, Gh, Gw = grids.shape
    G = grids.transpose(0, 2, 3, 4, 1)  # [V,L,Gh,Gw,12]
    if mut == "transposed":
        G = G.reshape(V, L, Gh, Gw, 4, 3).swapaxes(-1, -2).reshape(V, L, Gh, Gw, 12)
    fx, x0, tx = coords(W, Gw, dt, mut == "align_false")
    fy, y0, ty = coords(H, Gh, dt, mut == "align_false")
    lum = luminance(img, dt, (LW[1], LW[2], LW[0]) if mut == "lum_perm" else LW)
    with np.errstate(invalid="ignore"):
        cl = lum if mut == "no_clamp" else np.minimum(np.maximum(np.where(np.isnan(lum), dt(0), lum), dt(0)), dt(1))
    fz = cl * dt(L - 1)
    z0 = np.clip(np.floor(fz).astype(np.int64), 0, L - 2)
    tz = fz - z0.astype(dt)
    vi = np.arange(V)[:, None, None]
    xs = np.maximum(x0 - 1, 0) if mut == "stale_vertex" else x0

    def corner(dz, dy, dx, zc=z0):
        return G[vi, zc + dz, (y0 + dy)[None, :, None], (xs + dx)[None, None, :]]  # [V,H,W,12]

    TX, TY, TZ = tx[None, None, :, None], ty[None, :, None, None], tz[..., None]
    A = []
    for dz in (0, 1):
        r = [_lerp(corner(dz, dy, 0), corner(dz, dy, 1), TX, dt) for dy in (0, 1)]
        A.append(_lerp(r[0], r[1], TY, dt))
    D = A[1] - A[0]
    M = _fma(TZ, D, A[0], dt)
    p = [img[:, k] for k in range(3)]

    def affine(Q, c):
        return _fma(Q[..., 4 * c + 2], p[2], _fma(Q[..., 4 * c + 1], p[1], _fma(Q[..., 4 * c], p[0], Q[..., 4 * c + 3], dt), dt), dt)

    res = dict(out=np.stack([affine(M, c) for c in range(3)], 1), lum=lum, fz=fz, z0=z0, x0=x0, y0=y0, M=M, D=D)
    if g_out is None:
        return res
    g = np.asarray(g_out).astype(dt)
    S = g[:, 0] * affine(D, 0)
    S = _fma(g[:, 1], affine(D, 1), S, dt)
    S = _fma(g[:, 2], affine(D, 2), S, dt)
    inside = (lum > 0) & (lum < 1)
    if mut == "guidance_grad_unclamped":
        inside = np.ones_like(inside)
    S = np.where(inside, S * dt(L - 1), dt(0))
    if mut == "no_guidance_grad":
        S = np.zeros_like(S)
    res["g_in"] = np.stack([_fma(dt(LW[j]), S, _fma(M[..., 8 + j], g[:, 2], _fma(M[..., 4 + j], g[:, 1], M[..., j] * g[:, 0], dt), dt), dt) for j in range(3)], 1)
    if want_grids:
        res["g_grids"] = _grid_gradient_emulated(img, g, fz, Gh, Gw, L) if dt == np.float32 else scatter(
            V, L, Gh, Gw, (z0, tz), (y0, ty), (xs, tx), [g[:, c] * (p[k] if k < 3 else 1.0) for c in range(3) for k in range(4)])
    return res


def scatter(V, L, Gh, Gw, cz, cy, cx, values, weights=(None, None, None)):
    """sum over pixels of w_z w_y w_x values[ch] into [V,12,L,Gh,Gw]: the definition of the grid gradient.  cz = (z0 [V,H,W], tz), cy = (y0 [H],
    ty), cx = (x0 [W], tx); weights[axis] = (lo, hi) replaces (1 - t, t) on that axis (the bounds' derivative weights)."""
    (z0, tz), (y0, ty), (x0, tx) = cz, cy, cx
    H, W = y0.shape[0], x0.shape[0]
    wz = weights[0] or (1.0 - tz, tz)
    wy = weights[1] or (1.0 - ty, ty)
    wx = weights[2] or (1.0 - tx, tx)
    out = np.zeros((V, 12, L, Gh, Gw))
    vi = np.broadcast_to(np.arange(V)[:, None, None], (V, H, W))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = np.broadcast_to(wz[dz], (V, H, W)) * np.broadcast_to(wy[dy], (H,))[None, :, None] * np.broadcast_to(wx[dx], (W,))[None, None, :]
                yi = np.broadcast_to((y0 + dy)[None, :, None], (V, H, W))
                xi = np.broadcast_to((x0 + dx)[None, None, :], (V, H, W))
                for ch in range(12):
                    np.add.at(out[:, ch], (vi, z0 + dz, yi, xi), w * values[ch])
    return out


def window(i, n_pix, g):
    """the kernel's pixel window of vertex i along an axis, margin included"""
    s = n_pix / (g - 1)
    return max(math.floor((i - 1) * s - 0.5) - 1, 0), min(math.ceil((i + 1) * s - 0.5) + 1, n_pix - 1)


def terms_per_thread(H, W, Gh, Gw):
    """n_t: the most terms one thread of the grid-gradient kernel adds"""
    n = 0
    for iy in (0, Gh // 2, Gh - 1):
        for ix in (0, Gw // 2, Gw - 1):
            (a, b), (c, d) = window(iy, H, Gh), window(ix, W, Gw)
            n = max(n, (b - a + 1) * (d - c + 1))
    n = max(n, (math.ceil(2 * H / (Gh - 1)) + 4) * (math.ceil(2 * W / (Gw - 1)) + 4))
    return -(-n // NT)


def _grid_gradient_emulated(img, g, fz, Gh, Gw, L):
    """the gather of bilagrid_ggrid_kernel in float32: per vertex the window pixels idx = t, t + 256, ... per thread t in fp32, the threads in fp64"""
    f32 = np.float32
    V, _, H, W = img.shape
    _, y0, ty = coords(H, Gh, f32)
    _, x0, tx = coords(W, Gw, f32)
    out = np.zeros((V, 12, L, Gh, Gw), f32)
    for iy in range(Gh):
        ylo, yhi = window(iy, H, Gh)
        ys = np.arange(ylo, yhi + 1)
        wy = np.where(y0[ys] == iy, f32(1) - ty[ys], np.where(y0[ys] + 1 == iy, ty[ys], f32(0)))
        for ix in range(Gw):
            xlo, xhi = window(ix, W, Gw)
            xs = np.arange(xlo, xhi + 1)
            wx = np.where(x0[xs] == ix, f32(1) - tx[xs], np.where(x0[xs] + 1 == ix, tx[xs], f32(0)))
            wxy = (wy[:, None] * wx[None, :]).reshape(-1)
            n = wxy.shape[0]
            pad = -(-n // NT) * NT - n
            sel = np.ix_(range(V), range(3), ys, xs)
            pp = np.pad(img[sel].reshape(V, 3, n), ((0, 0), (0, 0), (0, pad))).reshape(V, 3, -1, NT)
            gg = np.pad(g[sel].reshape(V, 3, n), ((0, 0), (0, 0), (0, pad))).reshape(V, 3, -1, NT)
            ff = np.pad(fz[:, ys][:, :, xs].reshape(V, n), ((0, 0), (0, pad))).reshape(V, -1, NT)
            ww = np.pad(wxy, (0, pad)).reshape(-1, NT)
            for l in range(L):
                w = ww[None] * np.maximum(f32(0), f32(1) - np.abs(ff - f32(l)))
                for c in range(3):
                    wg = w * gg[:, c]
                    for k in range(4):
                        acc = np.zeros((V, NT), f32)
                        for j in range(ww.shape[0]):
                            live = ww[j] != 0
                            step = _fma(wg[:, j], pp[:, k, j], acc, f32) if k < 3 else acc + wg[:, j]
                            acc = np.where(live[None], step, acc)
                        out[:, 4 * c + k, l, iy, ix] = acc.astype(np.float64).sum(1).astype(f32)
    return out


def by_grid_sample(img, grids, g_out=None):
    """the same slice through torch's grid_sample in float64; with g_out also (g_in, g_grids) by autograd"""
    x = torch.as_tensor(np.asarray(img), dtype=torch.float64).clone().requires_grad_(g_out is not None)
    A = torch.as_tensor(np.asarray(grids), dtype=torch.float64).clone().requires_grad_(g_out is not None)
    V, _, H, W = x.shape
    lum = LW[0] * x[:, 0] + LW[1] * x[:, 1] + LW[2] * x[:, 2]
    gx = ((torch.arange(W, dtype=torch.float64) + 0.5) / W * 2 - 1)[None, None, :].expand(V, H, W)
    gy = ((torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1)[None, :, None].expand(V, H, W)
    gz = lum.clamp(0, 1) * 2 - 1
    grid = torch.stack((gx, gy, gz), -1)[:, None]  # [V,1,H,W,3]
    M = torch.nn.functional.grid_sample(A, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]  # [V,12,H,W]
    M = M.view(V, 3, 4, H, W)
    out = (M[:, :, :3] * x[:, None]).sum(2) + M[:, :, 3]
    if g_out is None:
        return out.detach().numpy()
    g_in, g_grids = torch.autograd.grad(out, (x, A), torch.as_tensor(np.asarray(g_out), dtype=torch.float64))
    return out.detach().numpy(), g_in.numpy(), g_grids.numpy()


def bounds(img, grids, g_out=None, n_t=None):
    """per-element bounds (module header) from float64: dict(out [V,3,H,W], g_in [V,3,H,W], g_grids [V,12,L,Gh,Gw])"""
    img, grids = np.asarray(img).astype(np.float64), np.asarray(grids).astype(np.float64)
    V, _, H, W = img.shape
    _, _, L, Gh, Gw = grids.shape
    G = np.abs(grids.transpose(0, 2, 3, 4, 1)), grids.transpose(0, 2, 3, 4, 1)
    fx, x0, tx = coords(W, Gw, np.float64)
    fy, y0, ty = coords(H, Gh, np.float64)
    lum = luminance(img, np.float64)
    fz = np.clip(np.nan_to_num(lum), 0, 1) * (L - 1)
    z0 = np.clip(np.floor(fz).astype(np.int64), 0, L - 2)
    tz = fz - z0
    vi = np.arange(V)[:, None, None]
    C = lambda zc, dz, dy, dx: G[1][vi, zc + dz, (y0 + dy)[None, :, None], (x0 + dx)[None, None, :]]
    TX, TY, TZ = tx[None, None, :, None], ty[None, :, None, None], tz[..., None]
    lerp = lambda a, b, t: a + t * (b - a)
    ap = np.abs(img)
    on = lambda Q, c: Q[..., 4 * c] * ap[:, 0] + Q[..., 4 * c + 1] * ap[:, 1] + Q[..., 4 * c + 2] * ap[:, 2] + Q[..., 4 * c + 3]  # applied to (|p|, 1)
    Cmax = np.max(np.stack([np.abs(C(z0, dz, dy, dx)) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]), 0)
    dX = lerp(lerp(np.abs(C(z0, 0, 0, 1) - C(z0, 0, 0, 0)), np.abs(C(z0, 0, 1, 1) - C(z0, 0, 1, 0)), TY),
              lerp(np.abs(C(z0, 1, 0, 1) - C(z0, 1, 0, 0)), np.abs(C(z0, 1, 1, 1) - C(z0, 1, 1, 0)), TY), TZ)
    dY = lerp(lerp(np.abs(C(z0, 0, 1, 0) - C(z0, 0, 0, 0)), np.abs(C(z0, 0, 1, 1) - C(z0, 0, 0, 1)), TX),
              lerp(np.abs(C(z0, 1, 1, 0) - C(z0, 1, 0, 0)), np.abs(C(z0, 1, 1, 1) - C(z0, 1, 0, 1)), TX), TZ)

    def dz_of(zc):
        return lerp(lerp(np.abs(C(zc, 1, 0, 0) - C(zc, 0, 0, 0)), np.abs(C(zc, 1, 0, 1) - C(zc, 0, 0, 1)), TX),
                    lerp(np.abs(C(zc, 1, 1, 0) - C(zc, 0, 1, 0)), np.abs(C(zc, 1, 1, 1) - C(zc, 0, 1, 1)), TX), TY)

    dZ = np.maximum(dz_of(z0), np.maximum(dz_of(np.maximum(z0 - 1, 0)), dz_of(np.minimum(z0 + 1, L - 2))))
    dfx, dfy = (2 * U * fx)[None, None, :], (2 * U * fy)[None, :, None]
    dfz = 3 * U * (L - 1) * (LW[0] * ap[:, 0] + LW[1] * ap[:, 1] + LW[2] * ap[:, 2]) + U * fz
    fin = lambda b: 1.001 * b + 1e-37
    res = dict(out=fin(np.stack([12 * U * on(Cmax, c) + dfx * on(dX, c) + dfy * on(dY, c) + dfz * on(dZ, c) for c in range(3)], 1)))
    if g_out is None:
        return res
    ag = np.abs(np.asarray(g_out).astype(np.float64))
    col = lambda Q, k: Q[..., k] * ag[:, 0] + Q[..., 4 + k] * ag[:, 1] + Q[..., 8 + k] * ag[:, 2]  # column k against |g|
    mixed = lambda a: np.abs(a[3] - a[2] - a[1] + a[0])
    Xxz = lerp(mixed([C(z0, 0, 0, 0), C(z0, 0, 0, 1), C(z0, 1, 0, 0), C(z0, 1, 0, 1)]), mixed([C(z0, 0, 1, 0), C(z0, 0, 1, 1), C(z0, 1, 1, 0), C(z0, 1, 1, 1)]), TY)
    Xyz = lerp(mixed([C(z0, 0, 0, 0), C(z0, 0, 1, 0), C(z0, 1, 0, 0), C(z0, 1, 1, 0)]), mixed([C(z0, 0, 0, 1), C(z0, 0, 1, 1), C(z0, 1, 0, 1), C(z0, 1, 1, 1)]), TX)
    gmag = sum(ag[:, c] * on(Cmax, c) for c in range(3))
    gmix = sum(ag[:, c] * (dfx * on(Xxz, c) + dfy * on(Xyz, c)) for c in range(3))
    res["g_in"] = fin(np.stack([12 * U * col(Cmax, k) + dfx * col(dX, k) + dfy * col(dY, k) + dfz * col(dZ, k) + LW[k] * (L - 1) * (30 * U * gmag + gmix)
                                for k in range(3)], 1))
    n_t = terms_per_thread(H, W, Gh, Gw) if n_t is None else n_t
    absv = [ag[:, c] * (ap[:, k] if k < 3 else 1.0) for c in range(3) for k in range(4)]
    cz, cy, cx = (z0, tz), (y0, ty), (x0, tx)
    one = (1.0, 1.0)
    b = (n_t + 9) * U * scatter(V, L, Gh, Gw, cz, cy, cx, absv)
    b += scatter(V, L, Gh, Gw, cz, cy, cx, [a * np.broadcast_to(dfx, a.shape) for a in absv], weights=(None, None, one))
    b += scatter(V, L, Gh, Gw, cz, cy, cx, [a * np.broadcast_to(dfy, a.shape) for a in absv], weights=(None, one, None))
    b += scatter(V, L, Gh, Gw, cz, cy, cx, [a * dfz for a in absv], weights=(one, None, None))
    res["g_grids"] = fin(b)
    return res


def tv(grids, mut=None):
    """(tv, d tv / d grids, the gradient's sum of absolute terms) in float64"""
    A = torch.as_tensor(np.asarray(grids), dtype=torch.float64).clone().requires_grad_(True)
    V = A.shape[0]
    total, absg = 0.0, torch.zeros_like(A)
    for axis in (2, 3, 4):
        if mut == "tv_drop_axis" and axis == 2:
            continue
        n = A.shape[axis]
        d = A.narrow(axis, 1, n - 1) - A.narrow(axis, 0, n - 1)
        count = A[0].numel() if mut == "tv_wrong_count" else d[0].numel()
        total = total + (d ** 2).sum() / (V * count)
        with torch.no_grad():
            w = 2 * d.abs() / (V * count)
            absg.narrow(axis, 1, n - 1).add_(w)
            absg.narrow(axis, 0, n - 1).add_(w)
    (g,) = torch.autograd.grad(total, A)
    return float(total.detach()), g.numpy(), absg.numpy()


def tv_emulated(grids):
    """bilagrid_tv_kernel's arithmetic: fp32 differences, everything else fp64, rounded once"""
    A = np.asarray(grids, np.float32)
    V = A.shape[0]
    total, g = 0.0, np.zeros(A.shape, np.float64)
    for axis in (2, 3, 4):
        n = A.shape[axis]
        d = (np.take(A, range(1, n), axis) - np.take(A, range(0, n - 1), axis)).astype(np.float64)
        c = 1.0 / (V * d[0].size)
        total += c * (d * d).sum()
        lo, hi = [slice(None)] * 5, [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        g[tuple(hi)] += 2 * c * d
        g[tuple(lo)] -= 2 * c * d
    return np.float32(total), g.astype(np.float32)


def tv_bounds(grids):
    value, _, absg = tv(grids)
    return 1.001 * 4 * U * value + 1e-37, 1.001 * 3 * U * absg + 1e-37


# ---- inputs and the case list -------------------------------------------------------------------------------------------------------------
KINK = 1e-4  # gradient cases keep lum this far from 0 and 1 and fz this far (times L - 1) from an integer


def kink_distances(img, L):
    """(min |lum - {0, 1}|, min |fz - integer| / (L - 1)) over the pixels, in float64 from the float32 image"""
    lum = luminance(np.asarray(img).astype(np.float64), np.float64)
    fz = np.clip(lum, 0, 1) * (L - 1)
    inside = (lum > 0) & (lum < 1)
    dz = np.abs(fz - np.round(fz))[inside]
    return float(np.minimum(np.abs(lum), np.abs(lum - 1)).min()), float(dz.min() / (L - 1)) if dz.size else 1.0


def smooth_grids(V, Gh, Gw, L, seed, noise=0.3):
    """identity plus bounded noise (|.| <= noise), float32"""
    rng = np.random.default_rng(seed)
    return (identity_grids(V, Gh, Gw, L) + noise * (rng.random((V, 12, L, Gh, Gw)) * 2 - 1)).astype(np.float32)


def image(V, H, W, L, seed, lo=0.02, hi=0.98):
    """float32 pixels uniform in [lo, hi], redrawn where a pixel lies within KINK of a kink (so that no gradient test excludes a pixel)"""
    rng = np.random.default_rng(seed)
    img = (lo + (hi - lo) * rng.random((V, 3, H, W))).astype(np.float32)
    for _ in range(100):
        lum = luminance(img.astype(np.float64), np.float64)
        fz = np.clip(lum, 0, 1) * (L - 1)
        bad = (np.abs(lum) < 2 * KINK) | (np.abs(lum - 1) < 2 * KINK) | ((lum > 0) & (lum < 1) & (np.abs(fz - np.round(fz)) < 2 * KINK * (L - 1)))
        if not bad.any():
            return img
        new = (lo + (hi - lo) * rng.random((V, 3, H, W))).astype(np.float32)
        img = np.where(bad[:, None], new, img)
    raise RuntimeError("could not draw an image away from the kinks")


# name -> (V, H, W, (Gh, Gw, L), pixel range); the letters are those of the GPU test's table
CASES = {
    "a_one_cell": (2, 5, 7, (2, 2, 2), (0.02, 0.98)),
    "b_uneven_432": (1, 33, 47, (4, 3, 2), (0.02, 0.98)),
    "b_uneven_345": (1, 33, 47, (3, 4, 5), (0.02, 0.98)),
    "c_default": (2, 64, 80, (16, 16, 8), (0.02, 0.98)),
    "d_finer_than_pixels": (1, 8, 8, (16, 16, 8), (0.02, 0.98)),
    "e_one_row": (1, 1, 37, (3, 5, 4), (0.02, 0.98)),
    "e_one_column": (1, 29, 1, (5, 2, 3), (0.02, 0.98)),
    "f_L9": (1, 19, 23, (3, 3, 9), (0.02, 0.98)),
    "f_L16": (1, 19, 23, (2, 3, 16), (0.02, 0.98)),
    "g_staged_side": (1, 24, 40, (10, 16, 8), (0.02, 0.98)),  # 10 vertex rows x 16 x 8 x 48 bytes = 60 KB: staged
    "g_global_side": (1, 24, 40, (11, 16, 8), (0.02, 0.98)),  # 11 rows = 66 KB: read from global memory
    "h_clamped": (2, 21, 26, (4, 5, 6), (-0.6, 1.6)),
}


def make_case(name):
    """(img, grids, g_out) float32 numpy of a case; the seed is the name's"""
    V, H, W, (Gh, Gw, L), (lo, hi) = CASES[name]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    rng = np.random.default_rng(seed + 1)
    return image(V, H, W, L, seed, lo, hi), smooth_grids(V, Gh, Gw, L, seed + 2), (rng.standard_normal((V, 3, H, W)) / (H * W)).astype(np.float32)


def kink_case():
    """forward only: pixels exactly on level boundaries and on both ends of the clamp (L = 5: fz integer at lum = 0, 0.25, 0.5, 0.75, 1)"""
    V, H, W, L = 1, 6, 9, 5
    img = image(V, H, W, L, 99)
    vals = [0.0, 0.25, 0.5, 0.75, 1.0, 1.5, -0.5, 0.2500001, 0.4999999]
    for i, x in enumerate(vals):
        img[0, :, i % H, i] = np.float32(x)  # r = g = b = x: lum = x up to rounding
    return img, smooth_grids(V, 3, 4, L, 98)
