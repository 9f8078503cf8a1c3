"""Dense restatement of the photometric loss (siu3r_amd/losses.py, csrc/photo_loss.hip) in plain torch: depthwise conv2d with the window of
metrics._gauss1d, autograd for the gradient.  float64 is the reference of the GPU tests, float32 (`dtype=`) the 'composed torch loss' their
tolerance is taken from; closed_form_grad is the derivative the kernel implements, checked against autograd on the CPU."""
import torch
import torch.nn.functional as F

from siu3r_amd.metrics import _gauss1d

K1, K2, TAPS = 0.01, 0.03, 11


def _blur(x, g):
    """valid separable 11-tap convolution of [V,C,H,W] per channel"""
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def _window(like):
    return torch.from_numpy(_gauss1d(TAPS, 1.5)).to(device=like.device, dtype=like.dtype)


def ssim_map(pred, target, data_range=1.0):
    """[V,C,H-10,W-10] SSIM of every valid window (variances clamped at 0)"""
    g = _window(pred)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu_p, mu_t = _blur(pred, g), _blur(target, g)
    s_pp = (_blur(pred * pred, g) - mu_p * mu_p).clamp_min(0)
    s_tt = (_blur(target * target, g) - mu_t * mu_t).clamp_min(0)
    s_pt = _blur(pred * target, g) - mu_p * mu_t
    return ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))


def photo_loss(pred, target, lam=0.2, data_range=1.0):
    """(loss, L1, SSIM) of [V,C,H,W] tensors in their own dtype; a term that lam switches off is None"""
    l1 = (pred - target).abs().mean() if lam != 1 else None
    ss = ssim_map(pred, target, data_range).mean() if lam != 0 else None
    loss = 0
    if l1 is not None:
        loss = loss + (1 - lam) * l1
    if ss is not None:
        loss = loss + lam * (1 - ss)
    return loss, l1, ss


def loss_and_grad(pred, target, lam=0.2, data_range=1.0, dtype=torch.float64):
    """the inputs converted to `dtype` (an upcast of float32 inputs is exact) -> ((loss, L1, SSIM) as floats or None, d loss / d pred)"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    t = target.detach().to(dtype)
    loss, l1, ss = photo_loss(p, t, lam, data_range)
    (g,) = torch.autograd.grad(loss, p)
    f = lambda x: None if x is None else float(x.detach())
    return (f(loss), f(l1), f(ss)), g


def closed_form_grad(pred, target, data_range=1.0):
    """d mean(SSIM map) / d pred without autograd: the three derivative maps per window and their transposed blur"""
    g = _window(pred)
    C = pred.shape[1]
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu_p, mu_t = _blur(pred, g), _blur(target, g)
    spp_raw = _blur(pred * pred, g) - mu_p * mu_p
    s_pp, s_tt = spp_raw.clamp_min(0), (_blur(target * target, g) - mu_t * mu_t).clamp_min(0)
    s_pt = _blur(pred * target, g) - mu_p * mu_t
    A1, A2, B1, B2 = 2 * mu_p * mu_t + c1, 2 * s_pt + c2, mu_p * mu_p + mu_t * mu_t + c1, s_pp + s_tt + c2
    d_epp = -A1 * A2 / (B1 * B2 * B2) * (spp_raw > 0)
    d_ept = 2 * A1 / (B1 * B2)
    d_mu = 2 * mu_t * A2 / (B1 * B2) - 2 * mu_p * A1 * A2 / (B1 * B1 * B2) - 2 * mu_p * d_epp - mu_t * d_ept

    def blur_t(x):
        x = F.conv_transpose2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)
        return F.conv_transpose2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)

    return (blur_t(d_mu) + 2 * pred * blur_t(d_epp) + target * blur_t(d_ept)) / d_mu.numel()


# ==== per-element parity of csrc/photo_loss.hip ==========================================================================================
"""(continued) The crafted cases, the float64 evaluation of everything siu3r_photo_loss writes, its per-element error scale, and a float32
emulation of the kernel, shared by tests/test_photo_loss_ref.py (CPU) and tests/test_loss_stages_gpu.py (GPU).

THE COMPARISON is |got - ref| <= PHOTO_BOUND * S + extra per element (dense_raster_bwd64.assert_elems_close), u = 2^-24.

REFERENCE.  photo_ref walks the kernel's tiling in float64: per 32 x 32 tile the windows that reach its pixels, their moments in the
two-pass centred form sum g (p - mu)^2 (so its own cancellation error is 2^-53 of the window's values, whatever the offset), the closed
form of this file's header, and the pixel gradient  sum_w g(w, x) [dmu_c + 2 d_epp (p(x) - mu_p(w)) + d_ept (t(x) - mu_t(w))].  The window
is the exact metrics._gauss1d; the kernel's float32 constants differ from it by <= u g_k per tap, which is one more rounding per product
(counted below; in shifted units, because sum_k dg_k p_k = sum_k dg_k (p_k - cp) + cp sum_k dg_k and the kernel adds cp back after
the sum: the second term is u |mu_p|, the rounding of mp = mp_s + cp that is counted anyway).

SCALE.  A first-order running error count of the kernel's arithmetic, evaluated on the float64 intermediates of the element, in units of u.
With Mp = max |p - cp|, Mt = max |t - ct| over the pixels the tile stages (cp, ct: the tile's centre pixel; a pixel off the image is
staged as the shift itself and adds 0):
  shifted window means     K_MEAN Mp:  p - cp 1, the float32 weight 1, the product 1, 11 adds, the vertical weight 1 and 11 fused adds: 26
  second moments           27 Mp^2 (p - cp enters twice); mp_s^2: 2 * 26 + 1; the subtraction 1:  K_VAR = 81, in Mp^2, Mp Mt, Mt^2.
                           THIS is the term that fails a lost shift: without it the moments round in units of max |p|^2.
  mp = mp_s + cp           K_MEAN Mp + |mp|
  A1, A2, B1, B2           the products and sums of the closed form, one u per operation on the magnitude of its result; c1, c2 are
                           float32 products of float32 constants: 3 u each
  1 / (B1 B2), s / B2, s / B1   2 u per division (v_rcp_f32 is 1 ulp), amplified by 1 / B of the window.  Denominators enter as their lower
                           ends B - 2 u e_B (never below 0.99 c: both variances are clamped at 0), numerators as their upper ends; with
                           them the first-order count holds for relative perturbations up to 1/2, which is the factor 2 of PHOTO_BOUND.
  d_mu' = dmu_c - 2 d_epp mp_s - d_ept mt_s   every term with its magnitude, the products 2 u, the two subtractions on the sum of magnitudes
  transposed blur          sum_w g(w, x) e(w) + K_BLUR sum_w g(w, x) |D(w)|, K_BLUR = 24: two float32 weights, two chains of 11 fused adds
  pixel                    o0 + 2 p' o1 + t' o2: p' 1, the products 2, the adds on the sum of magnitudes; w_ssim 1, the store 1; w_l1 1, the add 1
so a pixel's scale is the sum over the windows that reach it of g(w, x) times the magnitude of each term, 1 / (B1 B2) included.
  partials   SSIM: sum of e_s over the owned windows + 16 sum |s| (7 sequential adds, 6 shuffle levels, 3 waves); L1: 14 sum |d|.
  out        the sums are fp64: the partials' scales over N, + 2 for the float32 stores.

UNDECIDED BRANCH.  d_epp = spp_raw > 0 ? -s / B2 : 0.  A window with |spp| <= u K_VAR Mp^2 (every flat window whose value is not the
centre pixel's: its spp_raw is rounding noise of either sign) may take either side.  The reference takes 0 there.  The two answers differ at
pixel x by sum_w g(w, x) 2 |d_epp(w)| |p(x) - mu_p(w)|, and g(w, x) (p(x) - mu_p(w))^2 <= spp(w) (one term of the sum that spp is), so
g |p(x) - mu_p| <= sqrt(g spp): extra(x) = |w_ssim| sum_w 2 |s / B2| sqrt(g(w, x)) sqrt(spp(w)) over the undecided windows, which is
0 on an exactly flat window and at most sqrt(u K_VAR) Mp |d_epp| otherwise.  What the kernel then computes from its own noisy
p'(x) - mp_s is covered by S: the magnitudes |d_epp| |mp_s| and |d_epp| e(mp_s) of an undecided window are in it.  No pixel is left out.
L1: the sign of p - t is an exact float32 comparison; pred == target gives exactly 0 in both."""
import functools
import zlib

import numpy as np

U24 = 2.0 ** -24
PHOTO_BOUND = 2 * U24
K_MEAN, K_VAR, K_BLUR = 26.0, 81.0, 24.0
TILE = 32
SENT_BITS = -0x5A5A5A5B  # tests/test_raster_stages_gpu.py's sentinel; as float32 -2.9e-16
SENT_F = np.array([SENT_BITS], np.int32).view(np.float32)[0]
G64 = np.asarray(_gauss1d(TAPS, 1.5), np.float64)
GW32 = G64.astype(np.float32)  # the kernel's GW[] (test_photo_loss_ref.py compares it with the literals of photo_loss.hip)
LAM_NEAR_ONE = float(np.float32(1.0 - 2.0 ** -24))

# name: H, W, V, C, content, lambda, data_range, grad, pred layout, target layout
PHOTO_CASES = {
    "one_window_11x12": (11, 12, 1, 1, "noise", 0.2, 1.0, True, "nchw", "nchw"),
    "one_window_12x11_nograd": (12, 11, 2, 3, "noise", 0.2, 1.0, False, "nhwc", "nchw"),
    "tile_edge_32x33": (32, 33, 1, 2, "smooth", 0.2, 1.0, True, "nchw", "nhwc"),
    "sliver_33x43": (33, 43, 2, 3, "noise", 0.2, 1.0, True, "nhwc", "nhwc"),
    "no_window_tile_42x75": (42, 75, 1, 1, "smooth", 1.0, 1.0, True, "window", "nchw"),
    "one_column_43x74": (43, 74, 1, 2, "noise", LAM_NEAR_ONE, 1.0, True, "nchw", "window"),
    "third_tile_74x42": (74, 42, 1, 1, "noise", 0.2, 1.0, True, "nhwc_spare", "nchw"),
    "third_tile_75x32_nograd": (75, 32, 1, 2, "smooth", 1.0, 1.0, False, "window", "nhwc_spare"),
    "flat_equal": (33, 42, 1, 1, "flat_equal", 0.2, 1.0, True, "nchw", "nchw"),
    "flat_off_centre": (43, 33, 1, 2, "flat_off_centre", 0.2, 1.0, True, "nchw", "nchw"),
    "pred_flat": (32, 43, 1, 1, "pred_flat", 1.0, 1.0, True, "nchw", "nchw"),
    "target_flat": (43, 32, 1, 1, "target_flat", 0.2, 1.0, True, "nchw", "nchw"),
    "flat_across_seam": (33, 75, 1, 1, "flat_seam", 0.2, 1.0, True, "nchw", "nchw"),
    "outlier_centre": (42, 74, 1, 1, "outlier", 1.0, 1.0, True, "nchw", "nchw"),
    "range_255": (43, 42, 1, 3, "range255", 0.2, 255.0, True, "nhwc", "nchw"),
    "offset_1e4": (33, 43, 1, 1, "big", 1.0, 1.0, True, "nchw", "nchw"),
    "offset_1e4_right_tile": (12, 33, 1, 1, "big_right", 1.0, 1.0, True, "nchw", "nchw"),
    "offset_pair": (42, 43, 1, 1, "offset_pair", 0.2, 1.0, True, "nchw", "nchw"),
    "l1_only": (33, 43, 2, 3, "noise", 0.0, 1.0, True, "nhwc", "nchw"),
    "l1_only_equal": (12, 33, 1, 2, "flat_equal", 0.0, 1.0, True, "nchw", "nhwc"),
    "l1_only_nograd_small": (5, 7, 1, 1, "noise", 0.0, 1.0, False, "nchw", "nchw"),
    "ssim_only_nograd": (43, 33, 1, 1, "noise", 1.0, 1.0, False, "nchw", "nchw"),
    "one_target_for_all_views": (32, 42, 3, 2, "smooth", 0.2, 1.0, True, "nchw", "view0"),
    "one_pred_for_all_views": (32, 42, 3, 2, "smooth", 0.2, 1.0, True, "same_views", "nchw"),
    "grey_target": (33, 32, 2, 3, "noise", 0.2, 1.0, True, "nhwc", "chan0"),
    "many_planes_300": (11, 11, 100, 3, "noise", 0.2, 1.0, True, "nchw", "nchw"),
}
SHIFT_CASES = ("outlier_centre", "range_255", "offset_1e4", "offset_1e4_right_tile", "offset_pair")
PHOTO_FAULTS = ("no_shift", "swap_shift", "unclamped_centre", "valid_plus_one", "ownership", "clamp_inverted", "dmu_term", "tap_shift", "l1_sign",
                "norm_hw")


def _content(kind, V, C, H, W, rng):
    r = lambda *s: rng.random(s or (V, C, H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    wave = 0.5 + 0.3 * np.sin(yy / 7.0 + 0.3)[None, None] * np.cos(xx / 9.0)[None, None] + np.zeros((V, C, 1, 1))
    if kind == "noise":
        p, t = r(), r()
    elif kind == "smooth":
        p = wave + 0.01 * r()
        t = wave + 0.02 * r()
    elif kind == "flat_equal":  # pred == target bit for bit: the L1 subgradient is exactly 0, every window flat and equal to the centre
        p = np.full((V, C, H, W), 0.375)
        t = p.copy()
    elif kind == "flat_off_centre":  # flat but for the tiles' centre pixels: every window without one is flat and differs from the shift
        p, t = np.full((V, C, H, W), 0.3), np.full((V, C, H, W), 0.6)
        for y in range(TILE // 2, H, TILE):
            for x in range(TILE // 2, W, TILE):
                p[:, :, y, x], t[:, :, y, x] = 0.7, 0.2
        p[:, :, H - 1, W - 1] = 0.7
    elif kind == "pred_flat":
        p, t = np.full((V, C, H, W), 0.4), r()
        p[:, :, 3, 5] = 0.41
    elif kind == "target_flat":
        p, t = r(), np.full((V, C, H, W), 0.4)
    elif kind == "flat_seam":
        p, t = r(), r()
        p[:, :, :, 18:50], t[:, :, 4:, 20:46] = 0.25, 0.75
    elif kind == "outlier":  # the centre pixel of tile (0, 0) of pred
        p, t = 0.5 + 0.01 * (2 * r() - 1), 0.5 + 0.01 * (2 * r() - 1)
        p[:, :, TILE // 2, TILE // 2] = 1000.0
    elif kind == "range255":
        p = 100.0 + 40.0 * r()
        t = np.clip(p + 4.0 * (2 * r() - 1), 100.0, 140.0)
    elif kind == "big":
        p, t = 1e4 + 0.5 * r(), 1e4 + 0.5 * r()
    elif kind == "big_right":  # the columns the second tile stages (22 ..) sit at 1e4, the rest at 0.5
        p, t = 0.5 + 0.1 * r(), 0.5 + 0.1 * r()
        p[:, :, :, 22:] += 1e4
        t[:, :, :, 22:] += 1e4
    elif kind == "offset_pair":
        p, t = 0.2 + 0.005 * r(), 0.9 + 0.005 * r()
    else:
        raise ValueError(kind)
    p, t = p.astype(np.float32), t.astype(np.float32)
    if kind != "flat_equal":  # the inputs differ everywhere but in the case built for it
        same = p == t
        t[same] = np.nextafter(t[same], np.float32(2e4))
    return p, t


def place(x, kind):
    """x [V,C,H,W] float32 in a layout the ABI's four strides express -> dict(parent (flat, slack = sentinel), offset, strides, shape)"""
    V, C, H, W = x.shape
    off = 0
    if kind == "nchw":
        par, st = x.copy(), (C * H * W, H * W, W, 1)
    elif kind == "nhwc":
        par, st = x.transpose(0, 2, 3, 1).copy(), (H * W * C, 1, W * C, C)
    elif kind == "window":  # a window of a larger buffer
        Hp, Wp = H + 5, W + 7
        par = np.full((V, C, Hp, Wp), SENT_F, np.float32)
        par[:, :, 2:2 + H, 3:3 + W] = x
        st, off = (C * Hp * Wp, Hp * Wp, Wp, 1), 2 * Wp + 3
    elif kind == "nhwc_spare":  # channels-last with a channel nobody owns
        par = np.full((V, H, W, C + 1), SENT_F, np.float32)
        par[..., :C] = x.transpose(0, 2, 3, 1)
        st = (H * W * (C + 1), 1, W * (C + 1), C + 1)
    elif kind == "same_views":  # dense, every view a copy of the first (what the front-end makes of an expanded pred)
        par, st = np.repeat(x[:1], V, 0), (C * H * W, H * W, W, 1)
    elif kind == "view0":  # one target for all views
        par, st = x[:1].copy(), (0, H * W, W, 1)
    elif kind == "chan0":  # a grey target under a colour pred
        par, st = x[:, :1].copy(), (H * W, 0, W, 1)
    else:
        raise ValueError(kind)
    return dict(parent=np.ascontiguousarray(par).reshape(-1), offset=off, strides=st, shape=(V, C, H, W))


def logical(lay, parent=None):
    """the [V,C,H,W] array a layout addresses (a copy)"""
    par = lay["parent"] if parent is None else parent
    return np.lib.stride_tricks.as_strided(par[lay["offset"]:], lay["shape"], tuple(4 * s for s in lay["strides"])).copy()


def owned_mask(lay):
    """flat bool over the parent: the elements the layout addresses"""
    m = np.zeros(lay["parent"].shape, bool)
    np.lib.stride_tricks.as_strided(m[lay["offset"]:], lay["shape"], lay["strides"])[...] = True
    return m


@functools.lru_cache(maxsize=None)
def photo_case(name):
    H, W, V, C, kind, lam, dr, grad, pl, tl = PHOTO_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    p, t = _content(kind, V, C, H, W, rng)
    play, tlay = place(p, pl), place(t, tl)
    P, T = logical(play), logical(tlay)
    if kind != "flat_equal":
        same = P == T
        if same.any():  # (a layout that repeats a view or a channel can bring equal values together again)
            assert pl in ("nchw", "same_views")
            play["parent"][:] = np.where(same, np.nextafter(P, np.float32(2e4)), P).reshape(-1)
            P = logical(play)
        assert not (P == T).any()
    return dict(name=name, H=H, W=W, V=V, C=C, lam=float(np.float32(lam)), dr=float(np.float32(dr)), grad=grad, play=play, tlay=tlay, P=P, T=T)


def _tiles(H, W):
    return [(ty, tx) for ty in range(-(-H // TILE)) for tx in range(-(-W // TILE))]


def _blur_t(D, g=G64):
    """transposed valid blur: windows [N,a,b] -> pixels [N,a+10,b+10]"""
    N, a, b = D.shape
    out = np.zeros((N, a + TAPS - 1, b + TAPS - 1))
    for i in range(TAPS):
        for j in range(TAPS):
            out[:, i:i + a, j:j + b] += g[i] * g[j] * D
    return out


def _weights(c):
    lam, dr = c["lam"], c["dr"]
    do_ssim, do_l1 = lam != 0.0, lam != 1.0
    n_l1 = float(c["V"] * c["C"] * c["H"] * c["W"])
    n_ssim = float(c["V"] * c["C"] * (c["H"] - 10) * (c["W"] - 10)) if do_ssim else 1.0
    return do_ssim, do_l1, n_l1, n_ssim, (K1 * dr) ** 2, (K2 * dr) ** 2


@functools.lru_cache(maxsize=None)
def photo_ref(name, shifted=True):
    """everything siu3r_photo_loss writes, in float64, with the scale of every element and the branch population.  shifted=False:
    the scales of a kernel WITHOUT the per-tile shift (moments rounding in units of max |p|^2), which test_photo_loss_ref.py uses for the
    float64-autograd comparison (2^-53 instead of u) and to show what the shift buys."""
    c = photo_case(name)
    V, C, H, W, grad = c["V"], c["C"], c["H"], c["W"], c["grad"]
    N = V * C
    P, T = c["P"].reshape(N, H, W).astype(np.float64), c["T"].reshape(N, H, W).astype(np.float64)
    do_ssim, do_l1, n_l1, n_ssim, c1, c2 = _weights(c)
    lam = c["lam"]
    w_l1, w_ssim = (1.0 - lam) / n_l1, (-lam / n_ssim if do_ssim else 0.0)
    tiles = _tiles(H, W)
    nt = len(tiles)
    part, S_part = np.zeros((N, nt, 2)), np.zeros((N, nt, 2))
    G, S_G, X_G = np.zeros((N, H, W)), np.zeros((N, H, W)), np.zeros((N, H, W))
    pop = dict(windows=0, clamp_pp=0, clamp_tt=0, undecided=0, tiles_without_window=0, halo_windows=0, equal_pixels=int((P == T).sum()), tiles=nt)
    G2 = np.outer(G64, G64)
    sq = np.sqrt(G64)
    for ti, (ty, tx) in enumerate(tiles):
        y0, x0 = ty * TILE, tx * TILE
        y1, x1 = min(y0 + TILE, H), min(x0 + TILE, W)
        d = P[:, y0:y1, x0:x1] - T[:, y0:y1, x0:x1]
        if do_l1:
            part[:, ti, 0] = np.abs(d).sum((1, 2))
            S_part[:, ti, 0] = 14 * part[:, ti, 0]
            G[:, y0:y1, x0:x1] += w_l1 * np.sign(d)
            S_G[:, y0:y1, x0:x1] += 3 * w_l1 * np.abs(np.sign(d))  # (pred == target: exactly 0)
        if not do_ssim:
            continue
        wlo = TAPS - 1 if grad else 0
        # the windows the workgroup evaluates and that are valid: those that reach its pixels (grad) or that it owns
        wy0, wy1 = max(y0 - wlo, 0), min(y1 - 1 if grad else y0 + TILE - 1, H - TAPS)
        wx0, wx1 = max(x0 - wlo, 0), min(x1 - 1 if grad else x0 + TILE - 1, W - TAPS)
        own_y = (np.arange(wy0, wy1 + 1) >= y0)[:, None]
        own_x = (np.arange(wx0, wx1 + 1) >= x0)[None, :]
        own = (own_y & own_x)[None]
        if wy1 < wy0 or wx1 < wx0 or not own.any():
            pop["tiles_without_window"] += 1
        if wy1 < wy0 or wx1 < wx0:
            continue
        yc, xc = min(y0 + TILE // 2, H - 1), min(x0 + TILE // 2, W - 1)
        cp, ct = P[:, yc, xc][:, None, None], T[:, yc, xc][:, None, None]
        sy0, sy1, sx0, sx1 = max(y0 - wlo, 0), min(y0 + TILE + TAPS - 1, H), max(x0 - wlo, 0), min(x0 + TILE + TAPS - 1, W)
        if shifted:
            Mp = np.abs(P[:, sy0:sy1, sx0:sx1] - cp).max((1, 2), keepdims=True)
            Mt = np.abs(T[:, sy0:sy1, sx0:sx1] - ct).max((1, 2), keepdims=True)
        else:
            Mp = np.abs(P[:, sy0:sy1, sx0:sx1]).max((1, 2), keepdims=True)
            Mt = np.abs(T[:, sy0:sy1, sx0:sx1]).max((1, 2), keepdims=True)
        ps, ts = P[:, wy0:wy1 + TAPS, wx0:wx1 + TAPS] - cp, T[:, wy0:wy1 + TAPS, wx0:wx1 + TAPS] - ct
        wp = np.lib.stride_tricks.sliding_window_view(ps, (TAPS, TAPS), axis=(1, 2))
        wt = np.lib.stride_tricks.sliding_window_view(ts, (TAPS, TAPS), axis=(1, 2))
        mps, mts = np.einsum("nabij,ij->nab", wp, G2), np.einsum("nabij,ij->nab", wt, G2)
        dp, dt = wp - mps[..., None, None], wt - mts[..., None, None]
        spp, stt, spt = np.einsum("nabij,ij->nab", dp * dp, G2), np.einsum("nabij,ij->nab", dt * dt, G2), np.einsum("nabij,ij->nab", dp * dt, G2)
        mp, mt = mps + cp, mts + ct
        amp, amt = np.abs(mp), np.abs(mt)
        A1, A2, B1, B2 = 2 * mp * mt + c1, 2 * spt + c2, mp * mp + mt * mt + c1, spp + stt + c2
        s = A1 * A2 / (B1 * B2)
        # running error count, units of u
        z = np.zeros_like(s)
        e_mps, e_mts = K_MEAN * Mp + z, K_MEAN * Mt + z
        e_mp, e_mt = e_mps + amp, e_mts + amt
        e_spp, e_stt, e_spt = K_VAR * Mp * Mp + z, K_VAR * Mt * Mt + z, K_VAR * Mp * Mt + z
        e_A1 = 2 * (amt * e_mp + amp * e_mt) + 2 * amp * amt + np.abs(A1) + 3 * c1
        e_A2 = 2 * e_spt + np.abs(A2) + 3 * c2
        e_B1 = 2 * amp * e_mp + 2 * amt * e_mt + mp * mp + mt * mt + 2 * B1 + 3 * c1
        e_B2 = e_spp + e_stt + 2 * B2 + 3 * c2
        B1l, B2l = np.maximum(B1 - 2 * U24 * e_B1, 0.99 * c1), np.maximum(B2 - 2 * U24 * e_B2, 0.99 * c2)
        A1h, A2h = np.abs(A1) + 2 * U24 * e_A1, np.abs(A2) + 2 * U24 * e_A2
        iBh = 1.0 / (B1l * B2l)
        r_iB = e_B1 / B1l + e_B2 / B2l + 3
        sh = A1h * A2h * iBh
        e_s = A2h * iBh * e_A1 + A1h * iBh * e_A2 + sh * (r_iB + 2)
        part[:, ti, 1] = (s * own).sum((1, 2))
        S_part[:, ti, 1] = (e_s * own).sum((1, 2)) + 16 * (sh * own).sum((1, 2))
        und = spp <= U24 * e_spp
        pos = ~und
        pop["windows"] += int(own.sum()) * N
        pop["halo_windows"] += int((~own).sum()) * N
        pop["clamp_pp"] += int(((spp <= 0) & own).sum())
        pop["clamp_tt"] += int(((stt <= U24 * e_stt) & own).sum())
        pop["undecided"] += int(((und & (np.abs(mps) > 0)) & own).sum())
        if not grad:
            continue
        dpp = np.where(pos, -s / B2, 0.0)
        dpp_m = sh / B2l
        e_dpp = e_s / B2l + dpp_m * (e_B2 / B2l + 2)
        dpt, dpt_m = 2 * A1 / (B1 * B2), 2 * A1h * iBh
        e_dpt = 2 * iBh * e_A1 + dpt_m * (r_iB + 1)
        a_m, b_m = 2 * amt * A2h * iBh, 2 * amp * sh / B1l
        e_a = 2 * A2h * iBh * e_mt + 2 * amt * iBh * e_A2 + a_m * (r_iB + 2)
        e_b = 2 * sh / B1l * e_mp + 2 * amp / B1l * e_s + b_m * (e_B1 / B1l + 4)
        dmu_c = 2 * mt * A2 / (B1 * B2) - 2 * mp * s / B1
        t1, t2 = 2 * dpp_m * np.abs(mps), dpt_m * np.abs(mts)
        dmu = dmu_c - 2 * dpp * mps - dpt * mts
        dmu_m = a_m + b_m + t1 + t2
        e_dmu = e_a + e_b + (a_m + b_m) + 2 * (np.abs(mps) * e_dpp + dpp_m * e_mps) + 2 * t1 + (np.abs(mts) * e_dpt + dpt_m * e_mts) + 2 * t2 + 2 * dmu_m
        # pixels [wy0, wy1 + 10] x [wx0, wx1 + 10]; the tile's own are a slice of them
        oy, ox = y0 - wy0, x0 - wx0
        cut = lambda a: a[:, oy:oy + (y1 - y0), ox:ox + (x1 - x0)]
        o0, o1, o2 = cut(_blur_t(dmu)), cut(_blur_t(dpp)), cut(_blur_t(dpt))
        m0, m1, m2 = cut(_blur_t(dmu_m)), cut(_blur_t(dpp_m)), cut(_blur_t(dpt_m))
        E0, E1, E2 = cut(_blur_t(e_dmu)) + K_BLUR * m0, cut(_blur_t(e_dpp)) + K_BLUR * m1, cut(_blur_t(e_dpt)) + K_BLUR * m2
        pp_, tt_ = P[:, y0:y1, x0:x1] - cp, T[:, y0:y1, x0:x1] - ct
        app, att = np.abs(pp_), np.abs(tt_)
        g = o0 + 2 * pp_ * o1 + tt_ * o2
        g_m = m0 + 2 * app * m1 + att * m2
        S = E0 + 2 * app * (E1 + 3 * m1) + att * (E2 + 3 * m2) + 2 * g_m
        extra = 2 * cut(_blur_t(und * dpp_m * np.sqrt(spp), sq))
        G[:, y0:y1, x0:x1] += w_ssim * g
        S_G[:, y0:y1, x0:x1] += abs(w_ssim) * (S + 3 * g_m)
        X_G[:, y0:y1, x0:x1] += abs(w_ssim) * extra
    l1, ss = part[:, :, 0].sum() / n_l1, part[:, :, 1].sum() / n_ssim
    S_l1, S_ss = S_part[:, :, 0].sum() / n_l1 + 2 * abs(l1), S_part[:, :, 1].sum() / n_ssim + 2 * abs(ss)
    loss = (1.0 - lam) * l1 * do_l1 + lam * (1.0 - ss) * do_ssim
    nan = float("nan")
    out = np.array([loss, l1 if do_l1 else nan, ss if do_ssim else nan])
    S_out = np.array([(1.0 - lam) * S_l1 * do_l1 + lam * S_ss * do_ssim + 2 * abs(loss), S_l1, S_ss])
    r = dict(out=out, S_out=S_out, partials=part.reshape(N * nt, 2), S_partials=S_part.reshape(N * nt, 2), pop=pop, grad=None, S_grad=None, extra_grad=None)
    if grad:
        r.update(grad=G.reshape(V, C, H, W), S_grad=S_G.reshape(V, C, H, W), extra_grad=X_G.reshape(V, C, H, W))
    return r


# ---- the kernel's arithmetic in float32 --------------------------------------------------------------------------------------------------
F4, F8 = np.float32, np.float64


def _fma(a, b, c):
    """fmaf: the product of two float32 is exact in float64"""
    return (np.asarray(a, F8) * np.asarray(b, F8) + np.asarray(c, F8)).astype(F4)


def _block_sum(th):
    """block_reduce<Sum>: th [N,256] per-thread values -> [N]; the shuffle tree of each wave (lane 0's value), then the waves in order"""
    w = th.reshape(th.shape[0], 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :o] + w[:, :, o:2 * o]
    w = w[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def photo_emulate(name, fault=None):
    """siu3r_photo_loss in numpy float32 (fp64 where the kernel is): the same shift, tap order, fused adds, tile partition and reduction
    trees.  fault: one of PHOTO_FAULTS, the kernel with that one line wrong.  -> dict(out, partials, grad or None)"""
    c = photo_case(name)
    V, C, H, W, grad = c["V"], c["C"], c["H"], c["W"], c["grad"]
    N = V * C
    P, T = c["P"].reshape(N, H, W), c["T"].reshape(N, H, W)
    do_ssim, do_l1, n_l1, n_ssim, _, _ = _weights(c)
    if fault == "norm_hw":
        n_ssim = float(N * H * W)
    dr = F4(c["dr"])
    c1, c2 = (F4(0.01) * dr) * (F4(0.01) * dr), (F4(0.03) * dr) * (F4(0.03) * dr)
    w_l1, w_ssim = F4((1.0 - c["lam"]) / n_l1), F4(-c["lam"] / n_ssim)
    tiles = _tiles(H, W)
    part = np.zeros((N, len(tiles), 2), F4)
    G = np.zeros((N, H, W), F4)
    tid = np.arange(256)
    for ti, (ty, tx) in enumerate(tiles):
        y0, x0 = ty * TILE, tx * TILE
        y1, x1 = min(y0 + TILE, H), min(x0 + TILE, W)
        th, tw = y1 - y0, x1 - x0
        # L1 over the tile's pixels: thread t takes (t / 32 + 8 k, t % 32), k = 0 .. 3
        d = np.zeros((N, TILE, TILE), F4)
        d[:, :th, :tw] = P[:, y0:y1, x0:x1] - T[:, y0:y1, x0:x1]
        sgn = np.sign(d)
        if fault == "l1_sign" and y1 == H and x1 == W:
            sgn[N - 1, th - 1, tw - 1] *= -1
        if do_l1:
            acc = np.zeros((N, 256), F4)
            for k in range(4):
                acc = acc + np.abs(d)[:, tid // TILE + 8 * k, tid % TILE]
            part[:, ti, 0] = _block_sum(acc)
        g_l1 = (sgn * w_l1)[:, :th, :tw] if do_l1 else np.zeros((N, th, tw), F4)
        if not do_ssim:
            G[:, y0:y1, x0:x1] = g_l1
            continue
        WLO = TAPS - 1 if grad else 0
        NW = TILE + WLO
        NP = NW + TAPS - 1
        yc, xc = min(y0 + TILE // 2, H - 1), min(x0 + TILE // 2, W - 1)
        if fault == "unclamped_centre":  # the address of (y0 + 16, x0 + 16) in a dense plane, wrapped into it
            flat = ((y0 + TILE // 2) * W + x0 + TILE // 2) % (H * W)
            yc, xc = flat // W, flat % W
        cp, ct = P[:, yc, xc][:, None, None], T[:, yc, xc][:, None, None]
        if fault == "no_shift":
            cp, ct = np.zeros_like(cp), np.zeros_like(ct)
        if fault == "swap_shift":
            cp, ct = ct, cp
        ys, xs = np.arange(y0 - WLO, y0 - WLO + NP), np.arange(x0 - WLO, x0 - WLO + NP)
        inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        yi, xi = np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]
        sP, sT = np.where(inside[None], P[:, yi, xi], cp), np.where(inside[None], T[:, yi, xi], ct)
        p_, t_ = sP - cp, sT - ct
        h = [np.zeros((N, NP, NW), F4) for _ in range(5)]
        for m in range(TAPS):
            pm, tm = p_[:, :, m:m + NW], t_[:, :, m:m + NW]
            gp, gt = GW32[m] * pm, GW32[m] * tm
            h[0], h[1] = h[0] + gp, h[1] + gt
            h[2], h[3], h[4] = _fma(gp, pm, h[2]), _fma(gp, tm, h[3]), _fma(gt, tm, h[4])
        a = [np.zeros((N, NW, NW), F4) for _ in range(5)]
        for q in range(5):
            for m in range(TAPS):
                a[q] = _fma(GW32[m], h[q][:, m:m + NW, :], a[q])
        wy, wx = (y0 - WLO + np.arange(NW))[:, None], (x0 - WLO + np.arange(NW))[None, :]
        valid = (wy >= 0) & (wy <= H - TAPS) & (wx >= 0) & (wx <= W - TAPS + (1 if fault == "valid_plus_one" else 0))
        mp_s, mt_s = a[0], a[1]
        mp, mt = mp_s + cp, mt_s + ct
        spp_raw, stt_raw, spt = a[2] - mp_s * mp_s, a[4] - mt_s * mt_s, a[3] - mp_s * mt_s
        spp, stt = np.maximum(spp_raw, F4(0)), np.maximum(stt_raw, F4(0))
        A1, A2 = F4(2) * mp * mt + c1, F4(2) * spt + c2
        B1, B2 = mp * mp + mt * mt + c1, spp + stt + c2
        iB = F4(1) / (B1 * B2)
        s = A1 * A2 * iB
        own = valid & (np.arange(NW) >= WLO)[:, None] & (np.arange(NW) >= WLO)[None, :]
        if fault == "ownership":
            own = valid
        sm = np.where(own[None], s, F4(0))
        R, NSEG = 7, -(-NW // 7)
        acc = np.zeros((N, 256), F4)
        for seg in range(NSEG):
            for r in range(R):
                if seg * R + r < NW:
                    acc[:, seg * NW:(seg + 1) * NW] = acc[:, seg * NW:(seg + 1) * NW] + sm[:, seg * R + r, :]
        part[:, ti, 1] = _block_sum(acc)
        if not grad:
            continue
        take = (spp_raw <= 0) if fault == "clamp_inverted" else (spp_raw > 0)
        d_epp = np.where(take, -s / B2, F4(0))
        d_ept = F4(2) * A1 * iB
        dmu_c = F4(2) * mt * A2 * iB - F4(2) * mp * s / B1
        dmu = dmu_c - d_ept * mt_s if fault == "dmu_term" else dmu_c - F4(2) * d_epp * mp_s - d_ept * mt_s
        sD = [np.where(valid[None], x, F4(0)).astype(F4) for x in (dmu, d_epp, d_ept)]
        o = []
        for q in range(3):
            e = np.zeros((N, TILE, NW), F4)
            for m in range(TAPS):
                wgt = (GW32[m - 1] if m else F4(0)) if fault == "tap_shift" else GW32[m]
                e = _fma(wgt, sD[q][:, m:m + TILE, :], e)
            f = np.zeros((N, TILE, TILE), F4)
            for m in range(TAPS):
                f = _fma(GW32[m], e[:, :, m:m + TILE], f)
            o.append(f)
        ps_, ts_ = p_[:, WLO:WLO + TILE, WLO:WLO + TILE], t_[:, WLO:WLO + TILE, WLO:WLO + TILE]
        sO = o[0] + F4(2) * ps_ * o[1] + ts_ * o[2]
        g = (w_ssim * sO)[:, :th, :tw]
        G[:, y0:y1, x0:x1] = g + g_l1 if do_l1 else g
    pd = part.reshape(N * len(tiles), 2).astype(F8)
    l1, ss = pd[:, 0].sum() / n_l1, pd[:, 1].sum() / n_ssim
    lam = c["lam"]
    loss = (1.0 - lam) * l1 * do_l1 + lam * (1.0 - ss) * do_ssim
    out = np.array([loss, l1 if do_l1 else np.nan, ss if do_ssim else np.nan]).astype(F4)
    return dict(out=out, partials=part.reshape(N * len(tiles), 2), grad=G.reshape(V, C, H, W) if grad else None)


def photo_compare(got, ref, close):
    """every output of one call against photo_ref under the derived bound; `close(got, ref, S, bound, name, extra)` asserts or measures.
    -> the worst ratio per output"""
    w = dict(out=close(got["out"], ref["out"], ref["S_out"], PHOTO_BOUND, "out", None),
             partials=close(got["partials"], ref["partials"], ref["S_partials"], PHOTO_BOUND, "partials", None))
    if ref["grad"] is not None:
        w["grad"] = close(got["grad"], ref["grad"], ref["S_grad"], PHOTO_BOUND, "grad", ref["extra_grad"])
    return w
