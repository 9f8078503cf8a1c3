"""Float64 reference of the absolute-gradient (AbsGS, Ye et al. 2024) densification statistics that siu3r_raster_composite_rgb_bwd_abs
(siu3r_amd/csrc/raster_bwd.hip, composite_rgb_bwd_kernel<false, ABS = true>) sums next to the signed record: per Gaussian of one view,

    abs[g, 0] = sum over the pixels p that blend g of |d loss / d mean_x of g through p|,      abs[g, 1] likewise for mean_y,

the absolute value taken per pixel, before any sum.  It stands on the walk of tests/dense_raster_bwd64.py (`_walk`, `_tile_pixels`,
imported): the same entries front to back, the same branch rules as composite_bwd64 -- a term exists where the pixel blends the entry
and its alpha is not on the alpha_max clamp -- and the same float64 arithmetic, so its SIGNED sums are composite_bwd64's grad[:, MX / MY]
up to the order of the additions (tests/test_absgrad_ref.py holds them to 1e-12 S, and pins "absolute value per pixel, then sum" through
the linearity of the backward in its upstream gradient, without the hand-written terms below).

TOLERANCE.  No new number.  |x| is 1-Lipschitz: each pixel's |term| is off by at most what the term is off by, so the absolute sum inherits
the bound of the signed element of the same case, with composite_bwd64's S, chain and n_add (`_chain_errors` enters through them):
    |got - ref| <= comp_bound(n_add) S[:, k] + chain[:, k],   k = MX, MY.

Not a test module."""
import functools

import numpy as np

import dense_raster_bwd64 as B
from dense_raster_bwd64 import MX, MY, _tile_pixels, _walk


def abs_mean2d64(cam, rec, lists, g_out, g_alpha, g_depth, cache=None):
    """One K2 view.  rec [G,12] the fp32 records, lists = (tile_start [T+1], ids) front to back, g_out [3,H,W], g_alpha, g_depth [H,W].
    cache: the {tile: (walk, ...)} dict composite_bwd64 filled for the same case (the walks do not depend on the upstream gradients).
    -> dict abs [G,2] (the statistics), signed [G,2] (the same terms summed with their signs), n_term [G] (non-zero pixel terms)"""
    H, W = cam.height, cam.width
    rec = np.asarray(rec, np.float64)
    G = rec.shape[0]
    tile_start, ids_all = np.asarray(lists[0], np.int64), np.asarray(lists[1], np.int64)
    gC_img = np.asarray(g_out, np.float64).transpose(1, 2, 0)
    gD_img, gO_img = np.asarray(g_depth, np.float64), np.asarray(g_alpha, np.float64)
    bg = np.array(list(cam.bg), np.float64)
    out_abs, out_signed, n_term = np.zeros((G, 2)), np.zeros((G, 2)), np.zeros(G, np.int64)
    for tile in range(tile_start.shape[0] - 1):
        ids = ids_all[tile_start[tile]:tile_start[tile + 1]]
        if ids.shape[0] == 0:
            continue
        px, py, inside, off = _tile_pixels(cam, tile, False)
        w = cache[tile][0] if cache is not None and tile in cache else _walk(cam, rec[ids], px, py, inside, off, False, False)
        bl, a, Tb = w["bl"], w["a"], w["Tb"]
        pi, pj = np.minimum(py, H - 1), np.minimum(px, W - 1)
        gC = np.where(inside[:, None], gC_img[pi, pj], 0.0)
        gD, gO = np.where(inside, gD_img[pi, pj], 0.0), np.where(inside, gO_img[pi, pj], 0.0)
        wt = np.where(bl, a * Tb, 0.0)  # [L,P] blend weights
        gdc = rec[ids, 8:11] @ gC.T + rec[ids, 2][:, None] * gD[None] + gO[None]  # g . (colour, depth, 1) of the entry
        q = gdc * wt
        behind = np.cumsum(q[::-1], 0)[::-1] - q + (w["T"] * (gC @ bg))[None]  # everything the pixel blends behind the entry, background included
        dLda = np.where(bl & ~w["clamped"], Tb * gdc - behind / (1.0 - a), 0.0)  # (alpha on the clamp: constant, no term)
        dLds = -dLda * a
        tx = dLds * (w["ca"] * w["dx"] + w["cb"] * w["dy"])
        ty = dLds * (w["cc"] * w["dy"] + w["cb"] * w["dx"])
        for k, tv in ((0, tx), (1, ty)):
            np.add.at(out_abs[:, k], ids, np.abs(tv).sum(1))
            np.add.at(out_signed[:, k], ids, tv.sum(1))
        np.add.at(n_term, ids, ((tx != 0) | (ty != 0)).sum(1))
    return dict(abs=out_abs, signed=out_signed, n_term=n_term)


def abs_tolerance(ref):
    """comp_bound(n_add) S[:, MX / MY] + chain[:, MX / MY] of a composite_bwd64 result -> [G,2]"""
    return ref["bound"] * ref["S"][:, [MX, MY]] + ref["chain"][:, [MX, MY]]


def case_abs_ref(case, refs, ups):
    """per view abs_mean2d64 of a composite case (dense_raster_bwd64.comp_case, or a dict of the same keys) on the upstream gradients
    B.comp_ref returned with `refs` (margin pixels zeroed)"""
    assert case["kind"] == "k2"
    return [abs_mean2d64(case["cams"][v], case["rec"][v], case["lists"][v], ups["g_out"][v], ups["g_alpha"][v], ups["g_depth"][v], cache=case["walk_cache"][v])
            for v in range(case["V"])]


def small_case(name, W, H, rows, ups):
    """a one-view K2 composite case from hand-placed screen-space Gaussians, binned like dense_raster_bwd64.comp_case does it.
    rows [G,10] = (mx, my, sx, sy, theta, opacity, depth, r, g, b); ups: g_out [1,3,H,W], g_alpha, g_depth [1,H,W] fp32"""
    import torch

    import raster_stages_ref as RS

    p = np.asarray(rows, np.float64)
    G = p.shape[0]
    rec = np.zeros((G, 12))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7] = p[:, 0], p[:, 1], p[:, 6], p[:, 5]
    rec[:, 4], rec[:, 5], rec[:, 6] = B._conic(p[:, 2], p[:, 3], p[:, 4])
    rec[:, 8:11] = p[:, 7:10]
    rec = rec.astype(np.float32)[None]
    rect = B._rects(W, H, p[:, 0], p[:, 1], 3.33 * np.maximum(p[:, 2], p[:, 3]))[None]
    geo = RS.geometry_ref(W, H)
    live = (rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1]) != 0
    keys = np.where(live, rec[..., 2].view(np.uint32), np.uint32(RS.CULLED)).astype(np.uint32)
    sorted_ids = [s[1] for s in RS.sort_ref(keys)]
    bins = [RS.bin_ref(geo, sorted_ids[0], rect[0])]
    lists = [RS.tile_lists_ref(geo, *bins[0])]
    return dict(name=name, kind="k2", W=W, H=H, V=1, G=G, C=3, cams=[B.k2_cam(W, H, torch.eye(4, dtype=B.DD))], geo=geo, rec=rec, rect=rect, sorted_ids=sorted_ids,
                bins=bins, lists=lists, ups={k: np.asarray(v, np.float32) for k, v in ups.items()}, feats=None, scene="hand", walk_cache=[{}])


@functools.lru_cache(maxsize=None)
def one_tile_case():
    """a frame of one tile (16 x 16): fourteen Gaussians of mixed size in and around it, two of them nearly opaque (pixels on the
    alpha_max clamp), random upstream gradients of all three outputs"""
    rng = np.random.default_rng(1601)
    n = 14
    op = rng.uniform(0.1, 0.9, n)
    op[:2] = 0.999
    rows = np.stack([rng.uniform(-2, 18, n), rng.uniform(-2, 18, n), rng.uniform(1.0, 5.0, n), rng.uniform(1.0, 5.0, n), rng.uniform(0, np.pi, n), op,
                     rng.uniform(0.5, 5.0, n), *rng.uniform(0.0, 1.2, (3, n))], -1)
    rows[:2, :2] = [[5.0, 6.0], [11.0, 9.0]]  # (opacity * exp exceeds alpha_max only within a tenth of sigma of the mean: on pixel centres)
    ups = dict(g_out=rng.normal(size=(1, 3, 16, 16)), g_alpha=rng.normal(size=(1, 16, 16)), g_depth=rng.normal(size=(1, 16, 16)))
    return small_case("one_tile", 16, 16, rows, ups)


@functools.lru_cache(maxsize=None)
def cancel_case():
    """the case the statistics exist for: ONE isotropic Gaussian (sigma 4 px, opacity 0.1, red 1.0 over the camera's background 0.1) centred on
    the integer pixel position (16, 16) of a 32 x 32 frame -- the common corner of its four tiles; K2 pixel centres are integers, so the
    pixels come in mirror pairs about the centre (the footprint, 10.2 px where alpha >= 1 / 255, ends inside the frame).  The upstream
    gradient is even about the centre: red constant 1, nothing else.  Every pixel pulls the mean towards itself by as much as its mirror
    pixel pulls it away: the signed sums are 0, the absolute ones are not.  The low opacity keeps S, which counts the part behind an
    entry with 1 / (1 - alpha), within 2 x the absolute sum."""
    ups = dict(g_out=np.zeros((1, 3, 32, 32)), g_alpha=np.zeros((1, 32, 32)), g_depth=np.zeros((1, 32, 32)))
    ups["g_out"][:, 0] = 1.0
    return small_case("cancel", 32, 32, [[16.0, 16.0, 4.0, 4.0, 0.0, 0.1, 2.0, 1.0, 0.5, 0.5]], ups)


def case(name):
    hand = {"one_tile": one_tile_case, "cancel": cancel_case}
    return hand[name]() if name in hand else B.comp_case(name)


@functools.lru_cache(maxsize=None)
def crafted_ref(name, mode="all"):
    """-> (refs, ups, abs_refs) of a crafted case of B.COMP_CASES, or of "one_tile" / "cancel": computed once per (case, mode), shared by
    the tests, read-only"""
    c = case(name)
    refs, ups = B.comp_ref(c, mode)
    return refs, ups, case_abs_ref(c, refs, ups)
