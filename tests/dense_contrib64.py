"""Float64 windows, float32 emulation and crafted cases of the blend-contribution statistics (siu3r_amd/csrc/contrib.hip,
siu3r_raster_contrib), written from include/siu3r_hip.h; shared by tests/test_contrib_ref.py (CPU) and tests/test_contrib_gpu.py (GPU).

The walk, its chain errors and the decision margins are those of the forward composite: composite_fwd64 (tests/dense_raster_fwd64.py)
returns the float64 walk of every tile (bl: the entry blends in the pixel, a, Tb: the transmittance in front of it, reached) and the
margin of every pixel; MARGIN (4) and dense_raster_bwd64._chain_errors are used as they are.  With w = a Tb, e_w = e_a + e_T in front
of the entry, u = 2^-24 (the rounding of the product a T), a pixel DECIDED when its margin is at least MARGIN:

  count   in [lo, hi]: lo = the decided pixels that blend g, hi = lo + the undecided pixels that reach g (the n_touched pattern) and in
          which g's own tests do not rule a blend out: sigma < 0, or alpha < alpha_min, by MARGIN of their own errors (the two static terms
          of dense_raster_bwd64._tile_margin, per entry; they do not depend on the chain in front of the entry, so no earlier flip of an
          undecided pixel can undo them.  Without this a needle whose rect spans the frame counts every undecided pixel of the frame)
  wmax    in [max over the decided blended pixels of w (1 - e_w - u), max over the pixels that can hold g of w (1 + e_w + u)]; a pixel can
          hold g when it is decided and blends it, or undecided and reaches it (a decided pixel that does not blend g in float64 does not
          in float32 either: it adds nothing to the upper end)
  wsum    |wsum 2^-40 - sum over the blended pixels of w| <= sum w (e_w + u) + hi 2^-40 + the w of the undecided pixels that reach g
          (one truncation of less than 2^-40 per counted pixel)

Rows that no pixel can hold have the window [0, 0] in all three: the kernel leaves them exactly 0.

Not a test module."""
import copy
import functools

import numpy as np
import torch

import dense_raster_bwd64 as B
import dense_raster_fwd64 as F
import raster_stages_ref as RS

U24 = B.U24
MARGIN = B.MARGIN
ZERO_SHARE_CAP = B.ZERO_SHARE_CAP
TILE = B.TILE
F32 = np.float32
UNIT = 2.0 ** -40

# ---- the crafted cases: the smallest shapes at which the kernel can go wrong -----------------------------------------------------------------
#                kind-free: W   H  V  scene
NEW_CASES = {
    "span4":  (40, 24, 2, "span4"),
    "wall":   (40, 24, 2, "wall"),
    "clamp":  (40, 24, 2, "clamp"),
    "culled": (40, 24, 2, "culled"),
    "crowd":  (16, 16, 1, "crowd"),
}
CROWD_G = 700
NEW_NAMES = [f"{k}_{n}" for n in NEW_CASES for k in ("k2", "k3")]
OLD_NAMES = [n for n in list(B.COMP_CASES) + list(F.FWD_COMP_CASES) if (B.COMP_CASES.get(n) or F.FWD_COMP_CASES[n])[0] != "feat"]
ALL_NAMES = OLD_NAMES + NEW_NAMES


def _scene_view(kind, W, H, scene, rng, v):
    """one view's records in screen space -> rec [G,12] fp32, rect [G,4], the rows that must stay exactly 0 (bool [G])"""
    parts, zero = [], []
    half = 0.5 if kind == "k3" else 0.0

    def add(n, mx, my, sx, sy, op, depth, hidden=False):
        parts.append(np.stack([np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in (mx, my, sx, sy, rng.uniform(0, np.pi, n), op, depth)], -1))
        zero.append(np.full(n, hidden))

    if scene == "crowd":  # ~700 Gaussians that all cover the one tile: more than STG = 512 survivors, no pixel saturates
        n = CROWD_G
        add(n, rng.uniform(1, 15, n), rng.uniform(1, 15, n), rng.uniform(1.5, 3.0, n), rng.uniform(1.5, 3.0, n), rng.uniform(0.005, 0.012, n),
            1.0 + 1e-3 * rng.permutation(n))
    else:
        n = 60
        add(n, rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n), rng.uniform(0.8, 2.5, n), rng.uniform(0.8, 2.5, n), rng.uniform(0.05, 0.9, n),
            rng.uniform(1.0, 3.0, n))
        if scene == "span4":  # footprints over the corner of four tiles: the cross-workgroup merge of max and sum
            add(3, 16.0 + rng.uniform(-0.4, 0.4, 3), 16.0 + rng.uniform(-0.4, 0.4, 3), 3.0, 3.0, (0.7, 0.4, 0.2), (0.5, 1.5, 2.5))
            add(1, 31.7, 15.8, 2.0, 4.0, 0.6, 0.8)
        elif scene == "wall":
            # an opaque front wall (view 0: the whole frame; view 1: its left part): the fourth entry saturates every pixel under it; the
            # entries behind never blend there
            sx = 400.0 if v == 0 else 7.0
            add(6, 8.0 + rng.uniform(-0.5, 0.5, 6), 12.0 + rng.uniform(-0.5, 0.5, 6), sx, 400.0, 0.95, 0.3 + 0.01 * np.arange(6))
            add(14, rng.uniform(1, 9, 14), rng.uniform(2, H - 2, 14), 0.6, 0.6, rng.uniform(0.3, 0.9, 14), rng.uniform(3.5, 4.0, 14), hidden=True)
            add(6, rng.uniform(2, W - 2, 6), rng.uniform(2, H - 2, 6), 1.0, 1.0, 0.5, rng.uniform(0.1, 0.2, 6))  # in front of the wall
        elif scene == "clamp":  # opacity x exp above alpha_max next to the mean (means on pixel centres)
            hi_op = 0.999 if kind == "k2" else 0.9995
            add(8, np.floor(rng.uniform(3, W - 3, 8)) + half, np.floor(rng.uniform(3, H - 3, 8)) + half, rng.uniform(2, 4, 8), rng.uniform(2, 4, 8), hi_op,
                rng.uniform(0.5, 0.9, 8))
        elif scene == "culled":
            add(6, rng.uniform(-60, -30, 6), rng.uniform(0, H, 6), 1.0, 1.0, 0.8, rng.uniform(1, 3, 6), hidden=True)      # off frame: empty rect
            add(6, rng.uniform(0, W, 6), rng.uniform(H + 30, H + 60, 6), 1.0, 1.0, 0.8, rng.uniform(1, 3, 6), hidden=True)
            add(6, -3.5, rng.uniform(2, H - 2, 6), 1.0, 1.0, 0.8, rng.uniform(1, 3, 6), hidden=True)                      # listed, below alpha_min everywhere
            add(6, rng.uniform(3, W - 3, 6), rng.uniform(3, H - 3, 6), 2.0, 2.0, 0.0035, rng.uniform(1, 3, 6), hidden=True)  # opacity below alpha_min
            add(8, rng.uniform(3, W - 3, 8), rng.uniform(3, H - 3, 8), 2.0, 2.0, 0.6, rng.uniform(1, 3, 8), hidden=True)     # culled by hand below
    p = np.concatenate(parts)
    zero = np.concatenate(zero)
    G = p.shape[0]
    rec = np.zeros((G, 12))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7] = p[:, 0], p[:, 1], p[:, 6], p[:, 5]
    rec[:, 4], rec[:, 5], rec[:, 6] = B._conic(p[:, 2], p[:, 3], p[:, 4])
    rect = B._rects(W, H, p[:, 0], p[:, 1], 3.33 * np.maximum(p[:, 2], p[:, 3]))
    if scene == "culled":
        rect[-8:] = 0
    if scene == "wall" and v == 1:
        zero[:] = False  # (the partial wall hides nothing for certain)
    return rec.astype(np.float32), rect, zero


@functools.lru_cache(maxsize=None)
def contrib_case(name):
    """a composite case of dense_raster_bwd64 / dense_raster_fwd64 (k2 and k3 kinds) or one of NEW_NAMES, with the same keys; the new ones
    add zero_rows [V,G]: rows every output of which must be exactly 0"""
    if name in OLD_NAMES:
        return F.fwd_comp_case(name)
    kind, key = name.split("_", 1)
    W, H, V, scene = NEW_CASES[key]
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    views = [_scene_view(kind, W, H, scene, rng, v) for v in range(V)]
    rec, rect, zero = (np.stack([vw[i] for vw in views]) for i in range(3))
    G = rec.shape[1]
    c2w = torch.eye(4, dtype=torch.float64)
    cams = [B.k2_cam(W, H, c2w) if kind == "k2" else B.k3_cam(W, H, c2w) for _ in range(V)]
    geo = RS.geometry_ref(W, H)
    live = (rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1]) != 0
    keys = np.where(live, rec[..., 2].view(np.uint32), np.uint32(RS.CULLED)).astype(np.uint32)
    sorted_ids = [s[1] for s in RS.sort_ref(keys)]
    bins = [RS.bin_ref(geo, sorted_ids[v], rect[v]) for v in range(V)]
    lists = [RS.tile_lists_ref(geo, *bins[v]) for v in range(V)]
    return dict(name=name, kind=kind, W=W, H=H, V=V, G=G, C=3, cams=cams, geo=geo, rec=rec, rect=rect, sorted_ids=sorted_ids, bins=bins, lists=lists,
                feats=None, scene=scene, walk_cache=[{} for _ in range(V)], zero_rows=zero)


# ---- float64 windows ---------------------------------------------------------------------------------------------------------------------
def contrib_ref(c):
    """per view: dict of count_lo, count_hi (int64 [G]), wmax_lo, wmax_hi, wsum_ref, wsum_tol (float64 [G]) and the margin map; cached on the case"""
    if "contrib_ref" in c:
        return c["contrib_ref"]
    out = []
    for v, r in enumerate(F.comp_fwd_ref(c)):
        cam, G = c["cams"][v], c["G"]
        ts, ids_all = np.asarray(c["lists"][v][0], np.int64), np.asarray(c["lists"][v][1], np.int64)
        lo, und = np.zeros(G, np.int64), np.zeros(G, np.int64)
        m_lo, m_hi, s_ref, s_tol = (np.zeros(G) for _ in range(4))
        for tile, w in r["walks"].items():
            ids = ids_all[ts[tile]:ts[tile + 1]]
            px, py, inside, _ = B._tile_pixels(cam, tile, c["kind"] != "k2")
            margin = np.full(px.shape[0], np.inf)
            margin[inside] = r["margin"][py[inside], px[inside]]
            decided = (margin >= MARGIN) & inside
            undecided = ~decided & inside
            M, e_a, _, e_Tb, _ = B._chain_errors(w)
            bl = w["bl"]
            a_min = np.float32(cam.alpha_min)
            with np.errstate(divide="ignore", invalid="ignore"):
                m_sig = np.where(M > 0, np.abs(w["sigma"]) / (6 * U24 * M), np.inf)
                m_min = np.abs(w["a"] - a_min) / (a_min * e_a)
            never = ((w["sigma"] < 0) & (m_sig >= MARGIN)) | ((w["sigma"] >= 0) & (w["a"] < a_min) & (m_min >= MARGIN))
            wt = w["a"] * w["Tb"]
            e_w = e_a + e_Tb + U24
            sure = bl & decided[None]
            maybe = w["reached"] & undecided[None] & ~never
            np.add.at(lo, ids, sure.sum(1))
            np.add.at(und, ids, maybe.sum(1))
            np.maximum.at(m_lo, ids, np.where(sure, wt * (1.0 - e_w), 0.0).max(1, initial=0.0))
            np.maximum.at(m_hi, ids, np.where(sure | maybe, wt * (1.0 + e_w), 0.0).max(1, initial=0.0))
            np.add.at(s_ref, ids, np.where(bl, wt, 0.0).sum(1))
            np.add.at(s_tol, ids, np.where(bl, wt * e_w, 0.0).sum(1) + np.where(maybe, wt, 0.0).sum(1))
        out.append(dict(count_lo=lo, count_hi=lo + und, wmax_lo=m_lo, wmax_hi=m_hi, wsum_ref=s_ref, wsum_tol=s_tol + (lo + und) * UNIT, margin=r["margin"]))
    c["contrib_ref"] = out
    return out


def check_contrib(name, c, wmax, count, wsum, check_share=True):
    """wmax [V,G] f32, count [V,G], wsum [V,G] int (numpy) against the windows of contrib_ref -> the worst position inside a window (<= 1)"""
    worst = 0.0
    for v, r in enumerate(contrib_ref(c)):
        if check_share:
            share = 1.0 - (r["margin"] >= MARGIN).mean()
            assert share <= ZERO_SHARE_CAP, f"{name} view {v}: {share:.4f} of the pixels lie below the margin"
        n = np.asarray(count[v], np.int64)
        lo, hi = r["count_lo"], r["count_hi"]
        bad = np.flatnonzero((n < lo) | (n > hi))
        assert bad.size == 0, f"{name} view {v}: count of {bad[:8]}: {n[bad[:8]]} outside [{lo[bad[:8]]}, {hi[bad[:8]]}]"
        big = lo > 200
        assert ((hi - lo)[big] < 0.02 * lo[big]).all(), f"{name} view {v}: a count window is too wide to check anything"
        m = np.asarray(wmax[v], np.float64)
        assert not np.isnan(m).any(), f"{name} view {v}: NaN wmax"
        bad = np.flatnonzero((m < r["wmax_lo"]) | (m > r["wmax_hi"]))
        assert bad.size == 0, f"{name} view {v}: wmax of {bad[:8]}: {m[bad[:8]]} outside [{r['wmax_lo'][bad[:8]]}, {r['wmax_hi'][bad[:8]]}]"
        s = np.asarray(wsum[v], np.float64) * UNIT
        d = np.abs(s - r["wsum_ref"])
        bad = np.flatnonzero(d > r["wsum_tol"])
        assert bad.size == 0, f"{name} view {v}: wsum of {bad[:8]}: {s[bad[:8]]} against {r['wsum_ref'][bad[:8]]} +- {r['wsum_tol'][bad[:8]]}"
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(r["wsum_tol"] > 0, d / r["wsum_tol"], 0.0), initial=0.0)))
        if "zero_rows" in c:
            z = c["zero_rows"][v]
            assert (m[z] == 0).all() and (n[z] == 0).all() and (np.asarray(wsum[v])[z] == 0).all(), f"{name} view {v}: a row that blends nowhere is not exactly 0"
    return worst


# ---- float32 emulation (and the wrong answers) ---------------------------------------------------------------------------------------------
MUTATIONS = ("post_blend_T", "no_alpha_max", "count_saturating", "alpha_only", "no_tile_merge", "no_half")


def contrib_emul32(c, mutate=None):
    """the statistics in the kernel's definitions from B._walk(f32=True), the kernel's own decisions -> wmax [V,G] f32, count, wsum [V,G] int64.
    mutate: one of MUTATIONS, a wrong answer"""
    k3 = c["kind"] != "k2"
    V, G = c["V"], c["G"]
    wmax, count, wsum = np.zeros((V, G), F32), np.zeros((V, G), np.int64), np.zeros((V, G), np.int64)
    for v in range(V):
        cam = c["cams"][v]
        if mutate == "no_alpha_max":
            cam = copy.copy(cam)
            cam.alpha_max = 1e30
        rec32 = np.asarray(c["rec"][v], F32)
        ts, ids_all = np.asarray(c["lists"][v][0], np.int64), np.asarray(c["lists"][v][1], np.int64)
        for tile in range(ts.shape[0] - 1):
            ids = ids_all[ts[tile]:ts[tile + 1]]
            if ids.shape[0] == 0:
                continue
            px, py, inside, off = B._tile_pixels(cam, tile, k3)
            if mutate == "no_half" and k3:
                off = 0.0
            w = B._walk(cam, rec32[ids], px, py, inside, off, k3, True)
            bl, a = w["bl"], w["a"].astype(F32)
            Tq = (w["nT"] if mutate == "post_blend_T" else w["Tb"]).astype(F32)
            if mutate == "count_saturating":
                bl = bl | (w["reached"] & w["static"])  # (reached and static but not blended: the saturating entry)
            wt = a if mutate == "alpha_only" else (a * Tq).astype(F32)
            wt = np.where(bl, wt, F32(0.0)).astype(F32)
            tmax = wt.max(1)
            if mutate == "no_tile_merge":
                has = bl.any(1)
                wmax[v][ids[has]] = tmax[has]  # a plain store: the last tile wins
            else:
                np.maximum.at(wmax[v], ids, tmax)
            np.add.at(count[v], ids, bl.sum(1))
            np.add.at(wsum[v], ids, np.floor(wt.astype(np.float64) * 2.0 ** 40).astype(np.int64).sum(1))
    return wmax, count, wsum
