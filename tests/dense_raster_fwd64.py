"""Float64 references, bounds and crafted cases of the rasterizer's FORWARD stages that produce floating-point numbers
(siu3r_amd/csrc/raster.hip: project_kernel with cam_pose_kernel / cam_pose_c2w_kernel, composite_rgb_kernel, composite_feat_kernel,
composite_feat5_kernel), written from include/siu3r_hip.h and the kernels' comments; shared by tests/test_raster_fwd_stages_ref.py (CPU)
and tests/test_raster_fwd_stages_gpu.py (GPU).  The float64 projection (project64), the pixel walk (_walk), the chain errors
(_chain_errors) and the decision margin are those of tests/dense_raster_bwd64.py (imported, not copied); this file adds the forward's
own bounds, its integer outputs, the forward-only cases and a float32 emulation of every stage in the kernels' expression order.

SCALES.  As in dense_raster_bwd64: every reference value carries S, the sum of the absolute values of the terms it is a sum of.
  mean (mx, my)   the pinhole form m = f x / z + c of either mode (mode 0: f = W / (2 tanfovx), c = (W - 1) / 2): the error of x / z is
                  that of the camera-space point, k_pt per unit, once for x and |x / z| times for z: S = f (1 + |x / z|) k_pt + |c|.
                  (The plain |mx| is 0 on the frame's left edge and is no scale of anything.)
  depth           |z| k_pt
  conic a, c      |value| k_pt k_cov k_det (the three conditions of project64, as the backward weights its conic slots)
  conic b         sqrt(a c) k_pt k_cov k_det: the off-diagonal c01 = t0 Sigma t1 may cancel to nothing while its terms are of the size
                  sqrt(c00 c11) (Cauchy-Schwarz), so |b| itself is no scale
  colour          sh_basis_abs . |coefficients| + 0.5 (SH); precomputed and mode-1 record colours are copies: bit-equal
  opacity         a copy: bit-equal

BOUNDS (u = 2^-24, one fp32 rounding; device reciprocal and sqrtf 1 ulp = 2 u).
  PROJ_FWD_BOUND = 74 u.  Longest path, mean -> conic: the camera-space point 6, x / z 1, (clamp 0,) c x z 1, the Jacobian entry
      -(f c) rz rz 3, M = J W 3, Sigma M^T 5, c00 6, det 3, the conic's product with 1 / det 1, f = W / (2 tan) 2: 31 roundings; every
      sum's other inputs are of the same depth, counted once more: 62.  Reciprocals: 1 / z enters the Jacobian entry twice and x / z
      once, 1 / det once, the division in f once: 5 uses of 2 u, + 2 u for lim = 1.3 tan and the blur add.  (PROJ_BOUND of the backward,
      164 u, is this path AGAIN plus 48 backward roundings and eleven more reciprocal uses; it is not reused here.)
  PROJ_MEAN_BOUND = 26 u.  mode 0: the homogeneous row 6, hw + 1e-7 1, h pw 1, + 1, x W, - 1: 3 (x 0.5 is exact), the reciprocal 2 u:
      11 + 2, doubled for the fan-in; mode 1: point 6, x rz 1, f x 1, + c 1, 2 u: 9 + 2, doubled.  Depth is the point's third row: 6.
  SH_FWD_BOUND = 80 u.  direction: m - campos 1, d . d 5, sqrtf 2 u, reciprocal 2 u, d inv 1: 11 u on each of x, y, z; a band-4 monomial
      is of degree 4 in them: 44 u; the monomial's own products and differences 6, constant and coefficient 2, the 25-term sum and + 0.5: 26.
      78, rounded up to 80.
  POSE (cam_pose_c2w_kernel): the kernel evaluates in float64 and rounds once, so |got - ref| <= half an fp32 ulp of the value + the
      float64 evaluation error.  Adjugate inverse: a cofactor is a sum of six triple products (2 roundings each, 5 adds), det four more
      products and 3 adds, the division 1: |err(W_ij)| <= 12 u64 (A_ij + |W_ij| D) / |det|, A_ij = the cofactor's absolute terms, D =
      det's absolute terms (pose_inverse_error).  For a rigid pose with |t| <= 10: below 1e-13, eight orders below an fp32 ulp of an
      entry of size 1 (6e-8), so the effective check is "the correctly rounded value or its neighbour".  The fov / tan / projection
      chain (about 60 float64 operations, acos and tan at <= 1 ulp64, conditioned by 1 / sin(fov) <= 3 for the lenses used): 400 u64.
  COMPOSITE MAPS.  For a pixel with blended entries j, weight w_j = a_j T_j and value f_j (colour / feature channel, depth, 1 for alpha):
        |got - ref| <= sum_j |f_j| w_j (e_w(j) + K_FWD u) + |bg| T_final (e_T_final + u)
      e_w = e_a + e_T in front of j (dense_raster_bwd64._chain_errors).  k = K_FWD + n_behind(j), K_FWD = 2: the product a T (1) and the
      entry's own fused multiply-add (1; alpha is a plain add: 1), plus one per entry the pixel blends BEHIND j: every later fused
      multiply-add rounds the running sum, which contains term j (recursive summation: term j passes n - j + 1 roundings).  A constant k
      of 2 or 3 holds for the last entries of a pixel only: the float32 emulation of the kernels' own chain exceeds it (up to 1.26 x with
      k = 3, signed feature rows behind a heavy first entry: tests/test_raster_fwd_stages_ref.py reports the ratios), so the count is kept
      as derived.  The
      background term is one fused multiply-add: u, and T's own e_T.  The matrix-core form promises the same fmaf chain: same bound.
      A pixel that blends nothing has tolerance 0: the background bit for bit (K2), exactly 0 (K3, feat, depth, alpha).
  N_TOUCHED.  T (pre-blend) or T' (post-blend) > 0.5 is one more threshold: m_nt = |T - 0.5| / (0.5 (e_T + step)) joins the margin
      of the pixel, and got[g] must lie in [count over decided pixels, that + undecided pixels that reach g].

INTEGER OUTPUTS of the projection (radii, rect, tiles_touched, keys, stats) are computed from the float64 record.  A row is DECIDED when
every compared or rounded quantity lies farther than MARGIN (4) derived errors from its threshold (depth cull, det, radius_clip, off
frame, alpha_min of the opacity-aware extent; ceilf of the radius, the four rect edges).  Errors: PROJ_FWD_BOUND S for c00, c11, det;
PROJ_MEAN_BOUND S for mx, my, tz; the radius through sqrt: half the relative error + 2 u, the K2 eigenvalue through sqrt(max(0.1, mid^2
- det)) with its cancellation (mid^2 + det) 3 u + the inputs' errors, divided by 2 sqrt(.); logf <= 2 u |L| + u of the quotient.
After the clamp to [0, gw] truncation and floor agree on the lower edges ((int) of (-1, 0) is 0, floor is -1, clamped to 0): only the
upper edges tell K2 (trunc((x + 15) / 16)) from K3 (ceil(x / 16)), for x in (16 k, 16 k + 1).  The key clamp below 0xffffffff cannot be
reached by a valid row: a positive float's bit pattern is below 0x7f800001 and a NaN depth leaves rect empty ((int)NaN = 0), so its
only check is that culled rows, and only they, carry 0xffffffff.

Not a test module."""
import copy
import functools
import math

import numpy as np
import torch

import dense_raster64 as DR
import dense_raster_bwd64 as B
import raster_stages_ref as RS

U24 = B.U24
U53 = 2.0 ** -53
PROJ_FWD_BOUND = 74 * U24
PROJ_MEAN_BOUND = 26 * U24
SH_FWD_BOUND = 80 * U24
K_FWD = 2
MARGIN = B.MARGIN
ZERO_SHARE_CAP = B.ZERO_SHARE_CAP
TILE = B.TILE
DD = torch.float64
F32 = np.float32
STG, STG_PULL, FK = 512, 192, 4  # composite_rgb_kernel's staging constants (restated by refill_rounds)
CULLED = np.uint32(RS.CULLED)


# ---- projection: the float64 record, its scales, the integer outputs ---------------------------------------------------------------------
def proj_record64(mode, cam, means, cov6, opac, colors):
    """-> rec [G,10] (numpy float64, B's slot order), S [G,10], bound [10], aux.  colors as project64 takes them."""
    with torch.no_grad():
        rec, aux = B.project64(mode, cam, means, cov6, opac, colors)
    rec = rec.numpy()
    G = rec.shape[0]
    fx, fy, _, _ = B.lens_limits(mode, cam)
    cx, cy = ((cam.width - 1) / 2.0, (cam.height - 1) / 2.0) if mode == 0 else (cam.cx, cam.cy)
    k_pt, kc = aux["k_pt"].numpy(), (aux["k_pt"] * aux["k_cov"] * aux["k_det"]).numpy()
    S = np.zeros((G, 10))
    S[:, B.MX] = fx * (1.0 + np.abs(aux["txz"].numpy())) * k_pt + abs(cx)
    S[:, B.MY] = fy * (1.0 + np.abs(aux["tyz"].numpy())) * k_pt + abs(cy)
    S[:, B.ZZ] = np.abs(rec[:, B.ZZ]) * k_pt
    for k in (B.CA, B.CC):
        S[:, k] = np.abs(rec[:, k]) * kc
    S[:, B.CB] = np.sqrt(np.abs(rec[:, B.CA] * rec[:, B.CC])) * kc  # (c01 is a sum that may cancel to nothing: the scale of its terms is sqrt(c00 c11))
    bound = np.full(10, PROJ_FWD_BOUND)
    bound[[B.MX, B.MY, B.ZZ]] = PROJ_MEAN_BOUND
    bound[B.OP] = 0.0
    if mode == 0 and cam.sh_degree >= 0:
        m = means.to(DD)
        d = m - torch.tensor(list(cam.campos), dtype=DD)
        d = d / d.norm(dim=-1, keepdim=True)
        Ba = B.sh_basis_abs(d, cam.sh_degree, bool(cam.sh_band4))
        S[:, B.RR:B.BB + 1] = ((Ba[:, :, None] * colors.to(DD)[:, :Ba.shape[1], :].abs()).sum(1) + 0.5).numpy()
        bound[B.RR:B.BB + 1] = SH_FWD_BOUND
    else:
        bound[B.RR:B.BB + 1] = 0.0  # copies
    return rec, S, bound, aux


def _edge_decided(q, e, lo, hi):
    """q: the float an edge is rounded from, thresholds at the integers lo .. hi (outside them the clamp decides) -> decided"""
    near = np.clip(np.rint(q), lo, hi)
    return np.abs(q - near) > MARGIN * e


def proj_int64(mode, cam, rec, S, aux, opac, exact_depth=False, mutate=None):
    """the integer outputs of one view from the float64 record -> dict valid, radii [G,2], rect [G,4], tiles [G], decided [G], why [G]
    (the cull that removed the row: 0 none, 1 depth, 2 det, 3 alpha_min, 4 radius_clip, 5 off frame, 6 empty rect)"""
    mutate = mutate or {}
    W, H = cam.width, cam.height
    gw, gh = -(-W // TILE), -(-H // TILE)
    G = rec.shape[0]
    with np.errstate(all="ignore"):
        tz, mx, my = rec[:, B.ZZ], rec[:, B.MX], rec[:, B.MY]
        det = aux["det"].numpy()
        c00, c11, c01 = rec[:, B.CC] * det, rec[:, B.CA] * det, -rec[:, B.CB] * det
        kc = (aux["k_pt"] * aux["k_cov"]).numpy()
        e_tz = np.zeros(G) if exact_depth else PROJ_MEAN_BOUND * S[:, B.ZZ]
        e_mx, e_my = PROJ_MEAN_BOUND * S[:, B.MX], PROJ_MEAN_BOUND * S[:, B.MY]
        e00, e11 = PROJ_FWD_BOUND * c00 * kc, PROJ_FWD_BOUND * c11 * kc
        e_det = PROJ_FWD_BOUND * (c00 * c11 + c01 * c01) * kc
        why = np.zeros(G, np.int32)
        decided = np.ones(G, bool)
        op = np.asarray(opac, np.float64)

        def cull(cond, code, dist=None, err=None):
            nonlocal why, decided
            live = why == 0
            if dist is not None:
                decided &= ~live | (np.abs(dist) > MARGIN * err) | (err == 0)  # (err 0: an exact row, the comparison has no margin)
            why = np.where(live & cond, code, why)

        if mode == 0:
            thr = float(F32(cam.k2_znear_cull))
            cull((tz < thr) if mutate.get("znear_lt") else (tz <= thr), 1, tz - thr, e_tz)
            cull(det == 0, 2, det, e_det)
            mid = 0.5 * (c00 + c11)
            dd = mid * mid - det
            e_dd = 2 * mid * 0.5 * (e00 + e11) + e_det + 3 * U24 * (mid * mid + np.abs(det))
            sq = np.sqrt(np.maximum(0.1, dd))
            lam = mid + sq
            e_lam = 0.5 * (e00 + e11) + np.where(dd > 0.1 - MARGIN * e_dd, e_dd / (2 * sq), 0.0) + 3 * U24 * lam
            x = 3.0 * np.sqrt(lam)
            e_x = x * (0.5 * e_lam / lam + 3 * U24)
            rad = np.ceil(x)
            rad_ok = np.abs(x - np.rint(x)) > MARGIN * e_x
            # (a row off the frame with either neighbouring radius has radii 0 and an empty rect whichever the kernel rounds to)
            empty = lambda r_: (np.clip(np.trunc((mx + r_ + TILE - 1) / TILE), 0, gw) - np.clip(np.trunc((mx - r_) / TILE), 0, gw)) * \
                (np.clip(np.trunc((my + r_ + TILE - 1) / TILE), 0, gh) - np.clip(np.trunc((my - r_) / TILE), 0, gh)) == 0
            far_off = ((mx + rad + 2 + TILE < 0) | (mx - rad - 2 > gw * TILE + TILE) | (my + rad + 2 + TILE < 0) | (my - rad - 2 > gh * TILE + TILE)) & empty(rad - 1) & empty(rad + 1)
            decided &= (why != 0) | rad_ok | far_off
            rx = ry = rad
            q = [(mx - rad) / TILE, (my - rad) / TILE, (mx + rad + TILE - 1) / TILE, (my + rad + TILE - 1) / TILE]
            if mutate.get("k2_upper_ceil"):
                q[2], q[3] = np.ceil((mx + rad) / TILE), np.ceil((my + rad) / TILE)
            edges = [np.clip(np.trunc(v), 0, g_) for v, g_ in zip(q, (gw, gh, gw, gh))]
            lo_thr = (1, 1, 1, 1)
            hi_thr = (gw, gh, gw, gh)
        else:
            near, far = float(F32(cam.near_plane)), float(F32(cam.far_plane))
            cull(tz < near, 1, tz - near, e_tz)
            cull(tz > far, 1, tz - far, e_tz)
            cull(det <= 0, 2, det, e_det)
            ext = np.full(G, float(F32(cam.extent_sigma)))
            e_ext = np.zeros(G)
            if cam.opacity_aware_extent:
                amin = float(F32(cam.alpha_min))
                cull(op < amin, 3)  # (opacity and alpha_min are inputs: the comparison is exact)
                L = np.log(np.maximum(op / amin, 1e-300))
                lext = np.sqrt(2.0 * np.maximum(L, 0.0))
                e_lext = np.where(lext > 0, (U24 + 2 * U24 * np.abs(L) + 2 * U24 * np.abs(L)) / np.maximum(lext, 1e-300) + 2 * U24 * lext, 0.0)
                if not mutate.get("oae_no_min"):
                    decided &= (why != 0) | (np.abs(lext - ext) > MARGIN * e_lext)
                    e_ext = np.where(lext < ext, e_lext, 0.0)
                    ext = np.minimum(ext, lext)
                else:
                    ext, e_ext = lext, e_lext
            xs, ys = ext * np.sqrt(c00), ext * np.sqrt(c11)
            e_xs = xs * (0.5 * e00 / c00 + 3 * U24) + e_ext * np.sqrt(c00)
            e_ys = ys * (0.5 * e11 / c11 + 3 * U24) + e_ext * np.sqrt(c11)
            rx, ry = np.ceil(xs), np.ceil(ys)
            decided &= (why != 0) | ((np.abs(xs - np.rint(xs)) > MARGIN * e_xs) & (np.abs(ys - np.rint(ys)) > MARGIN * e_ys)) | ((xs == 0) & (ys == 0))
            clip = float(F32(cam.radius_clip))
            cull((rx < clip) & (ry < clip) if mutate.get("clip_lt") else (rx <= clip) & (ry <= clip), 4)  # (integers against the input: exact)
            cull(mx + rx <= 0, 5, mx + rx, e_mx)
            cull(mx - rx >= W, 5, mx - rx - W, e_mx)
            cull(my + ry <= 0, 5, my + ry, e_my)
            cull(my - ry >= H, 5, my - ry - H, e_my)
            q = [(mx - rx) / TILE, (my - ry) / TILE, (mx + rx) / TILE, (my + ry) / TILE]
            if mutate.get("k3_upper_trunc"):
                edges = [np.clip(np.floor(q[0]), 0, gw), np.clip(np.floor(q[1]), 0, gh), np.clip(np.trunc(q[2] + (TILE - 1) / TILE), 0, gw),
                         np.clip(np.trunc(q[3] + (TILE - 1) / TILE), 0, gh)]
            else:
                edges = [np.clip(np.floor(q[0]), 0, gw), np.clip(np.floor(q[1]), 0, gh), np.clip(np.ceil(q[2]), 0, gw), np.clip(np.ceil(q[3]), 0, gh)]
            lo_thr = (1, 1, 0, 0)
            hi_thr = (gw, gh, gw - 1, gh - 1)
        for i, (v, e) in enumerate(zip(q, (e_mx, e_my, e_mx, e_my))):
            decided &= (why != 0) | _edge_decided(v, (e + 2 * U24 * np.abs(v) * TILE) / TILE, lo_thr[i], hi_thr[i])
        rect = np.stack([np.nan_to_num(e_) for e_ in edges], -1).astype(np.int64)
        area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        why = np.where((why == 0) & (area == 0), 6, why)
        bad = ~np.isfinite(tz) | ~np.isfinite(det)  # a NaN mean or an Inf covariance takes no part
        why = np.where(bad & (why == 0), 2, why)
        decided |= bad
        valid = why == 0
        rect[~valid] = 0
        radii = np.stack([np.nan_to_num(rx), np.nan_to_num(ry)], -1).astype(np.int64)
        if mode == 0:
            radii[~valid] = 0
        else:
            radii[np.isin(why, (1, 2, 3, 4, 5))] = 0  # (mode 1 writes its radii in front of the empty-rect test)
    return dict(valid=valid, radii=radii, rect=rect, tiles=np.where(valid, area, 0), decided=decided, why=why)


# ---- projection: float32 emulation in the kernel's expression order -----------------------------------------------------------------------
def _f(x):
    return np.asarray(x, F32)


def _sh32(x, y, z, sh, deg, band4, mutate):
    """sh [G, 25, 3] float32 (zeros past the loaded block) -> col [G,3], the kernel's polynomial term by term"""
    C0, C1 = F32(DR.SH_C0), F32(DR.SH_C1)
    c2, c3, c4 = [F32(c) for c in DR.SH_C2], [F32(c) for c in DR.SH_C3], [F32(c) for c in DR.SH_C4]
    if mutate.get("sh_sign") is not None:
        k = mutate["sh_sign"]
        if k == 1:
            C1 = -C1
        elif k == 2:
            c2[2] = -c2[2]
        elif k == 3:
            c3[3] = -c3[3]
        else:
            c4[4] = -c4[4]
    out = []
    for ch in range(3):
        S = lambda i: sh[:, i, ch]
        r = C0 * S(0)
        if deg > 0:
            r = r - C1 * y * S(1) + C1 * z * S(2) - C1 * x * S(3)
            if deg > 1:
                xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
                r = r + c2[0] * xy * S(4) + c2[1] * yz * S(5) + c2[2] * (F32(2) * zz - xx - yy) * S(6) + c2[3] * xz * S(7) + c2[4] * (xx - yy) * S(8)
                if deg > 2:
                    r = (r + c3[0] * y * (F32(3) * xx - yy) * S(9) + c3[1] * xy * z * S(10) + c3[2] * y * (F32(4) * zz - xx - yy) * S(11) +
                         c3[3] * z * (F32(2) * zz - F32(3) * xx - F32(3) * yy) * S(12) + c3[4] * x * (F32(4) * zz - xx - yy) * S(13) +
                         c3[5] * z * (xx - yy) * S(14) + c3[6] * x * (xx - F32(3) * yy) * S(15))
                    if deg > 3 and band4:
                        r = (r + c4[0] * xy * (xx - yy) * S(16) + c4[1] * yz * (F32(3) * xx - yy) * S(17) + c4[2] * xy * (F32(7) * zz - F32(1)) * S(18) +
                             c4[3] * yz * (F32(7) * zz - F32(3)) * S(19) + c4[4] * (zz * (F32(35) * zz - F32(30)) + F32(3)) * S(20) +
                             c4[5] * xz * (F32(7) * zz - F32(3)) * S(21) + c4[6] * (xx - yy) * (F32(7) * zz - F32(1)) * S(22) +
                             c4[7] * xz * (xx - F32(3) * yy) * S(23) + c4[8] * (xx * (xx - F32(3) * yy) - yy * (F32(3) * xx - yy)) * S(24))
        r = r + F32(0.5)
        out.append(np.where(r < 0, F32(0), r))
    return np.stack(out, -1)


def project_emul32(mode, cam, means, cov6, opac, colors, planar=False, nf_loaded=None, k3_channels=3, mutate=None):
    """project_kernel for one view in numpy float32, operation for operation.  colors: mode 0 [G,n,3] interleaved values (the planar
    layout holds the same values: `planar` only matters to the mutation that reads it wrongly); nf_loaded: the floats of the SH block
    in registers (None: what this view needs).  -> rec [G,12] (slot 11 NaN where rp[2] is not written, all of a culled row's rp[2]
    NaN), radii, rect, tiles, keys (uint32), valid"""
    mutate = mutate or {}
    with np.errstate(all="ignore"):
        m, S6, op = _f(means), _f(cov6), _f(opac)
        G = m.shape[0]
        V = _f(list(cam.w2c))
        W, H = cam.width, cam.height
        gw, gh = -(-W // TILE), -(-H // TILE)
        tx = V[0] * m[:, 0] + V[1] * m[:, 1] + V[2] * m[:, 2] + V[3]
        ty = V[4] * m[:, 0] + V[5] * m[:, 1] + V[6] * m[:, 2] + V[7]
        tz = V[8] * m[:, 0] + V[9] * m[:, 1] + V[10] * m[:, 2] + V[11]
        alive = np.ones(G, bool)
        if mode == 0:
            cullz = F32(cam.k2_znear_cull)
            alive &= ~((tz < cullz) if mutate.get("znear_lt") else (tz <= cullz))
            tanx, tany = F32(cam.tanfovx), F32(cam.tanfovy)
            fx, fy = F32(W) / (F32(2) * tanx), F32(H) / (F32(2) * tany)
            lxp = lxn = F32(1.3) * tanx
            lyp = lyn = F32(1.3) * tany
            blur = F32(cam.dilation)
        else:
            alive &= ~((tz < F32(cam.near_plane)) | (tz > F32(cam.far_plane)))
            fx, fy, cx, cy = F32(cam.fx), F32(cam.fy), F32(cam.cx), F32(cam.cy)
            tfx, tfy = F32(0.5) * F32(W) / fx, F32(0.5) * F32(H) / fy
            lxp, lxn = (F32(W) - cx) / fx + F32(0.3) * tfx, cx / fx + F32(0.3) * tfx
            lyp, lyn = (F32(H) - cy) / fy + F32(0.3) * tfy, cy / fy + F32(0.3) * tfy
            blur = F32(cam.eps2d)
        if mutate.get("swap_lim"):
            lxp, lxn, lyp, lyn = lyp, lyn, lxp, lxn
        rz = F32(1) / tz
        txz, tyz = tx * rz, ty * rz
        cxz, cyz = np.minimum(lxp, np.maximum(-lxn, txz)), np.minimum(lyp, np.maximum(-lyn, tyz))
        ctx, cty = cxz * tz, cyz * tz
        j00, j02, j11, j12 = fx * rz, -(fx * ctx) * rz * rz, fy * rz, -(fy * cty) * rz * rz
        t0 = [j00 * V[i] + j02 * V[8 + i] for i in range(3)]
        t1 = [j11 * V[4 + i] + j12 * V[8 + i] for i in range(3)]
        S = [S6[:, i] for i in range(6)]
        a = [t0[0] * S[0] + t0[1] * S[1] + t0[2] * S[2], t0[0] * S[1] + t0[1] * S[3] + t0[2] * S[4], t0[0] * S[2] + t0[1] * S[4] + t0[2] * S[5]]
        b = [t1[0] * S[0] + t1[1] * S[1] + t1[2] * S[2], t1[0] * S[1] + t1[1] * S[3] + t1[2] * S[4], t1[0] * S[2] + t1[1] * S[4] + t1[2] * S[5]]
        c00 = a[0] * t0[0] + a[1] * t0[1] + a[2] * t0[2] + blur
        c01 = a[0] * t1[0] + a[1] * t1[1] + a[2] * t1[2]
        c11 = b[0] * t1[0] + b[1] * t1[1] + b[2] * t1[2] + blur
        det = c00 * c11 - c01 * c01
        alive &= ~((det == 0) if mode == 0 else (det <= 0))
        if not mutate.get("nonfinite_valid"):
            alive &= np.isfinite(det)  # (a NaN mean or an Inf covariance takes no part)
        det_inv = F32(1) / det
        ca, cb, cc = c11 * det_inv, -c01 * det_inv, c00 * det_inv
        toi = lambda v: np.nan_to_num(np.clip(np.where(np.isnan(v), 0, v), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
        if mode == 0:
            P = _f(list(cam.proj))
            hx = P[0] * m[:, 0] + P[1] * m[:, 1] + P[2] * m[:, 2] + P[3]
            hy = P[4] * m[:, 0] + P[5] * m[:, 1] + P[6] * m[:, 2] + P[7]
            hw = P[12] * m[:, 0] + P[13] * m[:, 1] + P[14] * m[:, 2] + P[15]
            pw = F32(1) / (hw + F32(0.0000001))
            mx = ((hx * pw + F32(1)) * F32(W) - F32(1)) * F32(0.5)
            my = ((hy * pw + F32(1)) * F32(H) - F32(1)) * F32(0.5)
            mid = F32(0.5) * (c00 + c11)
            lam = mid + np.sqrt(np.fmax(F32(0.1), mid * mid - det))
            lam2 = mid - np.sqrt(np.fmax(F32(0.1), mid * mid - det))
            rad = toi(np.ceil(F32(3) * np.sqrt(np.fmax(lam, lam2))))
            radf = rad.astype(F32)
            rxi = ryi = rad
            if mutate.get("k2_upper_ceil"):
                up = [toi(np.ceil((mx + radf) / F32(TILE))), toi(np.ceil((my + radf) / F32(TILE)))]
            else:
                up = [toi(np.trunc((mx + radf + F32(TILE - 1)) / F32(TILE))), toi(np.trunc((my + radf + F32(TILE - 1)) / F32(TILE)))]
            e4 = [np.clip(toi(np.trunc((mx - radf) / F32(TILE))), 0, gw), np.clip(toi(np.trunc((my - radf) / F32(TILE))), 0, gh), np.clip(up[0], 0, gw),
                  np.clip(up[1], 0, gh)]
        else:
            mx, my = fx * txz + cx, fy * tyz + cy
            ext = np.full(G, F32(cam.extent_sigma))
            if cam.opacity_aware_extent:
                amin = F32(cam.alpha_min)
                alive &= ~(op < amin)
                lext = np.sqrt(F32(2) * np.log(op / amin).astype(F32)).astype(F32)
                ext = lext if mutate.get("oae_no_min") else np.fmin(ext, lext)
            rx, ry = np.ceil(ext * np.sqrt(c00)), np.ceil(ext * np.sqrt(c11))
            clip = F32(cam.radius_clip)
            alive &= ~(((rx < clip) & (ry < clip)) if mutate.get("clip_lt") else ((rx <= clip) & (ry <= clip)))
            alive &= ~((mx + rx <= 0) | (mx - rx >= F32(W)) | (my + ry <= 0) | (my - ry >= F32(H)))
            rxi, ryi = toi(rx), toi(ry)
            if mutate.get("k3_upper_trunc"):
                up = [toi(np.trunc((mx + rx + F32(TILE - 1)) / F32(TILE))), toi(np.trunc((my + ry + F32(TILE - 1)) / F32(TILE)))]
            else:
                up = [toi(np.ceil((mx + rx) / F32(TILE))), toi(np.ceil((my + ry) / F32(TILE)))]
            e4 = [np.clip(toi(np.floor((mx - rx) / F32(TILE))), 0, gw), np.clip(toi(np.floor((my - ry) / F32(TILE))), 0, gh), np.clip(up[0], 0, gw),
                  np.clip(up[1], 0, gh)]
        rect = np.stack(e4, -1)
        area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        reached = alive.copy()  # rows that got as far as the rect
        valid = alive & (area != 0)
        rect[~valid] = 0
        radii = np.stack([rxi, ryi], -1)
        radii[~reached] = 0
        if mode == 0:
            radii[~valid] = 0
        rec = np.zeros((G, 12), F32)
        # rows that left at the depth cull keep mx = my = conic = 0; later culls have written what they had computed
        past_depth = ~((tz <= F32(cam.k2_znear_cull)) if mode == 0 else ((tz < F32(cam.near_plane)) | (tz > F32(cam.far_plane))))
        past_det = past_depth & ~((det == 0) if mode == 0 else (det <= 0)) & (np.isfinite(det) | bool(mutate.get("nonfinite_valid")))
        rec[:, 2], rec[:, 7] = tz, op
        for k, vv in ((4, ca), (5, cb), (6, cc)):
            rec[:, k] = np.where(past_det, vv, 0)
        rec[:, 0], rec[:, 1] = np.where(past_det, mx, 0), np.where(past_det, my, 0)
        rec[:, 8:12] = np.nan
        tzb = tz.view(np.uint32)
        keys = np.where(valid, tzb if mutate.get("key_unclamped") else np.minimum(tzb, np.uint32(0xFFFFFFFE)), CULLED).astype(np.uint32)
        if mode == 1:
            if colors is not None and k3_channels == 3:
                rec[valid, 8:11] = _f(colors)[valid]
                rec[valid, 11] = 0
        elif cam.sh_degree < 0:
            rec[valid, 8:11] = _f(colors).reshape(G, 3)[valid]
            rec[valid, 11] = 0
        else:
            cp = _f(list(cam.campos))
            dx, dy, dz = m[:, 0] - cp[0], m[:, 1] - cp[1], m[:, 2] - cp[2]
            inv = F32(1) / np.sqrt(dx * dx + dy * dy + dz * dz)
            deg, band4 = cam.sh_degree, bool(cam.sh_band4)
            ncf = 25 if (deg > 3 and band4) else (16 if deg > 2 else (9 if deg > 1 else (4 if deg > 0 else 1)))
            col = _f(colors)
            n = col.shape[1]
            flat = np.zeros((G, 76), F32)
            src = col.transpose(0, 2, 1).reshape(G, -1) if (planar and mutate.get("planar_as_interleaved")) else col.reshape(G, -1)
            nf = max(ncf * 3, nf_loaded or 0) if not mutate.get("sh_first_view_only") else (nf_loaded or ncf * 3)
            nf = min(4 * -(-nf // 4), 76)  # whole 16-byte loads
            k = min(nf, n * 3)
            flat[:, :k] = src[:, :k]
            sh = flat[:, :75].reshape(G, 25, 3)
            c3 = _sh32(dx * inv, dy * inv, dz * inv, sh, deg, band4, mutate)
            rec[valid, 8:11] = c3[valid]
            rec[valid, 11] = 0
    return dict(rec=rec, radii=radii, rect=rect, tiles=np.where(valid, area, 0), keys=keys, valid=valid)


# ---- projection cases ----------------------------------------------------------------------------------------------------------------------
def _flip(c2w):
    """the same camera centre, looking the other way (rotated by pi about its own y axis)"""
    c = c2w.clone()
    c[:3, 0], c[:3, 2] = -c2w[:3, 0], -c2w[:3, 2]
    return c


def _cloud(rng, c2w, G, lim, zlo=1.5, zhi=4.0, spread=0.95):
    xn, xp, yn, yp = lim
    tz = rng.uniform(zlo, zhi, G)
    u = rng.uniform(-spread, spread, (G, 2))
    pc = np.stack([np.where(u[:, 0] > 0, xp, xn) * u[:, 0] * tz, np.where(u[:, 1] > 0, yp, yn) * u[:, 1] * tz, tz, np.ones(G)], -1)
    return (torch.from_numpy(pc) @ c2w.T)[:, :3].float()


def _covs(rng, G, lo=0.05, hi=0.1):
    import dense_gsplat64 as DG

    return DG.quat_scale_to_cov6(torch.from_numpy(rng.normal(size=(G, 4))), torch.from_numpy(rng.uniform(lo, hi, (G, 3)))).float()


#                 mode  views (degree, band4) or V      G    channels planar stride  what
PROJ_FWD_NEW = {
    "k2_v16":     (0, 16, 257, 4, False, 6),
    "k2_v17":     (0, 17, 257, 4, False, 9),
    "k2_v33":     (0, 33, 257, 4, False, 6),
    "k2_mixed":   (0, 4, 300, 25, False, 6),
    "k2_mixed_planar": (0, 4, 300, 25, True, 6),
    "k2_ch4":     (0, 1, 257, 4, False, 6),
    "k2_ch9":     (0, 1, 257, 9, False, 6),
    "k2_edges":   (0, 1, 320, 1, False, 6),
    "k2_depth":   (0, 1, 12, 1, False, 6),
    "k2_nonfinite": (0, 1, 66, 1, False, 6),
    "k3_oae":     (1, 2, 300, 3, False, 6),
    "k3_clip":    (1, 1, 90, 3, False, 6),
    "k3_edges":   (1, 1, 320, 3, False, 9),
    "k3_depth":   (1, 1, 24, 3, False, 6),
    "k3_nonfinite": (1, 1, 66, 3, False, 6),
    "k3_nocolor": (1, 1, 64, 0, False, 6),
    "k3_c5":      (1, 1, 64, 5, False, 6),
}
PROJ_FWD_CASES = list(B.PROJ_CASES) + list(PROJ_FWD_NEW)
MIXED_DEGREES = ((0, False), (3, False), (1, False), (4, True))


def _ulps(x, k):
    v = F32(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
    return float(v)


@functools.lru_cache(maxsize=None)
def proj_fwd_case(name):
    """-> dict mode, V, G, cams, means, cov6, opac, colors (interleaved values; mode 1: [G,channels] or None), channels, planar, stride,
    exact_depth (identity pose: tz is the mean's z bit for bit)"""
    if name in B.PROJ_CASES:
        c = B.proj_case(name)
        d = dict(name=name, mode=c["mode"], V=c["V"], G=c["G"], cams=c["cams"], means=c["means"], cov6=c["cov6"], opac=c["opac"], colors=c["colors"],
                 planar=c["planar"], stride=c["stride"], exact_depth=False)
        d["channels"] = (25 if c["planar"] else c["channels"]) if c["mode"] == 0 else (3 if c["colors"] is not None else 0)
        return d
    mode, V, G, channels, planar, stride = PROJ_FWD_NEW[name]
    rng = np.random.default_rng(sum(map(ord, name.replace("_planar", ""))) + 11)  # (k2_mixed_planar: k2_mixed's values in the other layout)
    W, H = 96, 64
    c2w0 = B._c2w(rng)
    eye = torch.eye(4, dtype=DD)
    exact = False
    opac = torch.from_numpy(rng.uniform(0.05, 0.95, G)).float()
    cov6 = _covs(rng, G)
    if mode == 0:
        deg = {4: 1, 9: 2, 25: 4, 1: 0}[channels]
        if name.startswith("k2_v"):
            # the views of chunk c (16 views) look along +z for even c, backwards for odd c: the Gaussians in front are culled in every
            # view of the odd chunks, the block behind the camera in every view of the even ones
            c2ws = []
            for v in range(V):
                c = c2w0.clone()
                c[:3, :3] = c2w0[:3, :3] @ B._rotation(rng, 0.04)
                c[:3, 3] = c2w0[:3, 3] + torch.from_numpy(rng.normal(size=3) * 0.05)
                c2ws.append(_flip(c) if (v // 16) % 2 else c)
            cams = [B.k2_cam(W, H, c, deg) for c in c2ws]
            lim = B.lens_limits(0, cams[0])[2]
            means = torch.cat([_cloud(rng, c2w0, G - 80, lim), _cloud(rng, _flip(c2w0), 80, lim)])
        elif name.startswith("k2_mixed"):
            fwd = c2w0.clone()
            fwd[:3, 3] = c2w0[:3, 3] + 2.2 * c2w0[:3, 2]  # view 0 (degree 0) stands 2.2 further along its axis: the near block is behind it
            c2ws = [fwd, c2w0, c2w0.clone(), _flip(c2w0)]
            c2ws[2][:3, :3] = c2w0[:3, :3] @ B._rotation(rng, 0.05)
            cams = [B.k2_cam(W, H, c, d_, b_) for c, (d_, b_) in zip(c2ws, MIXED_DEGREES)]
            lim = B.lens_limits(0, cams[0])[2]
            means = torch.cat([_cloud(rng, c2w0, 120, lim, 3.0, 5.0, 0.5), _cloud(rng, c2w0, 100, lim, 1.0, 2.0), _cloud(rng, _flip(c2w0), 80, lim)])
        elif name == "k2_depth":
            cams = [B.k2_cam(W, H, eye, deg)]
            thr = cams[0].k2_znear_cull
            z = [_ulps(thr, k) for k in (-2, -1, 0, 1, 2, 3)] * 2
            means = torch.tensor([[0.01 * (i % 3 - 1), 0.01 * (i % 2), zz] for i, zz in enumerate(z)], dtype=torch.float32)
            cov6, exact = _covs(rng, G, 0.002, 0.004), True
        elif name == "k2_nonfinite":
            cams = [B.k2_cam(W, H, c2w0, deg)]
            means = _cloud(rng, c2w0, G, B.lens_limits(0, cams[0])[2])
            means[64, 1] = float("nan")
            cov6[65, 0] = float("inf")
        else:
            cams = [B.k2_cam(W, H, c2w0, deg, deg == 4)]
            lim = B.lens_limits(0, cams[0])[2]
            means = _cloud(rng, c2w0, G, lim, spread=1.6 if name == "k2_edges" else 0.95)
        colors = torch.from_numpy(rng.normal(size=(G, channels, 3)) * 0.05)
        colors[:, 0, :] = torch.from_numpy(np.where(np.arange(3)[None] < ((np.arange(G) // 6) % 4)[:, None], -4.0, 1.5))
        colors = colors.float()
    else:
        colors = torch.from_numpy(rng.uniform(0.0, 1.0, (G, channels))).float() if channels else None
        if name == "k3_oae":
            cams = [B.k3_cam(W, H, c) for c in (c2w0, c2w0.clone())]
            cams[1].w2c[3] += 0.05
            for cam in cams:
                cam.opacity_aware_extent, cam.extent_sigma = 1, 2.0  # (at 3.33 the logarithmic extent is the smaller one for every opacity <= 1)
            means = _cloud(rng, c2w0, G, B.lens_limits(1, cams[0])[2])
            amin = float(F32(cams[0].alpha_min))
            o = rng.uniform(0.03, 0.95, G)  # logarithmic extent > 2 above 0.029
            o[0::5] = rng.uniform(0.0045, 0.027, len(o[0::5]))  # the logarithmic extent is the smaller one
            o[1::10] = rng.uniform(0.0005, 0.0038, len(o[1::10]))  # below alpha_min
            o[2::30] = [_ulps(amin, -1), amin, amin * 1.05] * 3 + [amin]
            opac = torch.from_numpy(o).float()
            cov6 = _covs(rng, G, 0.05, 0.2)
        elif name == "k3_clip":
            cams = [B.k3_cam(W, H, eye)]
            cams[0].radius_clip, cams[0].eps2d = 2.0, 0.01
            fx, fy = cams[0].fx, cams[0].fy
            z = 2.0
            tgt = np.array([0.7, 1.6, 2.5])  # extent x sqrt(c): radii 1, 2, 3
            ix, iy = np.arange(G) % 3, (np.arange(G) // 3) % 3
            c00, c11 = (tgt[ix] / 3.33) ** 2 * rng.uniform(0.93, 1.07, G) ** 2, (tgt[iy] / 3.33) ** 2 * rng.uniform(0.93, 1.07, G) ** 2
            cov6 = torch.zeros(G, 6)
            cov6[:, 0] = torch.from_numpy((c00 - 0.01) * (z / fx) ** 2).float()
            cov6[:, 3] = torch.from_numpy((c11 - 0.01) * (z / fy) ** 2).float()
            cov6[:, 5] = 1e-4
            px, py = rng.uniform(10, W - 10, G), rng.uniform(10, H - 10, G)
            means = torch.from_numpy(np.stack([(px - cams[0].cx) / fx * z, (py - cams[0].cy) / fy * z, np.full(G, z)], -1)).float()
            exact = True
        elif name == "k3_depth":
            cams = [B.k3_cam(W, H, eye)]
            cams[0].near_plane, cams[0].far_plane = 0.25, 6.5
            z = [_ulps(t, k) for t in (0.25, 6.5) for k in (-2, -1, 0, 1, 2, 3)] * 2
            means = torch.tensor([[0.01 * (i % 3 - 1) * zz, 0.01 * (i % 2) * zz, zz] for i, zz in enumerate(z)], dtype=torch.float32)
            cov6, exact = _covs(rng, G, 0.002, 0.004), True
        elif name == "k3_nonfinite":
            cams = [B.k3_cam(W, H, c2w0)]
            means = _cloud(rng, c2w0, G, B.lens_limits(1, cams[0])[2])
            means[64, 1] = float("nan")
            cov6[65, 0] = float("inf")
        else:
            cams = [B.k3_cam(W, H, c2w0)]
            means = _cloud(rng, c2w0, G, B.lens_limits(1, cams[0])[2], spread=1.6 if name == "k3_edges" else 0.95)
    return dict(name=name, mode=mode, V=len(cams), G=G, cams=cams, means=means, cov6=cov6, opac=opac, colors=colors, channels=channels, planar=planar,
                stride=stride, exact_depth=exact)


def _finite_rows(c):
    return torch.isfinite(c["means"]).all(-1) & torch.isfinite(c["cov6"]).all(-1)


def proj_refs_for(c):
    """per view: rec, S, bound, ints (proj_int64) of a case dict; rows with a NaN mean / Inf covariance, and every row of a view whose
    pose is not finite (a singular c2w), are referenced as culled"""
    ok = _finite_rows(c)
    means, cov6 = c["means"].clone(), c["cov6"].clone()
    means[~ok], cov6[~ok] = c["means"][ok][0], c["cov6"][ok][0]
    out = []
    for cam in c["cams"]:
        col = c["colors"]
        if c["mode"] == 1 and (col is None or c["channels"] != 3):
            col = None
        dead = not np.isfinite(np.array(list(cam.w2c))).all()
        if dead:
            cam = copy.copy(cam)
            for i in range(16):
                cam.w2c[i] = float(i % 5 == 0)
            if c["mode"] == 0:
                for i in range(16):
                    cam.proj[i] = float(i % 5 == 0)
        rec, S, bound, aux = proj_record64(c["mode"], cam, means, cov6, c["opac"], col)
        ints = proj_int64(c["mode"], cam, rec, S, aux, c["opac"].numpy(), c["exact_depth"])
        bad = ~ok.numpy() | dead
        ints["valid"] = ints["valid"] & ~bad
        ints["rect"][bad], ints["radii"][bad], ints["tiles"][bad] = 0, 0, 0
        ints["why"][bad], ints["decided"][bad] = 2, True
        out.append(dict(rec=rec, S=S, bound=bound, aux=aux, ints=ints))
    return out


@functools.lru_cache(maxsize=None)
def proj_fwd_ref(name):
    return proj_refs_for(proj_fwd_case(name))


def nf_chunk(cams):
    n = 0
    for cam in cams:
        deg = cam.sh_degree
        ncf = 25 if (deg > 3 and cam.sh_band4) else (16 if deg > 2 else (9 if deg > 1 else (4 if deg > 0 else 1)))
        n = max(n, ncf * 3) if cam.mode == 0 else n
    return n


def check_projection(c, refs, got, log=None):
    """got: rec [V,G,12] float32, radii [V,G,2], rect [V,G,4], tiles [V,G], keys [V,G] uint32, stats [V,>=2] (numpy) and `fill`, the
    float32 the record buffer held before the call.  Asserts every contract of the header; -> dict of the worst ratios and shares"""
    mode, V, G = c["mode"], c["V"], c["G"]
    rec, fill = np.asarray(got["rec"]), got["fill"]
    worst, und = {}, 0
    for v in range(V):
        r, ints = refs[v], refs[v]["ints"]
        rect, radii, tiles, keys = (np.asarray(got[k][v]) for k in ("rect", "radii", "tiles", "keys"))
        area = (rect[:, 2] - rect[:, 0]).astype(np.int64) * (rect[:, 3] - rect[:, 1])
        gvalid = area != 0
        # self-consistency of every row, decided or not
        assert np.array_equal(tiles, area), f"view {v}: tiles_touched is not the rect's area"
        assert np.array_equal(keys == CULLED, ~gvalid), f"view {v}: a key is culled exactly when the rect is empty"
        assert np.array_equal(keys[gvalid], np.minimum(rec[v, gvalid, 2].view(np.uint32), np.uint32(0xFFFFFFFE))), f"view {v}: key != the record's depth bits"
        assert int(got["stats"][v][0]) == int(gvalid.sum()) and int(got["stats"][v][1]) == int(tiles.sum()), f"view {v}: stats are not the sums of what was written"
        dec = ints["decided"]
        und += int((~dec).sum())
        for k in ("rect", "radii"):
            bad = np.flatnonzero(dec & (np.asarray(got[k][v]) != ints[k]).any(-1))
            assert bad.size == 0, f"view {v}: {k} of decided rows {bad[:8]}: got {np.asarray(got[k][v])[bad[:4]]}, want {ints[k][bad[:4]]} (why {ints['why'][bad[:4]]})"
        assert np.array_equal(gvalid[dec], ints["valid"][dec]), f"view {v}: valid flag of a decided row"
        # undecided rows take a neighbouring outcome
        assert (np.abs(radii[~dec] - ints["radii"][~dec]) <= np.maximum(1, ints["radii"][~dec])).all()
        # the record
        assert (rec[v, :, 3] == 0).all(), f"view {v}: rec[..., 3] must be exactly 0 on every row"
        both = gvalid & ints["valid"]
        assert np.array_equal(rec[v, :, 7], c["opac"].numpy()), "opacity is a copy"
        for k, slot in ((B.MX, 0), (B.MY, 1), (B.ZZ, 2), (B.CA, 4), (B.CB, 5), (B.CC, 6)):
            w, i = B.worst_ratio(rec[v, both, slot], r["rec"][both, k], r["S"][both, k], r["bound"][k])
            worst[k] = max(worst.get(k, 0.0), w)
            assert w <= 1.0, f"{c['name']} view {v} slot {k}: row {np.flatnonzero(both)[i]} is {w:.2f} x the bound"
        if c["exact_depth"]:
            assert np.array_equal(rec[v, :, 2], c["means"].numpy()[:, 2]), "identity pose: tz is the mean's z bit for bit"
        writes = mode == 0 or (c["colors"] is not None and c["channels"] == 3)
        fb = np.float32(fill).view(np.uint32)
        if writes:
            assert (rec[v, gvalid, 11] == 0).all(), "rec[..., 11] is exactly 0 where the colour slot is written"
            if mode == 0 and c["cams"][v].sh_degree >= 0:
                for ch in range(3):
                    w, i = B.worst_ratio(rec[v, both, 8 + ch], r["rec"][both, B.RR + ch], r["S"][both, B.RR + ch], SH_FWD_BOUND)
                    worst["col"] = max(worst.get("col", 0.0), w)
                    assert w <= 1.0, f"{c['name']} view {v} colour {ch}: row {np.flatnonzero(both)[i]} is {w:.2f} x the bound"
            else:
                src = c["colors"].numpy().reshape(G, 3)
                assert np.array_equal(rec[v, gvalid, 8:11], src[gvalid]), "precomputed / record colours are copies"
            assert (rec[v, ~gvalid, 8:12].view(np.uint32) == fb).all(), "rp[2] of a culled row keeps the fill"
        else:
            assert (rec[v, :, 8:12].view(np.uint32) == fb).all(), "mode 1 without three colour channels never writes rp[2]"
    share = und / float(V * G)
    assert share <= ZERO_SHARE_CAP, f"{c['name']}: {share:.4f} of the rows are undecided"
    if log is not None:
        log(c["name"], worst, share)
    return worst, share


# ---- pose kernels -----------------------------------------------------------------------------------------------------------------------
def pose_inverse64(E):
    """adjugate inverse of a 4 x 4 (numpy float64) -> W, err [4,4] (the float64 evaluation error bound of the header), or None, None when
    singular.  Evaluated in longdouble so that the reference's own error is below the bound it states."""
    E = np.asarray(E, np.longdouble)
    idx = [0, 1, 2, 3]
    cof, cof_abs = np.zeros((4, 4), np.longdouble), np.zeros((4, 4), np.longdouble)
    for i in range(4):
        for j in range(4):
            rows, cols = [r for r in idx if r != i], [c_ for c_ in idx if c_ != j]
            M = E[np.ix_(rows, cols)]
            terms = [M[0, 0] * M[1, 1] * M[2, 2], M[0, 1] * M[1, 2] * M[2, 0], M[0, 2] * M[1, 0] * M[2, 1], -M[0, 2] * M[1, 1] * M[2, 0],
                     -M[0, 1] * M[1, 0] * M[2, 2], -M[0, 0] * M[1, 2] * M[2, 1]]
            cof[i, j] = ((-1) ** (i + j)) * sum(terms)
            cof_abs[i, j] = sum(abs(t) for t in terms)
    det = sum(E[0, j] * cof[0, j] for j in range(4))
    D = sum(abs(E[0, j]) * cof_abs[0, j] for j in range(4))
    if det == 0:
        return None, None
    Winv = (cof.T / det).astype(np.float64)
    err = (12 * U53 * (cof_abs.T + np.abs(cof.T / det) * D) / abs(det)).astype(np.float64)
    return Winv, err


def pose_c2w64(cam, c2w, Kn, t_scale):
    """cam_pose_c2w_kernel restated: -> dict field -> (value float64 array, float64 evaluation error); a singular pose: w2c None"""
    E = np.asarray(c2w, np.float32).astype(np.float64).reshape(4, 4).copy()
    for i in (3, 7, 11):
        E.flat[i] = float(F32(F32(E.flat[i]) * F32(t_scale)))
    Wm, err = pose_inverse64(E)
    out = dict(campos=(E[:3, 3].copy(), np.zeros(3)))
    K = np.asarray(Kn, np.float32).astype(np.float64).reshape(3, 3)
    if Wm is None:
        out["w2c"] = (None, None)
    else:
        out["w2c"] = (Wm.reshape(-1), err.reshape(-1))
    if cam.mode == 0:
        Ki = np.linalg.inv(K.astype(np.longdouble).astype(np.float64))
        ray = lambda x, y: (lambda r: r / np.linalg.norm(r))(Ki @ np.array([x, y, 1.0]))
        fov_x = math.acos(min(1.0, max(-1.0, float(ray(0.0, 0.5) @ ray(1.0, 0.5)))))
        fov_y = math.acos(min(1.0, max(-1.0, float(ray(0.5, 0.0) @ ray(0.5, 1.0)))))
        tx, ty = math.tan(0.5 * fov_x), math.tan(0.5 * fov_y)
        e = 400 * U53
        out["tanfovx"], out["tanfovy"] = (np.array([tx]), np.array([e * tx])), (np.array([ty]), np.array([e * ty]))
        near, far = float(cam.k2_near), float(cam.k2_far)
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1], P[3, 2], P[2, 2], P[2, 3] = 1.0 / tx, 1.0 / ty, 1.0, far / (far - near), -(far * near) / (far - near)
        if Wm is not None:
            out["proj"] = ((P @ Wm).reshape(-1), (np.abs(P) @ (err + e * np.abs(Wm))).reshape(-1))
    else:
        for k, (i, n) in dict(fx=(0, cam.width), fy=(4, cam.height), cx=(2, cam.width), cy=(5, cam.height)).items():
            out[k] = (np.array([float(F32(F32(K.flat[i]) * F32(n)))]), np.zeros(1))
    return out


def pose_close(got, ref, err):
    """|got - ref| <= half an fp32 ulp of the value + the float64 evaluation error, per element"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    half = 0.5 * np.spacing(np.abs(ref).astype(F32)).astype(np.float64)
    return bool((np.abs(got - ref) <= half + err).all())


# ---- composites: the float64 maps with their tolerances, n_touched windows -----------------------------------------------------------------
def composite_fwd64(kind, cam, rec, lists, feats=None, nt_post=True, cache=None):
    """One view.  rec [G,12] fp32 records, lists (tile_start, ids), feats [G,C] (kind "feat").  -> dict out [H,W,C] (channel-last for every
    kind), alpha, depth [H,W], tol_out, tol_alpha, tol_depth (the header's bound, element by element), margin [H,W] (with the n_touched
    threshold), blends [H,W] (any entry blended), nt_lo, nt_hi [G], nt_reach [G] and counts.  cache: dense_raster_bwd64's walk cache."""
    k3 = kind != "k2"
    H, W = cam.height, cam.width
    rec = np.asarray(rec, np.float64)
    G = rec.shape[0]
    ts, ids_all = np.asarray(lists[0], np.int64), np.asarray(lists[1], np.int64)
    F = np.asarray(feats, np.float64) if kind == "feat" else rec[:, 8:11]
    C = F.shape[1]
    bg = np.array([float(F32(x)) for x in cam.bg]) if kind == "k2" else np.zeros(C)
    out, tol, S_out = np.zeros((H, W, C)), np.zeros((H, W, C)), np.zeros((H, W, C))
    alpha, tol_a, depth, tol_d, S_d = (np.zeros((H, W)) for _ in range(5))
    margin = np.full((H, W), np.inf)
    blends = np.zeros((H, W), bool)
    nt_lo, nt_und, walks = np.zeros(G, np.int64), np.zeros(G, np.int64), {}
    cnt = dict(blend=0, saturated=0, longest_list=0, nt_flip=0)
    if kind == "k2":
        out[:] = bg
    for tile in range(ts.shape[0] - 1):
        ids = ids_all[ts[tile]:ts[tile + 1]]
        L = ids.shape[0]
        cnt["longest_list"] = max(cnt["longest_list"], L)
        if L == 0:
            continue
        px, py, inside, off = B._tile_pixels(cam, tile, k3)
        if cache is not None and tile in cache:
            w, mt, (e_a, e_Tb, e_Tf) = cache[tile]
        else:
            w = B._walk(cam, rec[ids], px, py, inside, off, k3, False)
            ce = B._chain_errors(w)
            mt, (e_a, e_Tb, e_Tf) = B._tile_margin(cam, w), (ce[1], ce[3], ce[4])
            if cache is not None:
                cache[tile] = (w, mt, (e_a, e_Tb, e_Tf))
        bl, a, Tb = w["bl"], w["a"], w["Tb"]
        mt = mt.copy()
        if kind == "k2":
            step = U24 + e_a * a / (1.0 - a)
            Tq, eq = (w["nT"], e_Tb + step) if nt_post else (Tb, e_Tb)
            with np.errstate(divide="ignore", invalid="ignore"):
                m_nt = np.where(bl & (eq > 0), np.abs(Tq - 0.5) / (0.5 * eq), np.inf)
            mt = np.minimum(mt, m_nt.min(0, initial=np.inf))
            decided = (mt >= MARGIN) & inside
            counted = bl & (Tq > 0.5)
            np.add.at(nt_lo, ids, (counted & decided[None]).sum(1))
            np.add.at(nt_und, ids, (w["reached"] & (~decided & inside)[None]).sum(1))
            cnt["nt_flip"] += int((bl & ~counted).sum())
        wt = np.where(bl, a * Tb, 0.0)
        n_behind = np.cumsum(bl[::-1], 0)[::-1] - bl
        ew = np.where(bl, wt * (e_a + e_Tb + (K_FWD + n_behind) * U24), 0.0)
        Fi, z = F[ids], rec[ids, 2]
        Tf = w["T"]
        sel = (py[inside], px[inside])
        out[sel] = (wt.T @ Fi + Tf[:, None] * bg[None])[inside]
        tol[sel] = (ew.T @ np.abs(Fi) + (Tf * (e_Tf + U24))[:, None] * np.abs(bg)[None])[inside]
        S_out[sel] = (wt.T @ np.abs(Fi) + Tf[:, None] * np.abs(bg)[None])[inside]
        S_d[sel] = (wt * np.abs(z)[:, None]).sum(0)[inside]
        alpha[sel], tol_a[sel] = wt.sum(0)[inside], ew.sum(0)[inside]
        depth[sel], tol_d[sel] = (wt * z[:, None]).sum(0)[inside], (ew * np.abs(z)[:, None]).sum(0)[inside]
        margin[sel] = mt[inside]
        blends[sel] = bl.any(0)[inside]
        cnt["blend"] += int(bl.sum())
        sat = w["saturated"] & inside
        cnt["saturated"] += int(sat.sum())
        walks[tile] = w
    blank = ~blends
    tol[blank], tol_a[blank], tol_d[blank] = 0.0, 0.0, 0.0  # nothing blended: the background bit for bit / exactly 0
    return dict(out=out, alpha=alpha, depth=depth, tol_out=tol, tol_alpha=tol_a, tol_depth=tol_d, S_out=S_out, S_alpha=alpha, S_depth=S_d, margin=margin, blends=blends, nt_lo=nt_lo,
                nt_hi=nt_lo + nt_und, counts=cnt, walks=walks)


def quadrant_lists_k2(cam, rec, ids, tile, k3=False):
    """quadrant_mask (siu3r_amd/csrc/raster_shared.h) in float64 for the entries `ids` of one tile -> mask [L] (bit = quadrant)"""
    r = np.asarray(rec, np.float64)[ids]
    gw = -(-cam.width // TILE)
    x0t, y0t = (tile % gw) * TILE, (tile // gw) * TILE
    amin = float(F32(cam.alpha_min))
    with np.errstate(all="ignore"):
        Lg = np.log(r[:, 7] / amin)
        det = r[:, 4] * r[:, 6] - r[:, 5] ** 2
        pad = 0.55 if k3 else 0.05
        ex, ey = np.sqrt(2 * Lg * r[:, 6] / det) * 1.01 + pad, np.sqrt(2 * Lg * r[:, 4] / det) * 1.01 + pad
        x0, x1, y0, y1 = r[:, 0] - ex - x0t, r[:, 0] + ex - x0t, r[:, 1] - ey - y0t, r[:, 1] + ey - y0t
        cx = ((x0 <= 7) & (x1 >= 0)) * 1 | ((x0 <= 15) & (x1 >= 8)) * 2
        cy = ((y0 <= 7) & (y1 >= 0)) * 1 | ((y0 <= 15) & (y1 >= 8)) * 2
        mk = np.where(cy & 1, cx, 0) | np.where(cy & 2, cx << 2, 0)
        mk = np.where(Lg <= 0, 0, np.where(det > 0, mk, 15))
    return mk


def refill_rounds(passes):
    """composite_rgb_kernel's refill loop restated for one tile, none of whose pixels saturates early: passes [E] bool, does entry i of the
    tile's bin cover the tile -> list of (staged at the loop test, slices committed kk, staged after, base after) per refill, and the
    number of walks"""
    E = len(passes)
    base, rounds, walks = 0, [], 0
    while True:
        staged = 0
        while staged < STG_PULL and base < E:
            s0, run, kk = staged, staged, 0
            for k in range(FK):
                tk = int(np.sum(passes[base + 256 * k: base + 256 * (k + 1)]))
                if kk == k and run + tk <= STG:
                    kk, run = k + 1, run + tk
            staged, base = run, base + 256 * kk
            rounds.append((s0, kk, staged, base))
        if staged == 0:
            break
        walks += 1
    return rounds, walks


# ---- composites: float32 emulation (and the wrong answers) --------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def composite_emul32(kind, cam, rec, lists, feats=None, nt_post=True, mutate=None, ring_np=None):
    """the composite of `kind` in float32 with the kernels' operations: _walk(f32=True) decides, the sums are fused multiply-adds in list
    order.  mutate: one wrong answer of the list in tests/test_raster_fwd_stages_ref.py.  -> out [H,W,C], alpha, depth, n_touched [G]"""
    mutate = mutate or {}
    k3 = kind != "k2"
    H, W = cam.height, cam.width
    rec32 = np.asarray(rec, F32)
    G = rec32.shape[0]
    ts, ids_all = np.asarray(lists[0], np.int64), np.asarray(lists[1], np.int64)
    F = np.asarray(feats, F32) if kind == "feat" else rec32[:, 8:11]
    C = F.shape[1]
    bg = np.array([F32(x) for x in cam.bg], F32) if kind == "k2" else np.zeros(C, F32)
    out, alpha, depth = np.zeros((H, W, C), F32), np.zeros((H, W), F32), np.zeros((H, W), F32)
    nt = np.zeros(G, np.int64)
    if kind == "k2":
        out[:] = bg
    cam_ = cam
    if mutate.get("no_alpha_max"):
        cam_ = copy.copy(cam)
        cam_.alpha_max = 1e30
    le = (not k3) if mutate.get("flip_sat") else k3
    for tile in range(ts.shape[0] - 1):
        ids = ids_all[ts[tile]:ts[tile + 1]]
        if ids.shape[0] == 0:
            continue
        px, py, inside, off = B._tile_pixels(cam, tile, k3)
        if mutate.get("no_half") and k3:
            off = 0.0
        quads = [(inside, ids, None)]
        if any(mutate.get(k) for k in ("dead_pair", "sat_pair", "ring_slot")):  # the wrong answers that depend on per-quadrant list positions
            lx, ly = px % TILE, py % TILE
            mk = quadrant_lists_k2(cam, rec32, ids, tile, k3)
            quads = []
            for q in range(4):
                pm = inside & ((lx >= 8) == bool(q & 1)) & ((ly >= 8) == bool(q >> 1))
                qi = ids[(mk >> q) & 1 == 1]
                quads.append((pm, qi, ids))
        for pm, qi, tile_ids in quads:
            n = qi.shape[0]
            if n == 0 or not pm.any():
                continue
            walk_ids = qi
            if mutate.get("dead_pair") and n % 2 == 1:
                walk_ids = np.concatenate([qi, tile_ids[:1]])  # the dead half of the last pair reads staged record 0
            w = B._walk(cam_, rec32[walk_ids], px, py, pm, off, k3, True, sat_le=le)
            bl, a, Tb = w["bl"], w["a"].astype(F32), w["Tb"].astype(F32)
            if mutate.get("sat_pair"):
                # a pixel that saturates on the first entry of a pair still blends the second
                first = np.argmax(~bl & w["reached"] & w["static"] & pm[None], 0)  # the saturating entry (a reached, static, unblended one)
                has = w["saturated"]
                for p_ in np.flatnonzero(has & (first % 2 == 0) & (first + 1 < len(walk_ids))):
                    j = first[p_] + 1
                    if w["static"][j, p_]:
                        bl[j, p_] = True
                        Tb[j, p_] = Tb[first[p_], p_]
            Fw = F[walk_ids]
            if mutate.get("ring_slot"):
                src = np.arange(len(walk_ids))
                src = np.where(src >= 24, src - 24, src)  # chunk k reads the ring slot chunk k - 3 left
                Fw = F[walk_ids[src]]
            acc = np.zeros((px.shape[0], C), F32)
            O, D = np.zeros(px.shape[0], F32), np.zeros(px.shape[0], F32)
            z = rec32[walk_ids, 2]
            T_last = np.ones(px.shape[0], F32)
            for j in range(len(walk_ids)):
                b = bl[j]
                if not b.any():
                    continue
                wj = (a[j] * Tb[j]).astype(F32)
                acc[b] = _fma32(Fw[j][None, :], wj[b][:, None], acc[b])
                D[b] = _fma32(z[j], wj[b], D[b])
                O[b] = (O[b] + wj[b]).astype(F32)
                if kind == "k2":
                    Tq = (w["nT"][j] if nt_post else Tb[j])
                    nt[walk_ids[j]] += int((b & (Tq > F32(0.5))).sum())
                T_last = np.where(b, Tb[j] if mutate.get("bg_before_last") else w["nT"][j].astype(F32), T_last)
            if kind == "k2":
                acc = _fma32(T_last[:, None], bg[None, :], acc)
            sel = (py[pm], px[pm])
            out[sel], alpha[sel], depth[sel] = acc[pm], O[pm], D[pm]
    if kind == "feat" and ring_np:
        out = _window_mutations(out, C, ring_np, mutate)
    if mutate.get("alpha_other_chunk") and kind == "feat" and -(-C // 32) < 2:
        alpha[:] = np.nan  # no second chunk exists: alpha is never written
    return dict(out=out, alpha=alpha, depth=depth, n_touched=nt)


def feat5_windows(C, np_max=6):
    """the channel windows of composite_feat5_kernel -> NP, [(ch0, [window start channel per 32-wide block])] per blockIdx.y"""
    NP = np_max if C >= 32 * np_max else -(-C // 32)
    CW = 32 * NP
    out = []
    for by in range(-(-C // CW)):
        ch0 = min(by * CW, max(0, C - CW))
        nch = min(CW, C - ch0)
        out.append((ch0, [ch0 + (nch - 32 if nb == NP - 1 else 32 * nb) for nb in range(NP)]))
    return NP, out


def _window_mutations(out, C, np_max, mutate):
    """the last channel window read where an unshifted one would lie (and written where the shifted one belongs): within a chunk, the last
    32-wide block of a workgroup at 32 (NP - 1) for last_off; for the last chunk, ch0 = blockIdx.y * CW for C - CW.  Columns past the row
    read as 0 (the buffer resource's range check)"""
    NP, wins = feat5_windows(C, np_max)
    CW = 32 * NP
    res = out.copy()

    def shifted(lo, hi, s):
        src = np.zeros_like(out[..., lo:hi])
        n = max(0, min(hi + s, C) - (lo + s))
        if n > 0:
            src[..., :n] = out[..., lo + s:lo + s + n]
        res[..., lo:hi] = src

    if mutate.get("window_unshifted"):
        for ch0, starts in wins:
            s_ = ch0 + 32 * (NP - 1) - starts[-1]
            if s_:
                shifted(starts[-1], starts[-1] + 32, s_)
    if mutate.get("chunk_unshifted"):
        ch0 = wins[-1][0]
        s_ = (len(wins) - 1) * CW - ch0
        if s_:
            shifted(ch0, min(ch0 + CW, C), s_)
    return res


# ---- the forward-only composite cases ------------------------------------------------------------------------------------------------------
#                 kind   W   H  V  scene        channels
FWD_COMP_CASES = {
    "k2_stage":   ("k2", 96, 64, 1, "stage", 3),
    "k2_pairs":   ("k2", 96, 64, 1, "pairs", 3),
    "k2_satpair": ("k2", 96, 64, 1, "satpair", 3),
    "k3_satpair": ("k3", 96, 64, 1, "satpair", 3),
    "k2_nt_pre":  ("k2", 96, 64, 2, "full", 3),
    "feat_ring":  ("feat", 96, 64, 1, "ring", 385),
    "feat_ring_ragged": ("feat", 90, 62, 2, "ring", 65),
    "feat_batch": ("feat", 96, 64, 1, "batch", 33),
    "feat_sat_early": ("feat", 96, 64, 1, "sat_early", 65),
}
RING_LENGTHS = (1, 7, 8, 9, 16, 17, 24, 25, 70)
RING_TILES = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (0, 2), (1, 2), (5, 2))  # quadrant 0 of each; Gaussian 0's footprint reaches none
RING_CHANNELS = (32, 33, 64, 65, 96, 97, 160, 161, 192, 193, 385)
BATCH_LENGTHS = (127, 128, 129, 257)
BATCH_TILES = ((0, 0), (2, 0), (4, 0), (1, 2))
BATCH_CHANNELS = (1, 31, 32, 33)
PAIR_COUNTS = {(0, 0): (1, 0, 2, 3), (2, 2): (4, 5, 6, 7)}  # tile -> listed entries per quadrant
STAGE_PLAN = ((250, 3, 3), (250, 3, 3), (100, 78, 78), (40, 104, 112), (60, 10, 10))  # per slice of 256 bin entries: coverers of tiles (0,0), (1,0), (2,0)


def _fwd_scene_view(kind, W, H, scene, rng):
    gw, gh = -(-W // TILE), -(-H // TILE)
    parts = []

    def add(n, mx, my, sx, sy, op, depth, th=None):
        parts.append(np.stack([np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in (mx, my, sx, sy, rng.uniform(0, np.pi, n) if th is None else th, op, depth)], -1))

    if scene == "stage":
        d = 1.0
        for na, nb_, nc in STAGE_PLAN:
            n = na + nb_ + nc
            which = rng.permutation(np.repeat([0, 1, 2], [na, nb_, nc]))  # interleaved in depth inside the slice
            add(n, which * TILE + rng.uniform(6.5, 9.5, n), rng.uniform(6.5, 9.5, n), 1.5, 1.5, rng.uniform(0.02, 0.05, n), d + 1e-3 * np.arange(n))
            d += 1e-3 * n
    elif scene == "pairs":
        for (tx, ty), counts in PAIR_COUNTS.items():
            span = counts[0] >= 4
            if span:  # one splat over all four quadrants, frontmost: staged record 0 of the tile, on every quadrant's list
                add(1, tx * TILE + 7.5, ty * TILE + 7.5, 4.0, 4.0, 0.6, 0.5)
            for q, n in enumerate(counts):
                n -= 1 if span else 0
                add(n, tx * TILE + 3.5 + 8 * (q & 1) + rng.uniform(-0.3, 0.3, n), ty * TILE + 3.5 + 8 * (q >> 1) + rng.uniform(-0.3, 0.3, n), 1.0, 1.0,
                    rng.uniform(0.2, 0.5, n), rng.uniform(1, 3, n))
    elif scene == "satpair":
        add(10, 40.0 + rng.uniform(-1, 1, 10), 24.0 + rng.uniform(-1, 1, 10), 8.0, 8.0, 0.95, 0.9 + 0.01 * np.arange(10))
        add(40, rng.uniform(0, W, 40), rng.uniform(0, H, 40), 2.5, 2.5, rng.uniform(0.2, 0.8, 40), rng.uniform(2, 5, 40))
    elif scene == "ring":
        add(1, W / 2, H / 2, 6.0, 6.0, 0.8, 1.2)  # Gaussian 0, heavy: the padding of a chunk reads its record and feature row
        for (tx, ty), n in zip(RING_TILES, RING_LENGTHS):
            add(n, tx * TILE + 4.0 + rng.uniform(-0.3, 0.3, n), ty * TILE + 4.0 + rng.uniform(-0.3, 0.3, n), 1.0, 1.0, 0.04, rng.uniform(2, 5, n))
    elif scene == "batch":
        add(1, 5 * TILE + 8.0, 3 * TILE + 8.0, 1.0, 1.0, 0.5, 1.2)
        for (tx, ty), n in zip(BATCH_TILES, BATCH_LENGTHS):
            add(n, tx * TILE + rng.uniform(6.5, 9.5, n), ty * TILE + rng.uniform(6.5, 9.5, n), 1.5, 1.5, rng.uniform(0.02, 0.05, n), rng.uniform(2, 5, n))
    elif scene == "sat_early":
        x0, y0 = 2 * TILE, TILE  # tile (2, 1): quadrant 0 saturates inside its first chunk, quadrant 1 never does
        add(8, x0 + 4.0 + rng.uniform(-0.2, 0.2, 8), y0 + 4.0 + rng.uniform(-0.2, 0.2, 8), 8.0, 8.0, 0.99, 0.5 + 0.01 * np.arange(8), th=0.0)
        add(40, x0 + 8.0 + rng.uniform(-1, 1, 40), y0 + 4.0 + rng.uniform(-1, 1, 40), 3.0, 3.0, 0.3, rng.uniform(2, 5, 40))
    p = np.concatenate(parts)
    G = p.shape[0]
    rec = np.zeros((G, 12))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7] = p[:, 0], p[:, 1], p[:, 6], p[:, 5]
    rec[:, 4], rec[:, 5], rec[:, 6] = B._conic(p[:, 2], p[:, 3], p[:, 4])
    rec[:, 8:11] = rng.uniform(0.0, 1.2, (G, 3))
    return rec.astype(np.float32), B._rects(W, H, p[:, 0], p[:, 1], 3.33 * np.maximum(p[:, 2], p[:, 3]))


@functools.lru_cache(maxsize=None)
def fwd_comp_case(name):
    """a case of B.COMP_CASES (its dict, as comp_case returns it) or of FWD_COMP_CASES (the same keys)"""
    if name in B.COMP_CASES:
        return B.comp_case(name)
    kind, W, H, V, scene, C = FWD_COMP_CASES[name]
    if name == "k2_nt_pre":
        c = {k: v for k, v in B.comp_case("k2_full").items() if not isinstance(k, tuple)}  # (not the references cached on k2_full)
        c["cams"] = [copy.copy(cam) for cam in c["cams"]]
        for cam in c["cams"]:
            cam.nt_post_blend = 0
        c["name"] = name
        return c
    seed = sum(map(ord, scene + kind)) + W + 3
    rng = np.random.default_rng(seed)
    views = [_fwd_scene_view(kind, W, H, scene, rng) for _ in range(V)]
    rec, rect = np.stack([v[0] for v in views]), np.stack([v[1] for v in views])
    G = rec.shape[1]
    c2w = torch.eye(4, dtype=DD)
    cams = [B.k2_cam(W, H, c2w) if kind == "k2" else B.k3_cam(W, H, c2w) for _ in range(V)]
    geo = RS.geometry_ref(W, H)
    live = (rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1]) != 0
    keys = np.where(live, rec[..., 2].view(np.uint32), np.uint32(RS.CULLED)).astype(np.uint32)
    sorted_ids = [s[1] for s in RS.sort_ref(keys)]
    bins = [RS.bin_ref(geo, sorted_ids[v], rect[v]) for v in range(V)]
    lists = [RS.tile_lists_ref(geo, *bins[v]) for v in range(V)]
    feats = None
    if kind == "feat":  # distinct per Gaussian and per channel: a row or a column from the wrong ring slot or window cannot cancel
        feats = ((np.arange(G)[:, None] + np.arange(C)[None] / 1024.0) / 64.0 * np.where(np.arange(G)[:, None] % 2, -1.0, 1.0)).astype(np.float32)
    return dict(name=name, kind=kind, W=W, H=H, V=V, G=G, C=C, cams=cams, geo=geo, rec=rec, rect=rect, sorted_ids=sorted_ids, bins=bins, lists=lists,
                feats=feats, scene=scene, walk_cache=[{} for _ in range(V)])


def case_feats(c, C):
    """the first C channels of a feat case's rows, contiguous"""
    return np.ascontiguousarray(c["feats"][:, :C])


def comp_fwd_ref(c, C=None):
    """per view composite_fwd64 of a case (feat: on its first C channels); cached on the case per C"""
    key = ("fwd_ref", C)
    if key not in c:
        kind = c["kind"]
        feats = case_feats(c, C or c["C"]) if kind == "feat" else None
        c[key] = [composite_fwd64(kind, c["cams"][v], c["rec"][v], c["lists"][v], feats, bool(c["cams"][v].nt_post_blend), c["walk_cache"][v])
                  for v in range(c["V"])]
    return c[key]


def check_maps(name, kind, refs, out, alpha, depth=None, n_touched=None, log=None):
    """out [V,H,W,C] (channel-last), alpha, depth [V,H,W], n_touched [V,G] (numpy) against comp_fwd_ref: every decided pixel within its
    tolerance, blank pixels exact, at most 1 % of a view's pixels undecided, n_touched inside its window -> worst ratio"""
    worst = 0.0
    for v, r in enumerate(refs):
        keep = r["margin"] >= MARGIN
        share = 1.0 - keep.mean()
        assert share <= ZERO_SHARE_CAP, f"{name} view {v}: {share:.4f} of the pixels lie below the margin"
        for what, got, ref, tol, S in (("out", out[v], r["out"], r["tol_out"], r["S_out"]), ("alpha", alpha[v], r["alpha"], r["tol_alpha"], r["S_alpha"])) + (
                (("depth", depth[v], r["depth"], r["tol_depth"], r["S_depth"]),) if depth is not None else ()):
            got = np.asarray(got, np.float64)
            k = keep if got.ndim == 2 else keep[..., None] & np.ones(got.shape, bool)
            d = np.abs(got - ref)
            assert not np.isnan(got[k]).any(), f"{name} view {v} {what}: NaN"
            blank = (tol == 0) & k
            assert (d[blank] == 0).all(), f"{name} view {v} {what}: a pixel that blends nothing must be exact (the background / 0)"
            ratio = np.where(k & (tol > 0), d / np.where(tol > 0, tol, 1.0), 0.0)
            w = float(ratio.max()) if ratio.size else 0.0
            worst = max(worst, w)
            if log is not None:  # the tolerance as a multiple of S, the sum of the absolute values of the element's terms
                rel = (tol / np.where(S > 0, S, 1.0))[k & (tol > 0) & (S > 0)]
                log(f"{name} view {v} {what}", w, float(np.median(rel)) if rel.size else 0.0, float(rel.max()) if rel.size else 0.0, share)
            assert w <= 1.0, f"{name} view {v} {what}: element {np.unravel_index(int(ratio.argmax()), ratio.shape)} is {w:.2f} x its bound"
        if n_touched is not None:
            nt = np.asarray(n_touched[v], np.int64)
            lo, hi = r["nt_lo"], r["nt_hi"]
            bad = np.flatnonzero((nt < lo) | (nt > hi))
            assert bad.size == 0, f"{name} view {v}: n_touched of {bad[:8]}: {nt[bad[:8]]} outside [{lo[bad[:8]]}, {hi[bad[:8]]}]"
            big = lo > 200
            assert ((hi - lo)[big] < 0.02 * lo[big]).all(), f"{name} view {v}: an n_touched window is too wide to check anything"
    return worst
