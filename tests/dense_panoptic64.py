"""Stage references, bounds, comparison rules and crafted cases of the panoptic post-process and the query-class-logit lifting
(siu3r_amd/csrc/postprocess.hip: pp_class, pp_mask256, pp_argmax, pp_accept, pp_write, pp_qcl; lift_pixel, lift_label, lift_fuse,
fill_i32), written from include/siu3r_hip.h, the kernels' comments and oracle/siu3r_oracle.py:632-729; shared by
tests/test_panoptic_stages_ref.py (CPU) and tests/test_panoptic_stages_gpu.py (GPU).  Every reference takes its stage's inputs as the
stage before it PRODUCED them (read back from the device, or from the float32 emulation below), so that each stage is judged alone.

BOUNDS (u = 2^-24, one float32 rounding per + - * /; the library is built with -ffp-contract=off and without fast-math: no fused
multiply-add, correctly rounded division; expf within 1 ulp = 2 u relative, the accuracy the ROCm device library documents for it; TINY =
2^-126 is added wherever a result may underflow: a device may flush what float64 still holds).
  class   a_c = l_c - max: one rounding of a number of size |a_c|, so exp(a_c) is off by |a_c| u relative, + 2 u for expf: e_c within
          (|a_c| + 2) u.  den: C - 1 additions of positive terms, (C - 1) u, + the terms' own errors weighted by their share, sum_c p_c
          (|a_c| + 2) u.  The quotient: u.
              |probs_c - ref| <= p_c ((|a_c| + 2) + (C - 1) + sum_c' p_c' (|a_c'| + 2) + 1) u + TINY
          score is the largest of them (same bound).  A row is EXACT when every a_c is 0 or <= -104 (expf gives 0: exp(-104) < 2^-149)
          and the number n of zeros is a power of two: e_c is 1 or 0, den = n and 1 / n are exact on the device and in float64, the
          comparison with thr is then between two exact float32 numbers (the one-hot +-80 rows: score 1.0; two equal logits at C = 2:
          score 0.5, which is NOT > 0.5).  Classes with bit-identical logits have bit-identical probabilities on the device: the first wins.
  src     src_idx: scale = in / out (u), scale (o + 0.5) (u; o + 0.5 is exact), - 0.5 (u of |src|): |src - ref| <= e_src = 4 u (src + 1).
          Where in == out the scale is 1.0, src = o and the weight l = 0 exactly: e_src = 0.  l = src - i0 is exact (Sterbenz).  A src
          within e_src of an integer may land in the neighbouring cell; bilinear interpolation is continuous across cells, so the value
          moves by at most e_src times a neighbouring cell's slope.
  lerp    (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11): the longest path is 1 - lx (u), its product (u), the inner sum
          (u), 1 - ly (u), the outer product (u), the outer sum (u): 6 u A, A = the same interpolation of |v| (the absolute terms).
              E_lerp = e_src_y Sy + e_src_x Sx + 6 u A
          Sy / Sx = the largest |difference| of vertically / horizontally neighbouring samples over the 3 x 3 cells around (y0, x0).
          Identity in BOTH axes: ly = lx = 0, (1 - 0) v00 = v00, 0 v = 0, v00 + 0 = v00: the value is the sample, bit for bit: E_lerp = 0.
  mask256 p = 1 / (1 + expf(-v)), |v - ref| <= E_v = E_lerp of the logits.  expf 2 u on e = exp(-v), 1 + e (u), the quotient (u): the
          relative error of p is 2 u e / (1 + e) + 2 u = (2 (1 - p) + 2) u, budgeted as (2 (1 - p) + 3) u; the argument's error moves p by
          E_v p (1 - p), second order E_v^2:
              |p256 - ref| <= E_v (p (1 - p) + E_v) + (2 (1 - p) + 3) u p + TINY
  argmax  wv = sample(plane_k) score_k: |wv - ref| <= E_w = E_lerp(plane_k) score_k + u wv (the inputs, read back, are exact).
          Identity target (H = W = mask_size): the sample is exact, wv = fl(p score) is ONE correctly rounded product, which numpy
          float32 reproduces bit for bit: every decision of such a case is decided, crafted equalities (wv == mask_thr) included.
  qcl     out = probs[q_j, c] sample(plane_{k_j}): |out - ref| <= probs E_lerp + u |out|.
  accept, write, lift: integers (and one float32 quotient, one float32 / double comparison): restated exactly, bound 0.

DECISIONS.  labels: decided when score - runner-up (the largest probability among the classes whose logit is not bit-identical to the
winner's) > the sum of the two bounds.  keep: exact rows, decided void rows, or |score - thr| > the score's bound.  lab_map: pixel
decided when wv_best - E_best > wv_k + E_k for every other k; a later query whose planes and score are bit-identical to an earlier one's
can never win (strict >) and is no candidate.  An undecided element must hold one of the candidates (wv_k + E_k >= wv_best - E_best).
area_k in [decided pixels of k, + undecided pixels with k among the candidates]; orig_k in [#(wv - E > thr), + #(|wv - thr| <= E)].
UNDECIDED_CAP: at most 0.5 % of a case's rows / pixels / (pixel, query) pairs may be undecided (asserted from the reference alone by
tests/test_panoptic_stages_ref.py; the cases are chosen so that it holds).

Not a test module."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
F32 = np.float32
F64 = np.float64
UNDECIDED_CAP = 0.005
FILL = F32(-0x5A5A5A5B)  # the sentinel of test_raster_stages_gpu._Guarded as a float32; as int32 it is SENT itself
SENT = -0x5A5A5A5B


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------
def src_idx(n_out, n_in, dtype=F64, variant=None):
    """src_idx of postprocess.hip for every output index -> i0, i1, l1, src.  variant "noclamp": without the clamp at 0;
    "align": align_corners=True sampling (both deliberately wrong)"""
    o = np.arange(n_out)
    if variant == "align":
        src = (o * ((n_in - 1) / max(n_out - 1, 1))).astype(dtype)
    elif dtype == F32:
        scale = F32(n_in) / F32(n_out)
        src = scale * (o.astype(F32) + F32(0.5)) - F32(0.5)
    else:
        src = (n_in / n_out) * (o + 0.5) - 0.5
    if variant != "noclamp":
        src = np.maximum(src, dtype(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (src - i0.astype(dtype)).astype(dtype), src


def bilinear(P, OH, OW, dtype=F64, variant=None):
    """P [..., IH, IW] -> [..., OH, OW] in `dtype`, the kernels' expression order"""
    P = np.asarray(P).astype(dtype)
    y0, y1, ly, _ = src_idx(OH, P.shape[-2], dtype, variant)
    x0, x1, lx, _ = src_idx(OW, P.shape[-1], dtype, variant)
    y0, y1, ly, x0, x1, lx = y0[:, None], y1[:, None], ly[:, None], x0[None, :], x1[None, :], lx[None, :]
    one = dtype(1)
    top = (one - lx) * P[..., y0, x0] + lx * P[..., y0, x1]
    bot = (one - lx) * P[..., y1, x0] + lx * P[..., y1, x1]
    return (one - ly) * top + ly * bot


def _spread3(d):
    H, W = d.shape[-2:]
    p = np.pad(d, [(0, 0)] * (d.ndim - 2) + [(1, 1), (1, 1)])
    out = d.copy()
    for a in range(3):
        for b in range(3):
            np.maximum(out, p[..., a:a + H, b:b + W], out=out)
    return out


def lerp_bound(P, OH, OW):
    """E_lerp of the header for every output of bilinear(P, OH, OW); P float64 (exact inputs)"""
    P = np.asarray(P, F64)
    IH, IW = P.shape[-2:]
    if IH == OH and IW == OW:
        return np.zeros(P.shape[:-2] + (OH, OW))
    y0, _, _, sy = src_idx(OH, IH)
    x0, _, _, sx = src_idx(OW, IW)
    ey = np.zeros(OH) if IH == OH else 4 * U * (sy + 1)
    ex = np.zeros(OW) if IW == OW else 4 * U * (sx + 1)
    dy, dx = np.zeros_like(P), np.zeros_like(P)
    dy[..., :-1, :] = np.abs(np.diff(P, axis=-2))
    dx[..., :, :-1] = np.abs(np.diff(P, axis=-1))
    Sy, Sx = _spread3(dy), _spread3(dx)
    g = (Ellipsis, y0[:, None], x0[None, :])
    return ey[:, None] * Sy[g] + ex[None, :] * Sx[g] + 6 * U * bilinear(np.abs(P), OH, OW)


def _worst(err, bound):
    """largest err / bound (0 / 0 = 0, x / 0 = inf)"""
    err, bound = np.asarray(err, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nanmax(r))


def _assert_within(got, ref, bound, what):
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    w = _worst(np.abs(got - ref), bound)
    assert w <= 1.0, f"{what}: worst element {w:.3f} of its bound"
    return w


# ---- stage references -------------------------------------------------------------------------------------------------------------------
def class_ref(cls, thr):
    """cls [B,Q,C] float32 -> dict: probs, bound [B,Q,C], score, label [B,Q], label_decided, cand [B,Q,C] (the classes an undecided row
    may report), keep, keep_decided [B,Q]"""
    l = cls.astype(F64)
    C = l.shape[-1]
    a = l - l.max(-1, keepdims=True)
    e = np.exp(a)
    p = e / e.sum(-1, keepdims=True)
    rel = (np.abs(a) + 2) + (C - 1) + (p * (np.abs(a) + 2)).sum(-1, keepdims=True) + 1
    bound = p * rel * U + TINY
    label = p.argmax(-1)
    score = np.take_along_axis(p, label[..., None], -1)[..., 0]
    sb = np.take_along_axis(bound, label[..., None], -1)[..., 0]
    same = cls == np.take_along_axis(cls, label[..., None], -1)  # bit-identical logits: identical bits on the device, the first wins
    cand = (~same) & (p + bound >= (score - sb)[..., None])
    label_decided = ~cand.any(-1)
    cand |= np.arange(C) == label[..., None]
    nz = (a == 0).sum(-1)
    exact = ((a == 0) | (a <= -104)).all(-1) & ((nz & (nz - 1)) == 0)
    score = np.where(exact, 1.0 / nz, score)
    s32 = score.astype(F32)
    keep = (label != C - 1) & (s32 > F32(thr))
    keep_decided = label_decided & (exact | (label == C - 1) | (np.abs(score - F64(F32(thr))) > sb))
    return dict(probs=p, bound=bound, score=score, score_bound=np.where(exact, 0.0, sb), label=label, label_decided=label_decided, cand=cand,
                keep=keep, keep_decided=keep_decided, exact=exact)


def mask256_ref(mcl, kept_idx, n_keep, MS, variant=None):
    """mcl [B,T,IH,IW,Q] float32, the device's kept_idx / n_keep -> list over b of (p [T,nk,MS,MS], bound)"""
    out = []
    for b in range(mcl.shape[0]):
        nk = int(n_keep[b])
        P = np.moveaxis(mcl[b][..., kept_idx[b, :nk]], -1, 1).astype(F64)  # [T,nk,IH,IW]
        v = bilinear(P, MS, MS, variant=variant)
        Ev = lerp_bound(P, MS, MS)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-v))
        out.append((p, Ev * (p * (1 - p) + Ev) + (2 * (1 - p) + 3) * U * p + TINY))
    return out


def _duplicates(planes32, sc32):
    """dup[k] = True when an earlier kept query has bit-identical planes and score"""
    nk = planes32.shape[1]
    dup = np.zeros(nk, bool)
    for k in range(1, nk):
        for j in range(k):
            if sc32[j] == sc32[k] and np.array_equal(planes32[:, j], planes32[:, k]):
                dup[k] = True
                break
    return dup


def argmax_ref(p256, scores, kept_idx, n_keep, b, H, W, mask_thr):
    """the device's planes p256 [B,T,Q,MS,MS] and scores [B,Q] (float32) -> dict for item b: best [T,H,W], cand [T,nk,H,W],
    decided [T,H,W], area_lo/hi, orig_lo/hi [nk], undecided_pairs"""
    nk, MS = int(n_keep[b]), p256.shape[-1]
    T = p256.shape[1]
    planes32 = p256[b, :, :nk]
    sc32 = scores[b, kept_idx[b, :nk]].astype(F32)
    if H == MS and W == MS:  # exact: one correctly rounded product
        wv = (planes32 * sc32[None, :, None, None]).astype(F64)
        bw = np.zeros_like(wv)
    else:
        P = planes32.astype(F64)
        wv = bilinear(P, H, W) * sc32.astype(F64)[None, :, None, None]
        bw = lerp_bound(P, H, W) * sc32.astype(F64)[None, :, None, None] + U * wv
    best = wv.argmax(1)  # the first maximum
    lo = np.take_along_axis(wv - bw, best[:, None], 1)
    cand = (wv + bw >= lo) & ~_duplicates(planes32, sc32)[None, :, None, None]
    np.put_along_axis(cand, best[:, None], True, 1)
    decided = cand.sum(1) == 1
    onehot = np.arange(nk)[None, :, None, None] == best[:, None]
    area_lo = (onehot & decided[:, None]).sum((0, 2, 3))
    area_hi = area_lo + (cand & ~decided[:, None]).sum((0, 2, 3))
    thr = F64(F32(mask_thr))
    maybe = (np.abs(wv - thr) <= bw) & (bw > 0)  # (bw == 0: wv is the device's own float32 number, the comparison is exact)
    sure = (wv >= thr) & ~maybe
    return dict(best=best, cand=cand, decided=decided, area_lo=area_lo, area_hi=area_hi, orig_lo=sure.sum((0, 2, 3)),
                orig_hi=sure.sum((0, 2, 3)) + maybe.sum((0, 2, 3)), undecided_pairs=int(maybe.sum()), pairs=int(wv.size), npix=T * H * W)


def accept_ref(area, orig, kept_idx, n_keep, labels, scores, b, overlap, fuse, f32_compare=False):
    """sequential acceptance of item b on the device's counters (oracle/siu3r_oracle.py:659-684): float32 quotient compared in DOUBLE with
    the double threshold.  -> seg_id [Q] (0 = rejected), rows {k: (label, fused, score)}, acc (list of k)"""
    Q = area.shape[1]
    seg_id, rows, acc = np.zeros(Q, np.int32), {}, []
    cur, stuff_mem = 0, {}
    for k in range(int(n_keep[b])):
        q = int(kept_idx[b, k])
        cls = int(labels[b, q])
        fuse_k = cls in fuse and cls < 32
        a, o = int(area[b, k]), int(orig[b, k])
        exists = a > 0 and o > 0
        if exists:
            ratio = F32(a) / F32(o)
            exists = bool(ratio > F32(overlap)) if f32_compare else float(ratio) > float(overlap)
        if not exists:
            continue
        if cls in stuff_mem:
            sid_f = stuff_mem[cls]
        else:
            cur += 1
            sid_f = cur
        sid = sid_f if fuse_k else cur
        seg_id[k] = sid
        rows[k] = (cls, int(fuse_k), F32(scores[b, q]))
        acc.append(k)
        if fuse_k and cls not in stuff_mem:
            stuff_mem[cls] = cur
    return seg_id, rows, acc


def write_ref(lab_map, seg_id, seg_label, n_keep, b):
    """seg / sem / ins of item b from the device's lab_map and tables; all zero where n_keep == 0"""
    shape = lab_map.shape[1:]
    if int(n_keep[b]) == 0:
        z = np.zeros(shape, np.int32)
        return z, z, z
    k = lab_map[b]
    sid = seg_id[b][k]
    sem = np.where(sid > 0, seg_label[b][k] + 1, 0).astype(np.int32)
    return sid.astype(np.int32), sem, sid.astype(np.int32)


def qcl_ref(p256, probs, kept_idx, acc_list, nq, b, H, W):
    """-> out [T*H*W, nq, C] float64, bound"""
    ks = acc_list[b, :nq]
    P = p256[b][:, ks].astype(F64)  # [T,nq,MS,MS]
    s, E = bilinear(P, H, W), lerp_bound(P, H, W)
    pr = probs[b, kept_idx[b, ks]].astype(F64)  # [nq,C]
    flat = lambda x: np.moveaxis(x, 1, -1).reshape(-1, nq)
    out = flat(s)[:, :, None] * pr[None]
    return out, flat(E)[:, :, None] * pr[None] + U * np.abs(out)


def lift_ref(qc, q, C, thr, num_queries, stuff_mask, variant=None):
    """qc [npix, q*C] float32 (channel-last: query-major, class-minor) -> sem [npix], ins [npix] int64, first_pix [q], q_label [q] int32.
    The winner is the smallest key = rolled class * q + query among the elements equal to the pixel's maximum (pipeline.py:141-150).
    variant "unrolled" / "lastquery": deliberately wrong"""
    npix = qc.shape[0]
    x = qc.reshape(npix, q, C)
    if variant != "unrolled":
        x = np.concatenate([x[:, :, -1:], x[:, :, :-1]], 2)  # rolled: void first
    x = np.moveaxis(x, 1, 2)  # [npix, C, q]
    if variant == "lastquery":
        x = x[:, :, ::-1]
    key = x.reshape(npix, C * q).argmax(1)  # first maximum = smallest key
    best = x.reshape(npix, C * q)[np.arange(npix), key]
    sem, qi = key // q, key % q
    if variant == "lastquery":
        qi = q - 1 - qi
    sem = np.where(best < F32(thr), 0, sem)
    ins = np.where(sem == 0, 0, qi + 1)
    first = np.full(q, 0x7fffffff, np.int32)
    for i in range(q):
        w = np.flatnonzero(ins == i + 1)
        if w.size:
            first[i] = w[0]
    qlab = np.where(first == 0x7fffffff, -1, sem[np.minimum(first, npix - 1)]).astype(np.int32)
    fused = (sem >= 1) & (sem <= 32) & (((stuff_mask >> np.clip(sem - 1, 0, 31)) & 1) == 1)
    ins = np.where(fused, num_queries + sem, ins)
    return sem.astype(np.int64), ins.astype(np.int64), first, qlab


# ---- float32 emulation of the device stage (the kernels' operation order) ------------------------------------------------------------------
def emulate_stage1(c, variant=None):
    """every buffer siu3r_panoptic_stage1 writes, computed in numpy float32 in the kernels' order; what the kernels leave unwritten holds
    the sentinel.  variant: None, or one deliberately wrong stage ("noclamp", "align", "lastmax", "gt", "f32overlap")"""
    cls, mcl = c["cls"], c["mcl"]
    B, Q, C = cls.shape
    T, MS, H, W = mcl.shape[1], c["MS"], c["H"], c["W"]
    i32 = lambda *s: np.full(s, SENT, np.int32)
    f32 = lambda *s: np.full(s, FILL, F32)
    o = dict(probs=f32(B, Q, C), scores=f32(B, Q), labels=i32(B, Q), kept_idx=i32(B, Q), n_keep=i32(B), p256=f32(B, T, Q, MS, MS),
             lab_map=i32(B, T, H, W), area=i32(B, Q), orig=i32(B, Q), seg_id=i32(B, Q), seg_label=i32(B, Q), seg_fused=i32(B, Q),
             seg_score=f32(B, Q), acc_list=i32(B, Q), n_acc=i32(B), seg=i32(B, T, H, W), sem=i32(B, T, H, W), ins=i32(B, T, H, W))
    a = cls - cls.max(-1, keepdims=True)
    e = np.exp(a.astype(F32))
    den = np.zeros((B, Q), F32)
    for ci in range(C):
        den = den + e[..., ci]
    o["probs"][:] = e / den[..., None]
    o["labels"][:] = o["probs"].argmax(-1)
    o["scores"][:] = o["probs"].max(-1)
    keep = (o["labels"] != C - 1) & (o["scores"] > F32(c["thr"]))
    o["area"][:] = 0
    o["orig"][:] = 0
    for b in range(B):
        idx = np.flatnonzero(keep[b])
        nk = o["n_keep"][b] = len(idx)
        o["kept_idx"][b, :nk] = idx
        if nk:
            sv = variant if variant in ("noclamp", "align") else None
            v = bilinear(np.moveaxis(mcl[b][..., idx], -1, 1), MS, MS, F32, sv)
            with np.errstate(over="ignore"):
                o["p256"][b, :, :nk] = F32(1) / (F32(1) + np.exp(-v))
            wv = bilinear(o["p256"][b, :, :nk], H, W, F32) * o["scores"][b, idx][None, :, None, None]
            best = (nk - 1 - wv[:, ::-1].argmax(1)) if variant == "lastmax" else wv.argmax(1)
            o["lab_map"][b] = best
            o["area"][b, :nk] = (np.arange(nk)[None, :, None, None] == best[:, None]).sum((0, 2, 3))
            o["orig"][b, :nk] = ((wv > F32(c["mask_thr"])) if variant == "gt" else (wv >= F32(c["mask_thr"]))).sum((0, 2, 3))
        seg_id, rows, acc = accept_ref(o["area"], o["orig"], o["kept_idx"], o["n_keep"], o["labels"], o["scores"], b, c["overlap"], c["fuse"],
                                       f32_compare=variant == "f32overlap")
        o["seg_id"][b] = seg_id
        for k, (lab, fu, sc) in rows.items():
            o["seg_label"][b, k], o["seg_fused"][b, k], o["seg_score"][b, k] = lab, fu, sc
        o["n_acc"][b] = len(acc)
        o["acc_list"][b, :len(acc)] = acc
        o["seg"][b], o["sem"][b], o["ins"][b] = write_ref(np.where(o["lab_map"] == SENT, 0, o["lab_map"]), o["seg_id"], np.where(o["seg_label"] == SENT, 0, o["seg_label"]), o["n_keep"], b)
    return o


def emulate_qcl(c, o, nq, b):
    ks = o["acc_list"][b, :nq]
    s = bilinear(o["p256"][b][:, ks], c["H"], c["W"], F32)
    return np.moveaxis(s, 1, -1).reshape(-1, nq)[:, :, None] * o["probs"][b, o["kept_idx"][b, ks]][None]


# ---- comparison rules (the GPU test feeds the read-back buffers, the CPU test the emulation) ----------------------------------------------
def check_class(c, o, fresh=True):
    """-> (worst ratio, undecided rows, rows).  fresh: the buffers held the sentinel before the call (what the kernels leave unwritten
    is then checked for it, here and in the other checks)"""
    r = class_ref(c["cls"], c["thr"])
    B, Q, C = c["cls"].shape
    w = _assert_within(o["probs"], r["probs"], r["bound"], "probs")
    w = max(w, _assert_within(o["scores"], r["score"], r["score_bound"], "scores"))  # (exact rows: bound 0)
    d = r["label_decided"]
    assert (o["labels"][d] == r["label"][d]).all(), "labels differ on decided rows"
    assert (o["labels"] >= 0).all() and (o["labels"] < C).all(), "a label outside [0, C)"
    assert np.take_along_axis(r["cand"], o["labels"][..., None].astype(np.int64), -1).all(), "an undecided row's label is no candidate"
    und = 0
    for b in range(B):
        nk = int(o["n_keep"][b])
        assert 0 <= nk <= Q, nk
        idx = o["kept_idx"][b, :nk]
        assert (np.diff(idx) > 0).all() and (nk == 0 or (idx[0] >= 0 and idx[-1] < Q)), f"item {b}: kept_idx is not an ascending compaction"
        assert not fresh or (o["kept_idx"][b, nk:] == SENT).all(), f"item {b}: kept_idx written behind n_keep"
        got = np.zeros(Q, bool)
        got[idx] = True
        kd = r["keep_decided"][b]
        assert (got[kd] == r["keep"][b][kd]).all(), f"item {b}: keep differs on decided rows {np.flatnonzero(got != r['keep'][b])[:8]}"
        und += int((~kd).sum())
    return w, und + int((~d & r["keep_decided"]).sum()), B * Q


def check_mask256(c, o, fresh=True):
    """-> (worst ratio, 0, elements); the planes of k >= n_keep[b] keep the sentinel"""
    ref = mask256_ref(c["mcl"], o["kept_idx"], o["n_keep"], c["MS"])
    w, n = 0.0, 0
    for b, (p, bound) in enumerate(ref):
        nk = int(o["n_keep"][b])
        w = max(w, _assert_within(o["p256"][b, :, :nk], p, bound, f"p256 item {b}"))
        assert not fresh or (o["p256"][b, :, nk:].view(np.int32) == FILL.view(np.int32)).all(), f"item {b}: a plane behind n_keep was written"
        n += p.size
    return w, 0, n


def check_argmax(c, o, fresh=True):
    """-> (0, undecided pixels + pairs, pixels + pairs)"""
    B, Q = o["area"].shape
    und = tot = 0
    for b in range(B):
        nk = int(o["n_keep"][b])
        assert (o["area"][b, nk:] == 0).all() and (o["orig"][b, nk:] == 0).all(), f"item {b}: counters behind n_keep are not zero"
        if nk == 0:
            assert not fresh or (o["lab_map"][b] == SENT).all(), f"item {b}: lab_map written although nothing is kept"
            continue
        r = argmax_ref(o["p256"], o["scores"], o["kept_idx"], o["n_keep"], b, c["H"], c["W"], c["mask_thr"])
        lab = o["lab_map"][b]
        assert (lab >= 0).all() and (lab < nk).all(), f"item {b}: lab_map outside [0, n_keep)"
        assert (lab[r["decided"]] == r["best"][r["decided"]]).all(), f"item {b}: lab_map differs on {(lab != r['best'])[r['decided']].sum()} decided pixels"
        assert np.take_along_axis(r["cand"], lab[:, None].astype(np.int64), 1).all(), f"item {b}: an undecided pixel holds no candidate"
        for name in ("area", "orig"):
            g = o[name][b, :nk]
            assert (g >= r[name + "_lo"]).all() and (g <= r[name + "_hi"]).all(), f"item {b}: {name} {g.tolist()} outside [{r[name + '_lo'].tolist()}, {r[name + '_hi'].tolist()}]"
        assert o["area"][b, :nk].sum() == r["npix"], "the areas do not sum to the pixel count"
        und += int((~r["decided"]).sum()) + r["undecided_pairs"]
        tot += r["npix"] + r["pairs"]
    return 0.0, und, tot


def check_accept(c, o, fresh=True):
    B, Q = o["area"].shape
    for b in range(B):
        seg_id, rows, acc = accept_ref(o["area"], o["orig"], o["kept_idx"], o["n_keep"], o["labels"], o["scores"], b, c["overlap"], c["fuse"])
        assert np.array_equal(o["seg_id"][b], seg_id), f"item {b}: seg_id {o['seg_id'][b].tolist()} != {seg_id.tolist()}"
        assert int(o["n_acc"][b]) == len(acc) and o["acc_list"][b, :len(acc)].tolist() == acc, f"item {b}: accepted {o['acc_list'][b].tolist()} != {acc}"
        assert not fresh or (o["acc_list"][b, len(acc):] == SENT).all(), f"item {b}: acc_list written behind n_acc"
        for k in range(Q):
            if k in rows:
                lab, fu, sc = rows[k]
                assert (int(o["seg_label"][b, k]), int(o["seg_fused"][b, k])) == (lab, fu) and o["seg_score"][b, k].view(np.int32) == sc.view(np.int32), (b, k)
            elif fresh:
                assert o["seg_label"][b, k] == SENT and o["seg_fused"][b, k] == SENT and o["seg_score"][b, k].view(np.int32) == FILL.view(np.int32), f"item {b}: table row {k} of a rejected slot was written"
    return 0.0, 0, B * Q


def check_write(c, o, fresh=True):
    B = o["seg"].shape[0]
    for b in range(B):
        lab = np.where(o["n_keep"].reshape((-1,) + (1,) * (o["lab_map"].ndim - 1)) > 0, o["lab_map"], 0)  # (an empty item's map is never read)
        seg, sem, ins = write_ref(lab, o["seg_id"], o["seg_label"], o["n_keep"], b)  # (a rejected slot's label is masked by its id 0)
        assert np.array_equal(o["seg"][b], seg) and np.array_equal(o["sem"][b], sem) and np.array_equal(o["ins"][b], ins), f"item {b}: seg / sem / ins differ"
    return 0.0, 0, int(o["seg"].size)


def check_qcl(c, o, nq, b, out):
    ref, bound = qcl_ref(o["p256"], o["probs"], o["kept_idx"], o["acc_list"], nq, b, c["H"], c["W"])
    return _assert_within(out.reshape(ref.shape), ref, bound, f"qcl item {b} nq {nq}"), 0, ref.size


def check_lift(c, sem, ins, first, qlab, variant=None):
    r = lift_ref(c["qc"], c["q"], c["C"], c["thr"], c["num_queries"], c["stuff_mask"])
    for name, g, e in zip(("sem_id", "ins_id", "first_pix", "q_label"), (sem, ins, first, qlab), r):
        assert np.array_equal(np.asarray(g).reshape(-1), e), f"lift {c['name']}: {name} differs at {np.flatnonzero(np.asarray(g).reshape(-1) != e)[:8]}"


STAGE_CHECKS = (("class", check_class), ("mask256", check_mask256), ("argmax", check_argmax), ("accept", check_accept), ("write", check_write))


def qcl_runs(c, o):
    """the (b, nq) pairs of a case: nq in c["nqs"] that the item accepted, every item"""
    return [(b, nq) for b in range(o["n_acc"].shape[0]) for nq in c["nqs"] if nq <= int(o["n_acc"][b])]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _smooth(rng, shape, h, w, amp, coarse=4):
    """smooth random planes [..., h, w]: coarse normals, bilinearly enlarged"""
    lo = rng.standard_normal(shape + (max(h // coarse, 2), max(w // coarse, 2)))
    return (bilinear(lo, h, w) * amp).astype(F32)


def _cell_masks(rng, B, Q, T, h, w, gy, gx):
    """smooth planes below 0.5 almost everywhere, + every query confident in its own cell of a gy x gx grid (so that segments are
    accepted), the smooth part deciding the borders"""
    m = _smooth(rng, (B, Q, T), h, w, 1.5, coarse=2) - 4.0
    ch, cw = h // gy, w // gx
    for q in range(Q):
        cy, cx = (q // gx) % gy, q % gx
        m[:, q, :, cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw] += 9.0
    return m


def _void(B, Q, C):
    cls = np.full((B, Q, C), -4.0, F32)
    cls[:, :, C - 1] = 4.0
    return cls


def _onehot(cls, b, q, c, hi=6.0, lo=-4.0):
    cls[b, q] = lo
    cls[b, q, c] = hi


def _finish(name, cls, msk, MS, H, W, thr=0.5, mask_thr=0.5, overlap=0.8, fuse=(0, 1), nqs=(1, 2, 3, 7)):
    msk = np.ascontiguousarray(msk, F32)  # [B,Q,T,IH,IW], the oracle's layout
    return dict(name=name, cls=np.ascontiguousarray(cls, F32), msk=msk, mcl=np.ascontiguousarray(np.transpose(msk, (0, 2, 3, 4, 1))), MS=MS, H=H, W=W,
                thr=thr, mask_thr=mask_thr, overlap=overlap, fuse=tuple(fuse), nqs=tuple(nqs))


def _accept_case(name, S):
    """identity sizes S x S: pixel counts set one by one on the flat pixel index (see ACCEPT_EXPECT)"""
    Q, C, N = 16, 21, S * S
    cls = _void(1, Q, C)
    klass = [0, 0, 4, 0, 5, 6, 7, 1, 8, 1, 9]
    for k, cl in enumerate(klass):
        _onehot(cls, 0, k, cl, hi=7.0)
    m = np.full((Q, N), -8.0, F32)
    Z = N - N // 4
    m[0, :Z] = -0.2                      # k0 stuff 0: wins everything nobody claims, never reaches 0.5: area > 0, orig == 0, rejected
    m[1, 0:5] = 4.0                      # k1 stuff 0: 5 px, 1 stolen: 4 / 5 == fp32(0.8) in float32: accepted
    m[2, 10:510] = 4.0                   # k2 thing 4: 500 px, 100 stolen: 400 / 500: accepted
    m[3, 520:540] = 4.0                  # k3 stuff 0 again (a thing between): ratio 1, fused into k1's id
    m[4, 550:555] = 4.0                  # k4 thing 5: 5 px, 2 stolen: 3 / 5: rejected
    m[5, Z:] = -0.5                      # k5 thing 6: wins the last quarter below 0.5: area > 0, orig == 0
    for a, e in ((4, 5), (410, 510), (553, 555), (600, 610)):
        m[6, a:e] = 8.0                  # k6 thing 7: the stealer
    m[7, 620:640] = 4.0                  # k7 stuff 1
    m[8, 650:670] = 4.0                  # k8 thing 8
    m[9, 680:700] = 4.0                  # k9 stuff 1 again: fused into k7's id
    m[10, 600:610] = 4.0                 # k10 thing 9: wholly under the stealer: orig 10, area 0
    return _finish(name, cls, m.reshape(1, Q, 1, S, S), S, S, S, nqs=(1, 2, 3, 7))


# (k, area, orig) of the accept cases and the table they must produce: (k, id, label, fused)
ACCEPT_COUNTS = {1: (4, 5), 2: (400, 500), 3: (20, 20), 4: (3, 5), 6: (113, 113), 7: (20, 20), 8: (20, 20), 9: (20, 20), 10: (0, 10)}
ACCEPT_EXPECT = [(1, 1, 0, 1), (2, 2, 4, 0), (3, 1, 0, 1), (6, 3, 7, 0), (7, 4, 1, 1), (8, 5, 8, 0), (9, 4, 1, 1)]


def _network_like(Q, T, h, w, C, kept, seed=0):
    """the statistics of the network's own output (tests/test_postprocess_gpu.py::_network_like_logits) at another size"""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(1, Q, C, generator=g)
    cls[:, :, C - 1] += 9.0
    lab = [1, 1, 0, 5, 12, 19, 13, 1, 10, 3, 19, 7, 4, 15][:kept]
    for i, c in enumerate(lab):
        cls[0, (7 * i + 2) % Q, c] += 14.0
    coarse = torch.randn(1 * Q * T, 1, max(h // 8, 2), max(w // 8, 2), generator=g)
    msk = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False).view(1, Q, T, h, w) * 2.2 - 2.8
    return cls.numpy(), (msk + 0.05 * torch.randn(1, Q, T, h, w, generator=g)).numpy()


STAGE1_CASES = ("q1_c2", "q63_c2_b3", "q64_c33", "q65_c64", "tiled128", "net256", "down256", "identity16", "accept32", "accept256")


@functools.lru_cache(maxsize=None)
def stage1_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "q1_c2":  # Q = 1, C = 2, one 1 x 1 logit, target 1 x 1: one thread of every kernel works
        return _finish(name, np.array([[[3.0, -3.0]]], F32), np.full((1, 1, 1, 1, 1), 2.0, F32), 16, 1, 1, fuse=(0,))
    if name == "q63_c2_b3":  # B = 3: a mixed item, an item that keeps nothing (all void), an item that keeps all 63
        B, Q, C, T = 3, 63, 2, 2
        cls = np.zeros((B, Q, C), F32)
        for q in range(Q):
            cls[0, q] = (2.0 + 0.01 * q, -2.0) if q % 3 == 0 else (-3.0, 3.0)
            cls[1, q] = (-3.0 - 0.1 * q, 3.0)
            cls[2, q] = (1.0 + 0.05 * q, -1.0)
        cls[0, 1] = (1.0, 1.0)      # two equal top logits: score exactly 0.5, NOT > 0.5: dropped; label 0 (the first)
        cls[0, 2] = (80.0, -80.0)   # exact row, score 1.0, kept
        cls[0, 4] = (-80.0, 80.0)   # exact row, void
        return _finish(name, cls, _cell_masks(rng, B, Q, T, 7, 9, 7, 9), 24, 37, 53, fuse=(0,))
    if name == "q64_c33":  # every query kept (n_keep = 64 = Q), T = 3, non-square logits, ragged target
        B, Q, C, T = 1, 64, 33, 3
        cls = _void(B, Q, C)
        for q in range(Q):
            _onehot(cls, 0, q, q % 32, hi=5.0 + 0.03 * q)
        cls[0, 7] = -6.0
        cls[0, 7, 3] = cls[0, 7, 9] = 6.0  # equal top logits between two non-void classes: label 3, score just below 0.5 (thr 0.3: kept)
        _onehot(cls, 0, 5, 31, hi=80.0, lo=-80.0)
        return _finish(name, cls, _cell_masks(rng, B, Q, T, 24, 40, 8, 8), 40, 50, 70, thr=0.3)
    if name == "q65_c64":  # n_keep = 65, C = 64, kept classes >= 32 (never fused, never in the stuff memory), up in y and down in x
        B, Q, C, T = 1, 65, 64, 1
        cls = _void(B, Q, C)
        for q in range(Q):
            _onehot(cls, 0, q, (q * 5) % 63, hi=7.0 + 0.02 * q)
        return _finish(name, cls, _cell_masks(rng, B, Q, T, 32, 32, 8, 8), 32, 300, 40, fuse=(0, 1, 5, 31))
    if name == "tiled128":  # n_keep = 128: the two frames are cut into 128 cells of 4 x 4, each query +6 in its own cell and -6 elsewhere
        B, Q, C, T, S = 1, 128, 21, 2, 32
        cls = _void(B, Q, C)
        msk = np.full((B, Q, T, S, S), -6.0, F32)
        for q in range(Q):
            _onehot(cls, 0, q, q % 20, hi=5.0 + 0.02 * q)
            t, cy, cx = q // 64, (q % 64) // 8, q % 8
            msk[0, q, t, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] = 6.0
        return _finish(name, cls, msk, S, S, S)
    if name == "net256":  # the shipped configuration: Q = 100, C = 21, 32 x 32 logits -> 256 x 256 -> 64 x 64
        cls, msk = _network_like(100, 2, 32, 32, 21, 14)
        return _finish(name, cls, msk, 256, 64, 64)
    if name == "down256":  # logits larger than the mask size (300 x 260 -> 256 x 256: downsampling, non-integer ratios), identity target
        cls, msk = _network_like(12, 1, 300, 260, 21, 6, seed=1)
        return _finish(name, cls, msk, 256, 256, 256)
    if name == "identity16":  # logits, mask and target all 16 x 16: wv == mask_thr exactly, bit-identical kept queries, a low-score row
        B, Q, C, T, S = 1, 6, 21, 1, 16
        cls = _void(B, Q, C)
        msk = np.full((B, Q, T, S, S), -9.0, F32)
        for q in (0, 1):
            _onehot(cls, 0, q, 2, hi=80.0, lo=-80.0)   # score 1.0
            msk[0, q, 0, :, :8] = 0.0                  # sigmoid(0) = 0.5 = wv: counted by >=
        _onehot(cls, 0, 2, 3, hi=5.0)
        msk[0, 2, 0, :8, 8:] = 3.0
        for q in (3, 4):
            _onehot(cls, 0, q, 4, hi=4.0)
            msk[0, q, 0, 8:, 8:] = 5.0
        cls[0, 5] = -4.0
        cls[0, 5, 7] = -3.5                            # label 7 with a score far below the threshold
        return _finish(name, cls, msk, S, S, S)
    if name == "accept32":
        return _accept_case(name, 32)
    if name == "accept256":
        return _accept_case(name, 256)
    raise KeyError(name)


def rolled(c, shift=1):
    """the same case with its batch items rolled: other inputs of the same shape (the second call on the same buffers)"""
    d = dict(c)
    for k in ("cls", "msk", "mcl"):
        d[k] = np.ascontiguousarray(np.roll(c[k], shift, 0))
    d["name"] = c["name"] + "_rolled"
    return d


# (q, C, V, H, W): q * C in {2, 63, 64, 65, 126, 2100, 6400}, V * H * W in {1, 63, 64, 65, 480, 4097}
LIFT_CASES = {"qc2_p1": (1, 2, 1, 1, 1), "qc63_p63": (3, 21, 1, 7, 9), "qc64_p64": (32, 2, 1, 8, 8), "qc65_p65": (5, 13, 1, 5, 13),
              "qc126_p480": (6, 21, 2, 12, 20), "qc2100_p4097": (100, 21, 1, 17, 241), "qc6400_p65": (100, 64, 1, 5, 13)}


@functools.lru_cache(maxsize=None)
def lift_case(name):
    """values from a grid of L = 2^k >= q C / 4 levels (the maximum of a pixel is attained about four times: exact ties across queries
    and across classes everywhere), then crafted pixels"""
    q, C, V, H, W = LIFT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    npix = V * H * W
    thr = F32(0.3)
    L = 8
    while L < q * C // 4:
        L *= 2
    x = (rng.integers(0, L, (npix, q, C)) / L).astype(F32)
    below = np.nextafter(thr, F32(0))
    crafted = {}
    owner = None
    if q >= 5 and npix > 64:
        owner = q - 2   # owns exactly one pixel: the last one, in the last, partial wave; nothing elsewhere (its values are 0)
        x[:, owner, :] = 0.0
        x[npix - 1] = 0.0
        x[npix - 1, owner, 0] = 1.0
        x[:, q - 3, :] = 0.0  # a query that owns nothing
    qm, cq = min(1, q - 1), min(2, C - 2)  # (classes 0 and 1 are stuff: their instance id hides the query)
    if npix >= 63:
        x[0] = 0.125
        x[0, q - 1, C - 1] = x[0, 0, 0] = 0.875          # void (rolled class 0) ties class 0: void wins, sem 0, ins 0
        x[1] = 0.0
        x[1, q - 1, cq] = x[1, 0, cq] = 0.5   # the same class at the first and the last query: the first wins
        x[2] = 0.0
        x[2, 0, C - 2] = x[2, q - 1, cq] = 0.5            # two classes: the lower rolled class wins although its query is the last
        x[3] = np.minimum(x[3], below)
        x[3, qm, cq] = thr                            # maximum == threshold: kept (not <)
        x[4] = np.minimum(x[4], below)                   # maximum one ulp below the threshold: sem 0
        x[4, qm, cq] = below
        crafted = dict(void_tie=0, query_tie=1, class_tie=2, at_thr=3, below_thr=4)
    stuff_mask = 0b11 if C > 2 else 0  # (C = 2: the one class stays a thing, so that the instance ids show the winning query)
    if C == 64:  # sem 1 and 32 fuse (bits 0 and 31), sem 33 cannot
        stuff_mask = (1 << 0) | (1 << 31)
        for i, cl in enumerate((0, 31, 32)):
            x[10 + i] = 0.0
            x[10 + i, 3 + i, cl] = 1.0
        crafted.update(stuff1=10, stuff32=11, unfusable33=12)
    return dict(name=name, q=q, C=C, V=V, H=H, W=W, qc=np.ascontiguousarray(x.reshape(npix, q * C)), thr=float(thr), num_queries=100,
                stuff_mask=stuff_mask, crafted=crafted, owner=owner)
