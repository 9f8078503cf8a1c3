"""Float64 restatements of the stages of the two rasterizer backward passes (siu3r_amd/csrc/raster_bwd.hip, raster_bwd_k3.hip,
raster_bwd_shared.h), written from the kernels' header comments and include/siu3r_hip.h, with the per-element comparison and the
crafted cases that tests/test_raster_bwd_stages_ref.py (CPU) and tests/test_raster_bwd_stages_gpu.py (GPU) share.

  project64 / project_bwd64   the per-(view, Gaussian) record (mx, my, conic a, b, c, opacity, r, g, b, depth) of either camera mode as
                              a differentiable function, and grad [V,G,10] pulled back through it by float64 AUTOGRAD (the kernels' chain
                              is hand derived: it is checked against differentiation, not against a second derivation)
  composite_bwd64             one view's composite backward from the fp32 records, the per-tile lists and the upstream gradients, with
                              the decision margin of every pixel; walk32_agrees compares it with the same walk in emulated float32
  quat_scale_cov6_bwd64, sh_eval_bwd64   the viewer helpers (dense_gsplat64.quat_scale_to_cov6 / sh_eval under autograd)
  rows_reduce64               the partial-row sums
  assert_elems_close          |got - ref| <= bound * S, element by element

SCALES.  Every reference value carries S, the magnitude its rounding errors are proportional to: the sum of the absolute values of the
terms it is a sum of.
  projection   one term per (view, record slot).  A vector-valued term (means, covariance, pose blocks) goes through rotations, so all
               components of a Gaussian share the Euclidean norm of the term.  NOT the plain sum: the slots whose chain subtracts nearly
               equal numbers are weighted by that subtraction's condition, computed in float64 per (view, Gaussian): k_pt = (sum_j |W_ij
               m_j| + |t_i|) / |z| of the camera-space point (mean and depth slots), and for the conic slots also k_cov = sum |t_i
               Sigma_ij t_j| / (t Sigma t) and k_det = (c00 c11 + c01^2) / det.  On the crafted cases the product is 2 in the median and
               at most 12.7 (the coverage test caps it at 16), so the effective bound on the plain sum is 164 u to 2100 u.  SH colours:
               |upstream| * B_k evaluated with absolute monomials (sh_basis_abs), and for the direction gradient the same with its
               partial derivatives.
  composite    the plain sum: one term per pixel that blends the entry, in its absolute form (every product with |.|, the part behind
               an entry as the sum over ALL blended entries of the pixel, because the kernels form it as total - prefix).  The error of
               the alpha / transmittance chain is NOT in S: it is the explicit allowance `chain` (below).
  pose rows    the sum over the Gaussians of their scales.

BOUNDS (u = 2^-24, one fp32 rounding; device reciprocal and sqrtf: 1 ulp = 2 u, the documented bounds of v_rcp_f32 / v_sqrt_f32 behind
1.0f / x and sqrtf in HIP's default mode).
  PROJ_BOUND = 164 u.  Longest path conic gradient -> mean: the forward chain again (point 6, 1 / z, x / z, c x z, J 3, M = J W 3,
      Sigma M^T 5, c00 6, det 3: 30 roundings), the backward (1 / det, conic 1, d det 6, d00 3, dt 4, dj 5, d ctx 4, d rz 8, d tz 7, W^T
      dp 6, sum over V <= 3 views: 48); every sum's other inputs are of the same depth, counted once more: 128 in all.  Reciprocals: 1 / z
      enters up to 8 times, 1 / det 3, 1 / (hw + 1e-7) 2, 1 / |m - campos| 2, 1 / det W 1: 16 uses of 2 u.  sqrtf once, used twice: 4 u.
  SH_BOUND = 72 u.  view direction 9 + 2 u (sqrt) + 2 u (reciprocal), the dual-number basis 8, the 3-channel sum 3, 25 coefficients
      accumulated into the direction gradient, its projection off d 5 and the scale by 1 / |.| 3 (+ 2 u, twice): 53 + 8, rounded up.
  QUAT_BOUND = 64 u.  |q| 4 + sqrt / reciprocal 4 u, R 5, M 1, d M 6, d R 1, the eight-term quaternion sums 10, the projection off q 7 + 3,
      scale by 1 / |q| 1 (+ 2 u): 38 + 8, with fan-in 64.  Its S is norm-wise (the normalisation projects a raw gradient of the size
      |g_cov| |M|^2 / |q| onto q's tangent space, which can leave nothing: isotropic scales): S_q = 8 sum_k c_k |g_k| max(s)^2 / |q|, S_s
      = 2 sum_k c_k |g_k| max(s) (c_k = 1 on the diagonal, 2 off it).
  ROWS: the reduction's fixed order, ceil(n / 256) + 9 (six wave levels, three LDS adds).
  COMPOSITE: |got - ref| <= (COMP_OPS + C + n_add[g]) u S + chain, per element.
      COMP_OPS = 64, the roundings of one pixel term that do not depend on the pixel's history: dx, dy 2, g . c and the part behind 6 + 6
      (plus one per channel of the sums over C channels: + C), 1 / (1 - a) 1 + 2 u, d alpha 3, the record term 5, the wave sum 6, the LDS
      slot 4: 35 + 2, rounded up to 64.  The float atomics add in any order: + (number of addends of the element) u.
      chain[g, k] = the sum over the element's pixel terms of |term part| x (derived relative error of that part), with the errors of the
      alpha / transmittance chain below, per (entry j, pixel):
        weight w = a T (colour, depth and feature terms)        e_w(j) = e_a(j) + e_T in front of j
        d loss / d alpha = T (g . c) - behind / (1 - a):  front part   e_T in front of j
                                                          behind part  (sum_k |q_k| e_w(k) over ALL blended k of the pixel, since behind =
                                                                       total - prefix, + the background's e_T) / (1 - a), and e_a a / (1 - a)
                                                                       of 1 - a itself
        the factors exp / a of the opacity, conic and mean terms       e_a(j) once more
      The effective bound (tolerance / S) on the crafted cases: 150 u .. 730 u in the median, up to 13000 u (8e-4) for a Gaussian whose
      pixels lie behind alphas of 0.99 (1 / (1 - a) = 100, twice); profiles/raster_bwd_parity.json records it per comparison.
  EXP_DET_REL: exp_det_sel (siu3r_amd/csrc/raster_shared.h) against exp over [-87, 0], measured with the float32 restatement below
      (test_raster_bwd_stages_ref.py::test_exp_det_sel_constant).  The error grows with the argument (x log2 e is rounded before the
      split into integer and fraction: 3.9e-6 at -87), so the constant is the largest error per (1 + |x|) and the chain uses
      EXP_DET_REL (1 + sigma).

THE PIXEL CHAIN AND THE DECISION MARGIN.  Per entry j of a pixel's walk, with M_j = 0.5 (|a| dx^2 + |c| dy^2) + |b dx dy|:
  sigma          absolute error 6 u M_j (a term passes two products and two fused adds, and dx or dy, rounded once, enters it twice)
  alpha          relative error e_a(j) = 6 u M_j + EXP_DET_REL (1 + sigma_j) + u (the product with the opacity)
  transmittance  T' = fma(-T, a, T): one rounding (u) plus e_a a / (1 - a) from alpha, so after the blended entries B:
                 e_T = sum_{i in B} (u + e_a(i) a_i / (1 - a_i))
The margin of a pixel is the smallest distance of a compared quantity to its threshold IN UNITS OF THAT QUANTITY'S DERIVED ERROR: |sigma| /
(6 u M), |alpha - alpha_min| / (alpha_min e_a), |opacity exp - alpha_max| / (alpha_max e_a), |T' - t_min| / (t_min (e_T + step)), over the
entries the pixel reaches.  MARGIN = 4 is the safety factor on the derived error; the GPU tests zero the upstream gradient of the pixels
below it, the CPU module shows that above it the float32 walk takes the float64 branch everywhere and that at most 1 % of a case's
pixels lie below it.

Not a test module."""
import functools
import math

import numpy as np
import torch

import dense_gsplat64 as DG
import dense_raster64 as DR
import raster_stages_ref as RS

U24 = 2.0 ** -24
PROJ_BOUND = 164 * U24
SH_BOUND = 72 * U24
QUAT_BOUND = 64 * U24
COMP_OPS = 64
EXP_DET_MEASURED = 7.2e-8  # the largest relative error of exp_det_sel32 against exp over [-87, 0], per (1 + |x|) (test_exp_det_sel_constant)
EXP_DET_REL = EXP_DET_MEASURED
MARGIN = 4.0
ZERO_SHARE_CAP = 0.01
TILE = DR.TILE
MX, MY, CA, CB, CC, OP, RR, GG, BB, ZZ = range(10)
DD = torch.float64


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def _t(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).double().cpu()


def tolerance(ref, S, bound, extra=None):
    """bound * S (+ extra), in the shape of ref"""
    ref, S = _t(ref), _t(S)
    lim = (torch.as_tensor(bound, dtype=DD) * (S.expand_as(ref) if S.shape != ref.shape else S)).expand_as(ref)
    return lim if extra is None else lim + _t(extra).expand_as(ref)


def worst_ratio(got, ref, S, bound, extra=None):
    """-> (max |got - ref| / (bound S + extra), flat index); an element whose tolerance is 0 must be exactly ref"""
    got, ref = _t(got), _t(ref)
    lim = tolerance(ref, S, bound, extra)
    d = (got - ref).abs()
    r = torch.where(lim > 0, d / lim.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    r = torch.where(torch.isnan(got), torch.full_like(r, math.inf), r)
    i = int(r.reshape(-1).argmax()) if r.numel() else 0
    return (float(r.reshape(-1)[i]) if r.numel() else 0.0), i


def observed(got, ref, S):
    """max |got - ref| / S over the elements with S > 0 (what profiles/raster_bwd_parity.json records)"""
    got, ref, S = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).double().cpu() for t in (got, ref, S))
    S = S.expand_as(ref)
    ok = S > 0
    return float(((got - ref).abs()[ok] / S[ok]).max()) if ok.any() else 0.0


def effective_bound(ref, S, bound, extra=None):
    """the tolerance as a multiple of S: (median, max) of (bound S + extra) / S over the elements with S > 0"""
    lim, S = tolerance(ref, S, bound, extra), _t(S).expand_as(_t(ref))
    r = (lim / S.clamp_min(1e-300))[S > 0]
    return (float(r.median()), float(r.max())) if r.numel() else (0.0, 0.0)


def assert_elems_close(got, ref, S, bound, name="", quiet=False, extra=None):
    """|got - ref| <= bound * S (+ extra) for every element (bound a number or an array that broadcasts; extra: an absolute allowance of
    ref's shape, the composite stages' chain error); names the worst one; returns its ratio"""
    w, i = worst_ratio(got, ref, S, bound, extra)
    if not quiet:
        print(f"[parity] {name}: worst element {i}: {w:.3f} of the bound; max |got - ref| / S = {observed(got, ref, S):.3e}")
    assert w <= 1.0, f"{name}: element {i}: |got - ref| is {w:.2f} x the bound"
    return w


def rejects(got, ref, S, bound, extra=None):
    return worst_ratio(got, ref, S, bound, extra)[0] > 1.0


# ---- projection ------------------------------------------------------------------------------------------------------------------------
def _hat(xi):
    z = torch.zeros_like(xi[..., 0])
    r, t = xi[..., :3], xi[..., 3:]
    return torch.stack([torch.stack([z, -t[..., 2], t[..., 1], r[..., 0]], -1), torch.stack([t[..., 2], z, -t[..., 0], r[..., 1]], -1),
                        torch.stack([-t[..., 1], t[..., 0], z, r[..., 2]], -1), torch.stack([z, z, z, z], -1)], -2)


def lens_limits(mode, cam):
    """-> fx, fy, (limx_neg, limx_pos, limy_neg, limy_pos), blur as siu3r_amd/csrc/raster_shared.h lens_k2 / lens_k3 state them"""
    W, H = cam.width, cam.height
    if mode == 0:
        fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
        return fx, fy, (1.3 * cam.tanfovx, 1.3 * cam.tanfovx, 1.3 * cam.tanfovy, 1.3 * cam.tanfovy), cam.dilation
    fx, fy, cx, cy = cam.fx, cam.fy, cam.cx, cam.cy
    tfx, tfy = 0.5 * W / fx, 0.5 * H / fy
    return fx, fy, (cx / fx + 0.3 * tfx, (W - cx) / fx + 0.3 * tfx, cy / fy + 0.3 * tfy, (H - cy) / fy + 0.3 * tfy), cam.eps2d


def sh_basis_abs(d, deg, band4):
    """DR.sh_basis with every monomial taken absolutely (|constants|, |x|, |y|, |z|, sums for differences): the magnitude of the terms a
    basis value is a sum of; its partial derivatives are those of the terms of the gradient"""
    x, y, z = d.abs().unbind(-1)
    c1, c2, c3, c4 = DR.SH_C1, [abs(c) for c in DR.SH_C2], [abs(c) for c in DR.SH_C3], [abs(c) for c in DR.SH_C4]
    b = [torch.full_like(x, DR.SH_C0)]
    if deg > 0:
        b += [c1 * y, c1 * z, c1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [c2[0] * xy, c2[1] * yz, c2[2] * (2 * zz + xx + yy), c2[3] * xz, c2[4] * (xx + yy)]
        if deg > 2:
            b += [c3[0] * y * (3 * xx + yy), c3[1] * xy * z, c3[2] * y * (4 * zz + xx + yy), c3[3] * z * (2 * zz + 3 * xx + 3 * yy),
                  c3[4] * x * (4 * zz + xx + yy), c3[5] * z * (xx + yy), c3[6] * x * (xx + 3 * yy)]
            if deg > 3 and band4:
                b += [c4[0] * xy * (xx + yy), c4[1] * yz * (3 * xx + yy), c4[2] * xy * (7 * zz + 1), c4[3] * yz * (7 * zz + 3),
                      c4[4] * (zz * (35 * zz + 30) + 3), c4[5] * xz * (7 * zz + 3), c4[6] * (xx + yy) * (7 * zz + 1),
                      c4[7] * xz * (xx + 3 * yy), c4[8] * (xx * (xx + 3 * yy) + yy * (3 * xx + yy))]
    return torch.stack(b, -1)


def _abs_gradient(Ba, dn):
    """sum over x, y, z of the absolute partial derivatives of every column of sh_basis_abs -> [G, K] (column 0 is a constant)"""
    cols = [torch.autograd.grad(Ba[:, k].sum(), dn, retain_graph=True)[0].abs().sum(-1) if Ba[:, k].requires_grad else torch.zeros(Ba.shape[0], dtype=DD)
            for k in range(Ba.shape[1])]
    return torch.stack(cols, -1)


def _basis(d, deg, band4, mutate):
    B = DR.sh_basis(d, deg, band4)
    sc = mutate.get("sh_scale")
    if sc:  # a wrong basis constant: column k times (1 + delta)
        f = torch.ones(B.shape[-1], dtype=DD)
        for k, delta in sc.items():
            if k < B.shape[-1]:
                f[k] = 1.0 + delta
        B = B * f
    return B


def _through(x, clamped, on):
    """the clamp's value with the gradient of the unclamped input (the straight-through edit of a wrong backward)"""
    return x + (clamped - x).detach() if on else clamped


def project64(mode, cam, means, cov6, opac, colors, pose=None, mutate=None):
    """The record of one view as a float64 function.  means [G,3], cov6 [G,6], opac [G]; colors: mode 0 SH [G,n,3] interleaved (or with
    cam.sh_degree < 0 the colours [G,1,3]), mode 1 the record colours [G,3] or None.  pose: None, or mode 0 xi = (rho, theta) [6] / [G,6]
    (left perturbation, the full projection moving with it), mode 1 the world->camera matrix [4,4] / [G,4,4]; a per-Gaussian pose gives the
    per-Gaussian pose terms.  mutate: the wrong answers of the rejection tests (clamp_through, colour_through, swap_xy, swap_posneg,
    sh_scale).  -> rec [G,10], aux (clamp inputs, conditions)"""
    mutate = mutate or {}
    W, H = cam.width, cam.height
    m, c6, G = means.to(DD), cov6.to(DD), means.shape[0]
    w2c0 = DG.cam_w2c(cam)
    if mode == 0:
        P0 = torch.tensor(list(cam.proj), dtype=DD).reshape(4, 4)
        if pose is None:
            w2c, P = w2c0.expand(G, 4, 4), P0.expand(G, 4, 4)
        else:
            xi = pose.to(DD)
            E = torch.linalg.matrix_exp(_hat(xi.expand(G, 6) if xi.dim() == 1 else xi))
            w2c = E @ w2c0
            P = P0 @ torch.linalg.inv(w2c0) @ E @ w2c0
    else:
        w2c = (w2c0 if pose is None else pose.to(DD))
        w2c = w2c.expand(G, 4, 4) if w2c.dim() == 2 else w2c
    R, t = w2c[:, :3, :3], w2c[:, :3, 3]
    pc = torch.einsum("gij,gj->gi", R, m) + t
    tx, ty, tz = pc.unbind(-1)
    fx, fy, lim, blur = lens_limits(mode, cam)
    xn, xp, yn, yp = lim
    if mutate.get("swap_xy"):
        xn, xp, yn, yp = yn, yp, xn, xp
    if mutate.get("swap_posneg"):
        xn, xp, yn, yp = xp, xn, yp, yn
    txz, tyz = tx / tz, ty / tz
    cxz = _through(txz, torch.minimum(torch.maximum(txz, torch.full_like(txz, -xn)), torch.full_like(txz, xp)), mutate.get("clamp_through"))
    cyz = _through(tyz, torch.minimum(torch.maximum(tyz, torch.full_like(tyz, -yn)), torch.full_like(tyz, yp)), mutate.get("clamp_through"))
    z0 = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, z0, -fx * cxz / tz], -1), torch.stack([z0, fy / tz, -fy * cyz / tz], -1)], -2)
    Tm = J @ R
    S3 = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], -1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], -1),
                      torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], -1)], -2)
    S2 = Tm @ S3 @ Tm.transpose(1, 2)
    c00, c01, c11 = S2[:, 0, 0] + blur, S2[:, 0, 1], S2[:, 1, 1] + blur
    det = c00 * c11 - c01 * c01
    if mode == 0:
        hom = torch.einsum("gij,gj->gi", P, torch.cat([m, torch.ones_like(m[:, :1])], -1))
        pw = 1.0 / (hom[:, 3] + 1e-7)
        mx, my = ((hom[:, 0] * pw + 1.0) * W - 1.0) * 0.5, ((hom[:, 1] * pw + 1.0) * H - 1.0) * 0.5
        if cam.sh_degree < 0:
            col = lin = colors.to(DD).reshape(-1, 3)
        else:
            d = m - torch.tensor(list(cam.campos), dtype=DD)
            d = d / d.norm(dim=-1, keepdim=True)
            B = _basis(d, cam.sh_degree, bool(cam.sh_band4), mutate)
            lin = (B[:, :, None] * colors.to(DD)[:, :B.shape[1], :]).sum(1) + 0.5
            col = _through(lin, torch.clamp(lin, min=0.0), mutate.get("colour_through"))
    else:
        mx, my = fx * txz + cam.cx, fy * tyz + cam.cy
        col = lin = colors.to(DD).reshape(-1, 3) if colors is not None else torch.zeros((G, 3), dtype=DD)
    rec = torch.stack([mx, my, c11 / det, -c01 / det, c00 / det, opac.to(DD).reshape(-1), col[:, 0], col[:, 1], col[:, 2], tz], -1)
    with torch.no_grad():
        k_pt = ((R.abs() * m.abs()[:, None, :]).sum(-1) + t.abs()).max(-1).values / tz.abs()
        Ta = Tm.abs()
        quad = torch.einsum("gai,gij,gaj->ga", Ta, S3.abs(), Ta)
        k_cov = torch.maximum(quad[:, 0] / (c00 - blur), quad[:, 1] / (c11 - blur)).clamp_min(1.0)
        k_det = (c00 * c11 + c01 * c01) / det
        aux = dict(txz=txz.detach(), tyz=tyz.detach(), cxz=cxz.detach(), cyz=cyz.detach(), lim=(xn, xp, yn, yp), lin=lin.detach(),
                   k_pt=k_pt, k_cov=k_cov, k_det=k_det, det=det.detach())
    return rec, aux


def clamp_class(aux):
    """-> int [G]: 0 none, 1 x at +lim, 2 x at -lim, 3 y at +lim, 4 y at -lim, 5 both; and the smallest relative distance of x / z, y / z
    to a limit (the float32 chain decides like float64 where it is far above 2^-24)"""
    xn, xp, yn, yp = aux["lim"]
    tx, ty = aux["txz"], aux["tyz"]
    xc = torch.where(tx > xp, 1, torch.where(tx < -xn, 2, 0))
    yc = torch.where(ty > yp, 3, torch.where(ty < -yn, 4, 0))
    cls = torch.where((xc > 0) & (yc > 0), 5, torch.maximum(xc, yc))
    dist = torch.stack([(tx - xp).abs() / xp, (tx + xn).abs() / xn, (ty - yp).abs() / yp, (ty + yn).abs() / yn]).min(0).values
    return cls, dist


def project_bwd64(mode, cams, means, cov6, opac, colors, rect, grad, mutate=None):
    """grad [V,G,10] pulled back through project64 over the (view, Gaussian) pairs whose rect [V,G,4] is non-empty.  Mode 1 has no depth
    output: slot 9 of grad is ignored.  -> dict name -> (value, S): g_means [G,3], g_cov [G,6], g_opac [G], g_colors (the shape of
    colors), g_mean2d [V,G,2] (mode 0; S = 0: a copy), pose [V,6] (mode 0) or [V,4,4] (mode 1), pose_g [V,G,6] / [V,G,4,4] (the
    per-Gaussian terms, for the partial rows) and aux per view"""
    V, G = len(cams), means.shape[0]
    grad, rect = torch.as_tensor(grad).to(DD), torch.as_tensor(rect).long()
    leaves = [means.detach().to(DD).requires_grad_(), cov6.detach().to(DD).requires_grad_(), opac.detach().to(DD).requires_grad_()]
    has_col = colors is not None
    if has_col:
        leaves.append(colors.detach().to(DD).requires_grad_())
    names = ["g_means", "g_cov", "g_opac"] + (["g_colors"] if has_col else [])
    val = {n: torch.zeros_like(l) for n, l in zip(names, leaves)}
    S = {n: torch.zeros_like(l) for n, l in zip(names, leaves)}
    pshape = (6,) if mode == 0 else (4, 4)
    pose_g, pose_gS, auxs = torch.zeros((V, G) + pshape, dtype=DD), torch.zeros((V, G) + pshape, dtype=DD), []
    for v, cam in enumerate(cams):
        live = ((rect[v, :, 2] - rect[v, :, 0]) * (rect[v, :, 3] - rect[v, :, 1]) != 0).to(DD)
        pose = (torch.zeros((G, 6), dtype=DD) if mode == 0 else DG.cam_w2c(cam).expand(G, 4, 4).clone()).requires_grad_()
        rec, aux = project64(mode, cam, leaves[0], leaves[1], leaves[2], leaves[3] if has_col else None, pose, mutate)
        auxs.append(aux)
        for k in range(10 if mode == 0 else 9):
            go = torch.zeros((G, 10), dtype=DD)
            go[:, k] = grad[v, :, k] * live
            gs = torch.autograd.grad(rec, leaves + [pose], go, retain_graph=True, allow_unused=True)
            kap = torch.ones(G, dtype=DD)
            if k in (MX, MY, ZZ):
                kap = aux["k_pt"]
            elif k in (CA, CB, CC):
                kap = aux["k_pt"] * aux["k_cov"] * aux["k_det"]
            for n, g in zip(names, gs[:-1]):
                if g is None:
                    continue
                val[n] += g
                if n in ("g_means", "g_cov"):
                    S[n] += (g.norm(dim=-1, keepdim=True) * kap[:, None]).expand_as(g)
                elif n == "g_colors" and mode == 0 and cam.sh_degree >= 0:
                    pass  # (below: the scale of an SH coefficient's term is |upstream| * |basis|, also where the value is clamped away)
                else:
                    S[n] += g.abs()
            gp = gs[-1]
            if gp is not None:
                pose_g[v] += gp
                if mode == 0:
                    pose_gS[v] += torch.cat([gp[:, :3].norm(dim=-1, keepdim=True).expand(G, 3), gp[:, 3:].norm(dim=-1, keepdim=True).expand(G, 3)], -1) * kap[:, None]
                else:
                    sR = gp[:, :3, :3].reshape(G, 9).norm(dim=-1)[:, None, None].expand(G, 3, 3)
                    sT = gp[:, :3, 3].norm(dim=-1)[:, None, None].expand(G, 3, 1)
                    pose_gS[v, :, :3] += torch.cat([sR, sT], -1) * kap[:, None, None]
        if mode == 0 and has_col and cam.sh_degree >= 0:
            with torch.no_grad():
                d = leaves[0] - torch.tensor(list(cam.campos), dtype=DD)
                inv = 1.0 / d.norm(dim=-1, keepdim=True)
                dn = (d * inv).requires_grad_()
            with torch.enable_grad():
                Ba = sh_basis_abs(dn, cam.sh_degree, bool(cam.sh_band4))
                dBa = _abs_gradient(Ba, dn)
            gcol = (grad[v, :, RR:BB + 1] * live[:, None]).abs()
            S["g_colors"][:, :Ba.shape[1], :] += Ba.detach()[:, :, None] * gcol[:, None, :]
            coef = leaves[3].detach()[:, :Ba.shape[1], :].abs()
            S["g_means"] += 2.0 * inv * (dBa[:, :, None] * coef * gcol[:, None, :]).sum((1, 2))[:, None]
    out = {n: (val[n], S[n]) for n in names}
    if mode == 0:
        live_all = ((rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1]) != 0)
        out["g_mean2d"] = (grad[..., :2] * live_all[..., None], torch.zeros((V, G, 2), dtype=DD), live_all)
    out["pose"] = (pose_g.sum(1), pose_gS.sum(1))
    out["pose_g"] = (pose_g, pose_gS)
    out["aux"] = auxs
    return out


def partial_rows64(pose_g, pose_gS, n):
    """per-Gaussian pose terms [V,G,...] -> the per-workgroup rows [ceil(G / 256), V, n] of the projection backwards (first n flat entries)"""
    V, G = pose_g.shape[:2]
    nb = -(-G // 256)
    f = lambda t: torch.stack([t[:, b * 256:(b + 1) * 256].reshape(V, min(256, G - b * 256), -1)[..., :n].sum(1) for b in range(nb)])
    return f(pose_g), f(pose_gS)


def rows_reduce64(part, n_out):
    """part [nrows, V, N] -> (out [V, n_out] with zeros past N, S, bound)"""
    part = torch.as_tensor(part).to(DD)
    nrows, V, N = part.shape
    out, S = torch.zeros((V, n_out), dtype=DD), torch.zeros((V, n_out), dtype=DD)
    out[:, :N], S[:, :N] = part.sum(0), part.abs().sum(0)
    return out, S, (-(-nrows // 256) + 9) * U24


# ---- viewer helpers --------------------------------------------------------------------------------------------------------------------
def quat_scale_cov6_bwd64(quats, scales, g_cov6):
    q, s = quats.detach().to(DD).requires_grad_(), scales.detach().to(DD).requires_grad_()
    g = torch.as_tensor(g_cov6).to(DD)
    gq, gs = torch.autograd.grad(DG.quat_scale_to_cov6(q, s), (q, s), g)
    w = (g.abs() * torch.tensor([1.0, 2.0, 2.0, 1.0, 2.0, 1.0], dtype=DD)).sum(-1, keepdim=True)
    smax = s.detach().abs().max(-1, keepdim=True).values
    return (gq, (8.0 * w * smax ** 2 / q.detach().norm(dim=-1, keepdim=True)).expand_as(gq)), (gs, (2.0 * w * smax).expand_as(gs))


def sh_eval_bwd64(means, campos, sh, degree, g_rgb, mutate=None):
    """-> (g_sh [G,K,3], S), (g_means [G,3], S), (g_campos [3], S), lin [G,3] (the colours in front of the clamp)"""
    m, cp, c = means.detach().to(DD).requires_grad_(), campos.detach().to(DD).requires_grad_(), sh.detach().to(DD).requires_grad_()
    g = torch.as_tensor(g_rgb).to(DD)
    d = m - cp
    d = d / d.norm(dim=-1, keepdim=True)
    B = _basis(d, degree, True, mutate or {})
    lin = (B[:, :, None] * c[:, :B.shape[1], :]).sum(1) + 0.5
    assert mutate or torch.equal(torch.clamp(lin, min=0.0).detach(), DG.sh_eval(m.detach(), cp.detach(), c.detach(), degree))
    gsh, gm, gc = (torch.zeros_like(x) if t is None else t  # (degree 0: no direction)
                   for t, x in zip(torch.autograd.grad(torch.clamp(lin, min=0.0), (c, m, cp), g, allow_unused=True), (c, m, cp)))
    with torch.no_grad():
        dd = m - cp
        inv = 1.0 / dd.norm(dim=-1, keepdim=True)
        dn = (dd * inv).requires_grad_()
    with torch.enable_grad():
        Ba = sh_basis_abs(dn, degree, True)
        dBa = _abs_gradient(Ba, dn)
    S_sh = torch.zeros_like(gsh)
    S_sh[:, :Ba.shape[1], :] = Ba.detach()[:, :, None] * g.abs()[:, None, :]
    S_m = (2.0 * inv * (dBa[:, :, None] * c.detach()[:, :Ba.shape[1], :].abs() * g.abs()[:, None, :]).sum((1, 2))[:, None]).expand_as(gm)
    return (gsh, S_sh), (gm, S_m), (gc, S_m.sum(0)), lin.detach()


# ---- the composite walk ----------------------------------------------------------------------------------------------------------------
def exp_det_sel32(x):
    """exp_det_sel (siu3r_amd/csrc/raster_shared.h) in numpy float32; the fused multiply-adds through float64 (the product is exact there)"""
    f32 = np.float32
    x = np.asarray(x, f32)
    y = x * f32(1.4426950408889634)
    n = np.floor(y + f32(0.5))
    f = (y - n).astype(f32)
    p = np.full_like(f, f32(1.52527338e-5))
    for c in (1.54035304e-4, 1.33335581e-3, 9.61812911e-3, 5.55041087e-2, 2.40226507e-1, 6.93147181e-1, 1.0):
        p = (p.astype(np.float64) * f.astype(np.float64) + np.float64(f32(c))).astype(f32)
    r = np.ldexp(p, n.astype(np.int32)).astype(f32)
    return np.where(x < f32(-87.0), f32(0.0), r)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _tile_pixels(cam, tile, k3):
    gw = -(-cam.width // TILE)
    tx, ty = tile % gw, tile // gw
    lx, ly = np.meshgrid(np.arange(TILE), np.arange(TILE))
    px, py = (tx * TILE + lx).reshape(-1), (ty * TILE + ly).reshape(-1)
    return px, py, (px < cam.width) & (py < cam.height), 0.5 if k3 else 0.0


def _walk(cam, r, px, py, inside, off, k3, f32, sat_le=None):
    """one tile: r [L,12] the list's records front to back -> per (entry, pixel) arrays of the walk.  f32: the kernels' operations in
    float32 (conic_sigma's fused order, exp_det_sel, fminf, fma(-T, a, T)); else float64 with exp"""
    ft = np.float32 if f32 else np.float64
    L, P = r.shape[0], px.shape[0]
    a_min, a_max, t_min = ft(np.float32(cam.alpha_min)), ft(np.float32(cam.alpha_max)), ft(np.float32(cam.t_min))
    le = k3 if sat_le is None else sat_le
    r = r.astype(ft)
    dx = r[:, 0:1] - (px.astype(ft) + ft(off))[None]
    dy = r[:, 1:2] - (py.astype(ft) + ft(off))[None]
    ca, cb, cc, op = r[:, 4:5], r[:, 5:6], r[:, 6:7], r[:, 7:8]
    if f32:
        q = _fma32(cc * dy, dy, (ca * dx) * dx)
        sigma = _fma32(cb * dx, dy, ft(0.5) * q)
        ex = exp_det_sel32(-sigma)
    else:
        sigma = 0.5 * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
        ex = np.exp(np.minimum(-sigma, 0.0))
    araw = op * ex
    a = np.minimum(a_max, araw)
    static = (sigma >= 0) & (a >= a_min) & inside[None]
    T = np.ones(P, ft)
    done = ~inside
    satd = np.zeros(P, bool)
    bl, Tb, reached, nTs = np.zeros((L, P), bool), np.ones((L, P), ft), np.zeros((L, P), bool), np.ones((L, P), ft)
    for j in range(L):
        if done.all():
            break
        reached[j] = ~done
        nT = _fma32(-T, a[j], T) if f32 else T * (1.0 - a[j])
        reach = ~done & static[j]
        sat = reach & ((nT <= t_min) if le else (nT < t_min))
        done, satd = done | sat, satd | sat
        bl[j] = reach & ~sat
        Tb[j], nTs[j] = T, nT
        T = np.where(bl[j], nT, T)
    return dict(dx=dx, dy=dy, sigma=sigma, ex=ex, araw=araw, a=a, static=static, bl=bl, Tb=Tb, nT=nTs, reached=reached, T=T, saturated=satd,
                clamped=araw > a_max, ca=ca, cb=cb, cc=cc, op=op)


def _chain_errors(w):
    """the derived errors of the header for one tile's float64 walk -> M, e_a, the step's error [L,P]; e_T in front of every entry [L,P]; e_T
    behind the last blended entry [P]"""
    M = 0.5 * (np.abs(w["ca"]) * w["dx"] ** 2 + np.abs(w["cc"]) * w["dy"] ** 2) + np.abs(w["cb"] * w["dx"] * w["dy"])
    e_a = 6 * U24 * M + EXP_DET_REL * (1.0 + np.abs(w["sigma"])) + U24
    step = U24 + e_a * w["a"] / (1.0 - w["a"])
    csum = np.cumsum(np.where(w["bl"], step, 0.0), 0)
    e_T_before = csum - np.where(w["bl"], step, 0.0)
    e_T_final = csum[-1] if len(csum) else np.zeros(M.shape[1:])
    return M, e_a, step, e_T_before, e_T_final


def _tile_margin(cam, w):
    M, e_a, step, e_T, _ = _chain_errors(w)
    inf = np.full(M.shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        m_sig = np.where(M > 0, np.abs(w["sigma"]) / (6 * U24 * M), inf)
        pos = w["sigma"] >= 0
        m_min = np.where(pos, np.abs(w["a"] - cam.alpha_min) / (np.float32(cam.alpha_min) * e_a), inf)
        m_max = np.where(pos & (w["a"] >= np.float32(cam.alpha_min)), np.abs(w["araw"] - np.float32(cam.alpha_max)) / (np.float32(cam.alpha_max) * e_a), inf)
        m_T = np.where(w["static"], np.abs(w["nT"] - np.float32(cam.t_min)) / (np.float32(cam.t_min) * (e_T + step)), inf)
    m = np.minimum(np.minimum(m_sig, m_min), np.minimum(m_max, m_T))
    return np.where(w["reached"], m, inf).min(0, initial=np.inf)


def composite_bwd64(kind, cam, rec, lists, g_out, g_alpha, g_depth=None, feats=None, through_alpha_max=False, sat_le=None, cache=None):
    """One view.  kind "k2" (image [3,H,W] with background, depth, alpha), "k3" (colours [H,W,3], alphas) or "feat" (feats [G,C], out
    [H,W,C], alphas).  rec [G,12] the fp32 records, lists = (tile_start [T+1], ids) front to back.  g_out in the layout of the output.
    -> dict: grad, S, chain [G,10] and bound [G,1] (|got - ref| <= bound S + chain); n_add [G] (pixels that blend the Gaussian: the addends of its sums); g_feats, S_feats [G,C]; margin [H,W];
    out, alpha (and depth): the float64 totals; counts of the branches taken.  through_alpha_max / sat_le: the wrong answers.
    The part of an output behind an entry is summed here in float64; the kernels form it as (the forward's saved total) - (running
    prefix), which is the same number up to the roundings the bound and `chain` account for, so the saved totals are no input of the reference
    (the GPU tests check them against `out` / `alpha` where both walks agree)."""
    k3 = kind != "k2"
    H, W = cam.height, cam.width
    rec = np.asarray(rec, np.float64)
    G = rec.shape[0]
    tile_start, ids_all = np.asarray(lists[0], np.int64), np.asarray(lists[1], np.int64)
    g_out, g_alpha = np.asarray(g_out, np.float64), np.asarray(g_alpha, np.float64)
    gC_img = g_out.transpose(1, 2, 0) if kind == "k2" else g_out  # [H,W,C]
    C = gC_img.shape[-1]
    gD_img = np.asarray(g_depth, np.float64) if kind == "k2" else np.zeros((H, W))
    F = np.asarray(feats, np.float64) if kind == "feat" else rec[:, 8:11]
    bg = np.array(list(cam.bg), np.float64) if kind == "k2" else np.zeros(C)
    grad, S, n_add = np.zeros((G, 10)), np.zeros((G, 10)), np.zeros(G, np.int64)
    g_feats, S_feats, chain_feats, chain = np.zeros((G, C)), np.zeros((G, C)), np.zeros((G, C)), np.zeros((G, 10))
    margin = np.full((H, W), np.inf)
    out, out_a, out_d = np.zeros((H, W, C)), np.zeros((H, W)), np.zeros((H, W))
    cnt = dict(blend=0, clamped=0, below_alpha_min=0, sigma_skip=0, saturated=0, entries_behind_saturation=0, longest_list=0, empty_tiles=0)
    hit_clamped, hit_free = np.zeros(G, np.int64), np.zeros(G, np.int64)
    walks = {}
    for tile in range(tile_start.shape[0] - 1):  # first the walks (they do not depend on the upstream gradients) and the addend counts
        ids = ids_all[tile_start[tile]:tile_start[tile + 1]]
        if ids.shape[0] == 0:
            continue
        px, py, inside, off = _tile_pixels(cam, tile, k3)
        if cache is not None and sat_le is None and tile in cache:
            walks[tile] = cache[tile]
        else:
            w = _walk(cam, rec[ids], px, py, inside, off, k3, False, sat_le)
            ce = _chain_errors(w)
            walks[tile] = (w, _tile_margin(cam, w), (ce[1], ce[3], ce[4]))
            if cache is not None and sat_le is None:
                cache[tile] = walks[tile]
        np.add.at(n_add, ids, walks[tile][0]["bl"].sum(1))
    for tile in range(tile_start.shape[0] - 1):
        ids = ids_all[tile_start[tile]:tile_start[tile + 1]]
        L = ids.shape[0]
        px, py, inside, off = _tile_pixels(cam, tile, k3)
        cnt["longest_list"] = max(cnt["longest_list"], L)
        if L == 0:
            cnt["empty_tiles"] += 1
            if kind == "k2":
                out[py[inside], px[inside]] = bg
            continue
        w, mt, (e_a, e_Tb, e_Tf) = walks[tile]
        margin[py[inside], px[inside]] = mt[inside]
        e_w = e_a + e_Tb  # [L,P] relative error of the weight a T of (entry, pixel): its own alpha, the transmittance in front of it
        bl, a, Tb = w["bl"], w["a"], w["Tb"]
        pi, pj = np.minimum(py, H - 1), np.minimum(px, W - 1)
        gC = np.where(inside[:, None], gC_img[pi, pj], 0.0)  # [P,C]
        gD, gO = np.where(inside, gD_img[pi, pj], 0.0), np.where(inside, g_alpha[pi, pj], 0.0)
        wt = np.where(bl, a * Tb, 0.0)  # [L,P]
        z = rec[ids, 2]
        Fi = F[ids]  # [L,C]
        gdc = Fi @ gC.T + (z[:, None] * gD[None] if kind == "k2" else 0.0) + gO[None]
        gdc_abs = np.abs(Fi) @ np.abs(gC).T + (np.abs(z)[:, None] * np.abs(gD)[None] if kind == "k2" else 0.0) + np.abs(gO)[None]
        q, q_abs = gdc * wt, gdc_abs * wt
        bgt, bgt_abs = w["T"] * (gC @ bg), w["T"] * (np.abs(gC) @ np.abs(bg))
        rc = np.cumsum(q[::-1], 0)[::-1]
        behind = rc - q + bgt[None]
        behind_abs = q_abs.sum(0)[None] + bgt_abs[None]
        dLda = Tb * gdc - behind / (1.0 - a)
        dLda_abs = Tb * gdc_abs + behind_abs / (1.0 - a)
        live = bl if through_alpha_max else (bl & ~w["clamped"])
        # chain error of d loss / d alpha: the front part carries the transmittance in front of the entry; the part behind is (total -
        # prefix) / (1 - a): every weight of the pixel with its own error, and 1 - a itself; the factors ex / a that follow carry e_a once more
        a1 = a / (1.0 - a)
        behind_err = (q_abs * e_w).sum(0)[None] + (bgt_abs * e_Tf)[None]
        dLda_err = Tb * gdc_abs * e_Tb + (behind_err + behind_abs * e_a * a1) / (1.0 - a) + dLda_abs * e_a
        dLda, dLda_abs, dLda_err = np.where(live, dLda, 0.0), np.where(live, dLda_abs, 0.0), np.where(live, dLda_err, 0.0)
        dx, dy, ca, cb, cc = w["dx"], w["dy"], w["ca"], w["cb"], w["cc"]
        dLds = -dLda * a  # d / d sigma
        geo_abs = {MX: np.abs(ca * dx) + np.abs(cb * dy), MY: np.abs(cc * dy) + np.abs(cb * dx), CA: 0.5 * dx * dx, CB: np.abs(dx * dy), CC: 0.5 * dy * dy}
        terms = {MX: dLds * (ca * dx + cb * dy), MY: dLds * (cc * dy + cb * dx), CA: 0.5 * dx * dx * dLds, CB: dx * dy * dLds, CC: 0.5 * dy * dy * dLds}
        terms = {k: (tv, geo_abs[k] * dLda_abs * a, geo_abs[k] * dLda_err * a) for k, tv in terms.items()}  # (value, |terms|, chain error)
        terms[OP] = (dLda * w["ex"], dLda_abs * w["ex"], dLda_err * w["ex"])
        if kind != "feat":
            for ch, k in enumerate((RR, GG, BB)):
                terms[k] = (gC[None, :, ch] * wt, np.abs(gC[None, :, ch]) * wt, np.abs(gC[None, :, ch]) * wt * e_w)
        if kind == "k2":
            terms[ZZ] = (gD[None] * wt, np.abs(gD)[None] * wt, np.abs(gD)[None] * wt * e_w)
        for k, (tv, ta, te) in terms.items():
            np.add.at(grad[:, k], ids, tv.sum(1))
            np.add.at(S[:, k], ids, ta.sum(1))
            np.add.at(chain[:, k], ids, te.sum(1))
        if kind == "feat":
            np.add.at(g_feats, ids, wt @ gC)
            np.add.at(S_feats, ids, wt @ np.abs(gC))
            np.add.at(chain_feats, ids, (wt * e_w) @ np.abs(gC))
        np.add.at(hit_clamped, ids, (bl & w["clamped"]).sum(1))
        np.add.at(hit_free, ids, (bl & ~w["clamped"]).sum(1))
        oc = wt.T @ Fi + (w["T"][:, None] * bg[None] if kind == "k2" else 0.0)
        out[py[inside], px[inside]] = oc[inside]
        out_a[py[inside], px[inside]] = wt.sum(0)[inside]
        out_d[py[inside], px[inside]] = (wt * z[:, None]).sum(0)[inside]
        rch = w["reached"] & inside[None]
        cnt["blend"] += int(bl.sum())
        cnt["clamped"] += int((bl & w["clamped"]).sum())
        cnt["sigma_skip"] += int((rch & (w["sigma"] < 0)).sum())
        cnt["below_alpha_min"] += int((rch & (w["sigma"] >= 0) & (a < np.float32(cam.alpha_min))).sum())
        cnt["saturated"] += int(w["saturated"].sum())
        cnt["entries_behind_saturation"] += int((L - rch.sum(0))[w["saturated"]].sum())
    res = dict(grad=grad, S=S, chain=chain, bound=comp_bound(n_add, C)[:, None], n_add=n_add, margin=margin, out=out if kind != "k2" else out.transpose(2, 0, 1), alpha=out_a, depth=out_d,
               counts=cnt, hit_clamped=hit_clamped, hit_free=hit_free)
    if kind == "feat":
        res.update(g_feats=g_feats, S_feats=S_feats, chain_feats=chain_feats)
    return res


def walk32_agrees(kind, cam, rec, lists, margin):
    """the float32 walk against the float64 one: -> (pixels with margin >= MARGIN at which any entry's decision (blend, clamped) differs,
    pixels below MARGIN, pixels of the frame)"""
    k3 = kind != "k2"
    tile_start, ids_all = np.asarray(lists[0], np.int64), np.asarray(lists[1], np.int64)
    rec = np.asarray(rec, np.float64)
    bad = 0
    for tile in range(tile_start.shape[0] - 1):
        ids = ids_all[tile_start[tile]:tile_start[tile + 1]]
        if ids.shape[0] == 0:
            continue
        px, py, inside, off = _tile_pixels(cam, tile, k3)
        w64 = _walk(cam, rec[ids], px, py, inside, off, k3, False)
        w32 = _walk(cam, rec[ids], px, py, inside, off, k3, True)
        diff = ((w64["bl"] != w32["bl"]) | ((w64["bl"] & w64["clamped"]) != (w32["bl"] & w32["clamped"]))).any(0)
        ok = inside & (margin[np.minimum(py, cam.height - 1), np.minimum(px, cam.width - 1)] >= MARGIN)
        bad += int((diff & ok).sum())
    return bad, int((margin < MARGIN).sum()), margin.size


def comp_bound(n_add, channels=3):
    """per-Gaussian bound of the composite stages: the roundings of a pixel term (COMP_OPS), of the channel sums in g . c and in the part
    behind (one per channel), and the order-free accumulation of n_add float atomics"""
    return (COMP_OPS + channels + np.asarray(n_add, np.float64)) * U24


def quadrant_lists_ref(cam, rec, lists):
    """the footprint test of ql_build_kernel (siu3r_amd/csrc/raster_quad_lists.h) in float64 -> {(tile, quadrant): ids}: the tile's list cut to the
    entries whose alpha >= alpha_min ellipse, padded by 0.1 % + 0.001 in the logarithm and 0.01 px, reaches a pixel centre of the 8 x 8
    quadrant.  (The box is conservative: it decides which entries a wave looks at, never what blends.)"""
    rec = np.asarray(rec, np.float64)
    gw = -(-cam.width // TILE)
    ts, ids_all = np.asarray(lists[0], np.int64), np.asarray(lists[1], np.int64)
    out = {}
    for tile in range(ts.shape[0] - 1):
        ids = ids_all[ts[tile]:ts[tile + 1]]
        r = rec[ids]
        x0t, y0t = (tile % gw) * TILE, (tile // gw) * TILE
        with np.errstate(divide="ignore", invalid="ignore"):
            Lg = np.log(r[:, 7] / cam.alpha_min) * 1.001 + 0.001
            det = r[:, 4] * r[:, 6] - r[:, 5] ** 2
            ex = np.sqrt(2 * Lg * r[:, 6] / det) + 0.01
            ey = np.sqrt(2 * Lg * r[:, 4] / det) + 0.01
        xl, xr = (r[:, 0] - ex <= x0t + 7.5) & (r[:, 0] + ex >= x0t + 0.5), (r[:, 0] - ex <= x0t + 15.5) & (r[:, 0] + ex >= x0t + 8.5)
        yt, yb = (r[:, 1] - ey <= y0t + 7.5) & (r[:, 1] + ey >= y0t + 0.5), (r[:, 1] - ey <= y0t + 15.5) & (r[:, 1] + ey >= y0t + 8.5)
        mk = (xl & yt) * 1 | (xr & yt) * 2 | (xl & yb) * 4 | (xr & yb) * 8
        mk = np.where(Lg < 0, 0, np.where((det > 0) & np.isfinite(ex) & np.isfinite(ey), mk, 15))
        for q in range(4):
            out[(tile, q)] = ids[(mk >> q) & 1 == 1]
    return out


# ---- the crafted cases -----------------------------------------------------------------------------------------------------------------
def _rotation(rng, amp):
    a = rng.normal(size=3) * amp
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return torch.linalg.matrix_exp(torch.from_numpy(K))


def _c2w(rng):
    c = torch.eye(4, dtype=DD)
    c[:3, :3] = _rotation(rng, 0.25)
    c[:3, 3] = torch.from_numpy(rng.normal(size=3) * 0.3)
    return c


def k2_cam(W, H, c2w, deg=0, band4=False, tanx=0.7, tany=0.45):
    """a mode-0 camera with tanfovx != tanfovy (the Jacobian clamp's limx != limy)"""
    from siu3r_amd import cuda_splatting as cs, raster

    w2c = torch.linalg.inv(c2w)
    proj = cs.get_projection_matrix(torch.tensor([0.2]), torch.tensor([1000.0]), torch.tensor([2 * math.atan(tanx)]), torch.tensor([2 * math.atan(tany)]))[0].double()
    return raster.make_cam_k2(w2c.float(), (proj @ w2c).float(), tanx, tany, c2w[:3, 3].tolist(), [0.1, 0.2, 0.3], W, H, sh_degree=deg, sh_band4=band4)


def k3_cam(W, H, c2w, fx=70.0, fy=55.0):
    """a mode-1 camera with the principal point off the centre (cx = 0.35 W, cy = 0.6 H: lim*_pos != lim*_neg)"""
    from siu3r_amd import raster

    return raster.make_cam_k3(torch.linalg.inv(c2w).float(), fx, fy, 0.35 * W, 0.6 * H, W, H)


#            mode V  G    deg band4 planar channels stride mean2d pose  k3 colours
PROJ_CASES = {
    "k2_deg0":          (0, 1, 257, 0, False, False, 1, 6, True, True, None),
    "k2_deg1_planar":   (0, 3, 256, 1, False, True, 25, 9, False, True, None),
    "k2_deg2_wide":     (0, 1, 255, 2, False, False, 16, 6, True, False, None),
    "k2_deg3":          (0, 3, 257, 3, True, False, 16, 9, True, True, None),
    "k2_deg4_band4":    (0, 1, 257, 4, True, False, 25, 6, False, False, None),
    "k2_deg4_no_band4": (0, 2, 256, 4, False, True, 25, 9, True, True, None),
    "k2_precomputed":   (0, 2, 255, -1, False, False, 1, 6, True, True, None),
    "k2_one":           (0, 1, 1, 2, False, False, 9, 6, True, True, None),
    "k3_rgb":           (1, 1, 257, 0, False, False, 0, 6, False, True, True),
    "k3_views":         (1, 3, 256, 0, False, False, 0, 9, False, False, False),
    "k3_two":           (1, 2, 255, 0, False, False, 0, 6, False, True, True),
    "k3_one":           (1, 1, 1, 0, False, False, 0, 9, False, True, True),
}


@functools.lru_cache(maxsize=None)
def proj_case(name):
    """-> dict: cams, means [G,3], cov6 [G,6], opac [G], colors (mode 0: interleaved [G,channels,3]; mode 1: [G,3] or None), rect [V,G,4],
    grad [V,G,10] (every term non-zero), all fp32 / int32 CPU tensors, and the case's row.  Gaussian g is of clamp class g % 6 in view 0
    (none, x at +lim, x at -lim, y at +lim, y at -lim, both) and of colour class (g // 6) % 4 (0 .. 3 channels clamped at 0)."""
    mode, V, G, deg, band4, planar, channels, stride, m2d, pose, k3col = PROJ_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    W, H = 96, 64
    c2w0 = _c2w(rng)
    c2ws = [c2w0] + [c2w0.clone() for _ in range(V - 1)]
    for c in c2ws[1:]:  # the other views: a few degrees and centimetres away (every Gaussian stays in front of them)
        c[:3, :3] = c2w0[:3, :3] @ _rotation(rng, 0.05)
        c[:3, 3] = c2w0[:3, 3] + torch.from_numpy(rng.normal(size=3) * 0.1)
    cams = [k2_cam(W, H, c, deg, band4) if mode == 0 else k3_cam(W, H, c) for c in c2ws]
    _, _, (xn, xp, yn, yp), _ = lens_limits(mode, cams[0])
    g = np.arange(G) if G > 1 else np.array([11])  # (a single Gaussian: both components clamped, one colour channel clamped)
    cls = g % 6
    u = rng.uniform(-0.8, 0.8, (G, 2))
    over = rng.uniform(1.1, 1.5, (G, 2))
    txz = np.where(np.isin(cls, (1, 5)), xp * over[:, 0], np.where(cls == 2, -xn * over[:, 0], np.where(u[:, 0] > 0, xp, xn) * u[:, 0]))
    tyz = np.where(cls == 3, yp * over[:, 1], np.where(np.isin(cls, (4, 5)), -yn * over[:, 1], np.where(u[:, 1] > 0, yp, yn) * u[:, 1]))
    tz = rng.uniform(1.5, 4.0, G)
    pc = torch.from_numpy(np.stack([txz * tz, tyz * tz, tz, np.ones(G)], -1))
    means = (pc @ c2w0.T)[:, :3].float()
    q = torch.from_numpy(rng.normal(size=(G, 4)))
    sc = torch.from_numpy(rng.uniform(0.05, 0.1, (G, 3)))
    cov6 = DG.quat_scale_to_cov6(q, sc).float()
    opac = torch.from_numpy(rng.uniform(0.05, 0.95, G)).float()
    if mode == 0 and deg >= 0:
        colors = torch.from_numpy(rng.normal(size=(G, channels, 3)) * 0.05)
        ccls = (g // 6) % 4
        colors[:, 0, :] = torch.from_numpy(np.where(np.arange(3)[None] < ccls[:, None], -4.0, 1.5))
        colors = colors.float()
    elif mode == 0:
        colors = torch.from_numpy(rng.uniform(-0.25, 1.25, (G, 1, 3))).float()
    else:
        colors = torch.from_numpy(rng.uniform(0.0, 1.0, (G, 3))).float() if k3col else None
    rect = torch.zeros((V, G, 4), dtype=torch.int32)
    rect[:] = torch.tensor([1, 1, 3, 2], dtype=torch.int32)
    for v in range(V):  # culled in some views, visible in others (and a few rows in none)
        culled = (g % 7 == 3 + v) | (g % 31 == 30) if G > 1 else np.zeros(1, bool)
        rect[v, torch.from_numpy(culled)] = 0
    mag = rng.uniform(0.1, 1.0, (V, G, 10)) * np.where(rng.random((V, G, 10)) < 0.5, -1.0, 1.0)
    return dict(name=name, mode=mode, cams=cams, means=means, cov6=cov6, opac=opac, colors=colors, rect=rect, grad=torch.from_numpy(mag).float(),
                planar=planar, stride=stride, m2d=m2d, pose=pose, G=G, V=V, deg=deg, channels=channels)


@functools.lru_cache(maxsize=None)
def proj_ref(name):
    c = proj_case(name)
    return project_bwd64(c["mode"], c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], c["rect"], c["grad"])


@functools.lru_cache(maxsize=None)
def forward_scene(kind):
    """a scene for the forward itself to project, sort and bin (the composite stages on the state of a real call): two views, 800
    Gaussians in and around the frustum, a few of them nearly opaque.  -> cams, means, cov6, opac, colors (k2: SH degree 1 [G,4,3], k3:
    rgb [G,3], feat: [G,21]), fp32"""
    rng = np.random.default_rng(sum(map(ord, kind)) + 5)
    W, H, G = 96, 64, 800
    c2w0 = _c2w(rng)
    c2w1 = c2w0.clone()
    c2w1[:3, :3] = c2w0[:3, :3] @ _rotation(rng, 0.05)
    cams = [k2_cam(W, H, c, 1) if kind == "k2" else k3_cam(W, H, c) for c in (c2w0, c2w1)]
    _, _, (xn, xp, yn, yp), _ = lens_limits(0 if kind == "k2" else 1, cams[0])
    tz = rng.uniform(1.5, 4.0, G)
    pc = torch.from_numpy(np.stack([rng.uniform(-xn, xp, G) * tz, rng.uniform(-yn, yp, G) * tz, tz, np.ones(G)], -1))
    means = (pc @ c2w0.T)[:, :3].float()
    cov6 = DG.quat_scale_to_cov6(torch.from_numpy(rng.normal(size=(G, 4))), torch.from_numpy(rng.uniform(0.05, 0.25, (G, 3)))).float()
    opac = rng.uniform(0.05, 0.95, G)
    opac[::25] = 0.999 if kind == "k2" else 0.9999
    C = 21 if kind == "feat" else 3
    if kind == "k2":
        colors = torch.from_numpy(rng.normal(size=(G, 4, 3)) * 0.3).float()
    else:
        colors = torch.from_numpy(rng.uniform(0, 1, (G, C)) if kind == "k3" else rng.normal(size=(G, C))).float()
    return dict(cams=cams, means=means, cov6=cov6, opac=torch.from_numpy(opac).float(), colors=colors, W=W, H=H, C=C)


def _conic(sx, sy, th):
    c, s = np.cos(th), np.sin(th)
    cxx, cxy, cyy = c * c * sx * sx + s * s * sy * sy, c * s * (sx * sx - sy * sy), s * s * sx * sx + c * c * sy * sy
    det = cxx * cyy - cxy * cxy
    return cyy / det, -cxy / det, cxx / det


def _rects(W, H, mx, my, radius):
    gw, gh = -(-W // TILE), -(-H // TILE)
    x0, x1 = np.clip(np.floor((mx - radius - 1) / TILE), 0, gw), np.clip(np.ceil((mx + radius + 1) / TILE), 0, gw)
    y0, y1 = np.clip(np.floor((my - radius - 1) / TILE), 0, gh), np.clip(np.ceil((my + radius + 1) / TILE), 0, gh)
    r = np.stack([x0, y0, x1, y1], -1).astype(np.int32)
    r[(x1 <= x0) | (y1 <= y0)] = 0
    return r


#             kind   W   H  V  scene     channels
COMP_CASES = {
    "k2_full":    ("k2", 96, 64, 2, "full", 3),
    "k2_ragged":  ("k2", 90, 62, 1, "full", 3),
    "k3_full":    ("k3", 90, 62, 2, "full", 3),
    "feat_full":  ("feat", 90, 62, 2, "full", 21),
    "feat_qlen":  ("feat", 96, 64, 1, "qlen", 33),
    "k2_small":   ("k2", 96, 64, 1, "small", 3),
    "k3_small":   ("k3", 96, 64, 1, "small", 3),
}
for _c in (1, 3, 5, 32, 63, 64, 168):
    COMP_CASES[f"feat_c{_c}"] = ("feat", 96, 64, 1, "small", _c)
COMP_MODES = ("all", "depth_only", "alpha_only", "one_colour")


def _scene_view(kind, W, H, scene, rng):
    """one view's crafted records in screen space -> rec [G,12] fp32, rect [G,4]"""
    gw, gh = -(-W // TILE), -(-H // TILE)
    hi_op = 0.999 if kind == "k2" else 0.9995  # (mode 1 clamps at 0.999: an opacity of 0.999 itself never exceeds it)
    parts = []  # (mx, my, sx, sy, th, op, depth)

    def add(n, mx, my, sx, sy, op, depth):
        parts.append(np.stack([np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in (mx, my, sx, sy, rng.uniform(0, np.pi, n), op, depth)], -1))

    if scene == "qlen":
        # quadrant lists of 0, 1, 31, 32, 33 and 70 entries: small splats on the centres of six quadrants (footprint box inside the quadrant)
        add(1, W / 2, H / 2, 6.0, 6.0, 0.8, 1.2)  # Gaussian 0, heavy
        for k, n in enumerate((1, 31, 32, 33, 70)):
            tx, ty = k % gw, 2 * (k // gw)
            add(n, tx * TILE + 4.0 + rng.uniform(-0.3, 0.3, n), ty * TILE + 4.0 + rng.uniform(-0.3, 0.3, n), 1.0, 1.0, 0.04, rng.uniform(2, 5, n))
        # 40 slivers: inside the padded box (+ 0.01 px) of quadrant 0 of tile (3, 3), 0.005 px short of its nearest pixel centres (a chunk in
        # which nothing blends)
        s, op = 1.2, 0.5
        reach = math.sqrt(2 * math.log(op / (1.0 / 255.0))) * s
        add(40, 3 * TILE + 7.5 + reach + 0.005, 3 * TILE + rng.uniform(1.0, 7.0, 40), s, s, op, rng.uniform(2, 5, 40))
    else:
        n_base, n_crowd = (300, 280) if scene == "full" else (120, 0)
        add(1, W / 2, H / 2, 6.0, 6.0, 0.8, 1.2)  # Gaussian 0, heavy (the padding of the quadrant lists reads record 0)
        add(n_base, rng.uniform(-8, W + 8, n_base), rng.uniform(-8, H + 8, n_base), rng.uniform(1.5, 6, n_base), rng.uniform(1.5, 6, n_base),
            rng.uniform(0.05, 0.95, n_base), np.where(np.arange(n_base) < 40, 2.0, rng.uniform(1.0, 5.0, n_base)))  # 40 equal depth keys
        hx, hy = rng.uniform(8, W - 8, 24), rng.uniform(8, H - 24, 24)
        if kind != "k2":  # opacity * exp exceeds 0.999 only within a tenth of a pixel of the mean: the means sit on pixel centres
            hx, hy = np.floor(hx) + 0.5, np.floor(hy) + 0.5
        add(24, hx, hy, rng.uniform(3, 5, 24), rng.uniform(3, 5, 24), hi_op, rng.uniform(0.5, 0.9, 24))
        add(12, rng.uniform(8, W - 8, 12), rng.uniform(8, H - 24, 12), 4.0, 4.0, 0.003, rng.uniform(0.5, 0.9, 12))  # below alpha_min
        for sx_, sy_ in ((30.0, 20.0), (60.0, 40.0), (40.0, 12.0)):  # opaque stacks: the pixels under them saturate, with entries behind
            add(6, sx_ + rng.uniform(-1, 1, 6), sy_ + rng.uniform(-1, 1, 6), 8.0, 8.0, 0.9, 0.95 + 0.001 * np.arange(6))
        if n_crowd:  # more than 256 entries of bin 0 that cover tile (0, 0)
            add(n_crowd, rng.uniform(4, 12, n_crowd), rng.uniform(4, 12, n_crowd), 1.5, 1.5, rng.uniform(0.02, 0.06, n_crowd), rng.uniform(1, 5, n_crowd))
    p = np.concatenate(parts)
    G = p.shape[0]
    rec = np.zeros((G, 12))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7] = p[:, 0], p[:, 1], p[:, 6], p[:, 5]
    rec[:, 4], rec[:, 5], rec[:, 6] = _conic(p[:, 2], p[:, 3], p[:, 4])
    rec[:, 8:11] = rng.uniform(0.0, 1.2, (G, 3))
    rect = _rects(W, H, p[:, 0], p[:, 1], 3.33 * np.maximum(p[:, 2], p[:, 3]))
    if scene != "qlen":
        # sixteen indefinite conics (the limit of a needle seen diagonally, after rounding): sigma < 0 on the pixels of their diagonal
        nd = rng.choice(np.arange(1, 1 + (300 if scene == "full" else 120)), 16, replace=False)
        s = rng.uniform(0.05, 0.5, 16)
        fr = rng.uniform(0.1, 0.4, 16)
        rec[nd, 0] = np.floor(rec[nd, 0]) + fr
        rec[nd, 1] = np.floor(rec[nd, 1]) + fr
        rec[nd, 4], rec[nd, 5], rec[nd, 6], rec[nd, 7] = s, -s * (1 + 2.0 ** -12), s, 0.3
        rect[nd] = np.array([0, 0, gw, gh - 1], np.int32)
        touch = (rect[:, 2] == gw) & (rect[:, 3] == gh)  # the last tile stays empty
        rect[touch] = 0
    return rec.astype(np.float32), rect


@functools.lru_cache(maxsize=None)
def comp_case(name):
    """-> dict: kind, cams, rec [V,G,12] fp32, rect [V,G,4], per view: sorted ids, bins (bin_start, entries), lists (tile_start, ids); feats
    [G,C] fp32 (feat); upstream gradients (numpy fp32, in the stage's layouts) before the margin pixels are zeroed"""
    kind, W, H, V, scene, C = COMP_CASES[name]
    seed = sum(map(ord, scene + kind)) + W
    rng = np.random.default_rng(seed)
    views = [_scene_view(kind, W, H, scene, rng) for _ in range(V)]
    rec, rect = np.stack([v[0] for v in views]), np.stack([v[1] for v in views])
    G = rec.shape[1]
    c2w = torch.eye(4, dtype=DD)
    cams = [k2_cam(W, H, c2w) if kind == "k2" else k3_cam(W, H, c2w) for _ in range(V)]
    geo = RS.geometry_ref(W, H)
    live = (rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1]) != 0
    keys = np.where(live, rec[..., 2].view(np.uint32), np.uint32(RS.CULLED)).astype(np.uint32)
    sorted_ids = [s[1] for s in RS.sort_ref(keys)]
    bins = [RS.bin_ref(geo, sorted_ids[v], rect[v]) for v in range(V)]
    lists = [RS.tile_lists_ref(geo, *bins[v]) for v in range(V)]
    g = np.random.default_rng(seed + 1)
    ups = dict(g_out=g.normal(size=(V, 3, H, W) if kind == "k2" else (V, H, W, C)).astype(np.float32), g_alpha=g.normal(size=(V, H, W)).astype(np.float32),
               g_depth=g.normal(size=(V, H, W)).astype(np.float32))
    feats = g.normal(size=(G, C)).astype(np.float32) if kind == "feat" else None
    return dict(name=name, kind=kind, W=W, H=H, V=V, G=G, C=C, cams=cams, geo=geo, rec=rec, rect=rect, sorted_ids=sorted_ids, bins=bins, lists=lists,
                ups=ups, feats=feats, scene=scene, walk_cache=[{} for _ in range(V)])


def comp_upstream(case, mode, margins=None):
    """the upstream gradients of a mode ("all", "depth_only", "alpha_only", "one_colour"), exactly 0 at the pixels whose margin is below
    MARGIN (margins [V,H,W]; None: not zeroed)"""
    u = {k: v.copy() for k, v in case["ups"].items()}
    if mode == "depth_only":
        u["g_out"][:], u["g_alpha"][:] = 0, 0
    elif mode == "alpha_only":
        u["g_out"][:], u["g_depth"][:] = 0, 0
    elif mode == "one_colour":
        u["g_alpha"][:], u["g_depth"][:] = 0, 0
        if case["kind"] == "k2":
            u["g_out"][:, (0, 2)] = 0
        else:
            u["g_out"][..., :1], u["g_out"][..., 2:] = 0, 0
    if case["kind"] != "k2":
        u["g_depth"][:] = 0
    if margins is not None:
        low = margins < MARGIN
        u["g_alpha"][low], u["g_depth"][low] = 0, 0
        if case["kind"] == "k2":
            u["g_out"][np.broadcast_to(low[:, None], u["g_out"].shape)] = 0
        else:
            u["g_out"][low] = 0
    return u


def comp_ref(case, mode="all", zero_margin=True, **wrong):
    """-> per view composite_bwd64 of the case with the mode's upstream gradients (margin pixels zeroed), and those gradients"""
    V = case["V"]
    kind = case["kind"]
    zeros = np.zeros((case["H"], case["W"]))
    if zero_margin:
        if "margins" not in case:  # (functools-cached dict: computed once per case, read-only afterwards)
            case["margins"] = np.stack([composite_bwd64(kind, case["cams"][v], case["rec"][v], case["lists"][v], np.zeros_like(case["ups"]["g_out"][v]), zeros,
                                                        zeros, case["feats"], cache=case["walk_cache"][v])["margin"] for v in range(V)])
        ups = comp_upstream(case, mode, case["margins"])
    else:
        ups = comp_upstream(case, mode)
    refs = [composite_bwd64(kind, case["cams"][v], case["rec"][v], case["lists"][v], ups["g_out"][v], ups["g_alpha"][v], ups["g_depth"][v], case["feats"],
                            cache=case["walk_cache"][v], **wrong) for v in range(V)]
    return refs, ups
