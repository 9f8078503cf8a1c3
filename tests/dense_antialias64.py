"""Float64 restatements of the anti-aliased K2 projection (siu3r_raster_project_aa / _c2w_aa, siu3r_raster_project_bwd_aa) and of the 3-D
smoothing filter (siu3r_mip_filter3d, siu3r_mip_apply, siu3r_mip_apply_bwd), written from the comments of include/siu3r_hip.h, with the
bounds and the crafted cases that tests/test_antialias_ref.py (CPU) and tests/test_antialias_gpu.py (GPU) share.

  aa_record64 / project_bwd_aa64   the anti-aliased record as a differentiable function -- dense_raster_bwd64.project64 (imported, not
                                   copied) with its opacity slot multiplied by comp = sqrt(max(2.5e-5, det0 / det1)) -- and grad [V,G,10]
                                   pulled back through it by float64 AUTOGRAD (the kernel's chain is hand derived, with the quotient rule
                                   simplified by hand: it is checked against differentiation, not against a second derivation)
  comp_emul32                      comp in numpy float32, operation for operation as project_kernel<true> forms it
  filter3d64, apply64              the 3-D filter and its application

THE 2-D COVARIANCE is recovered from project64's conic: det1 = 1 / (a c - b^2), (c00, c01, c11) = (c, -b, a) det1, c00' = c00 - B.  In
float64 the subtraction costs B / c00' units of 2^-53: 1e-11 relative on the smallest crafted splat (c00' = 2e-6), four orders below u.

SCALES AND BOUNDS (u = 2^-24; the conventions of dense_raster_bwd64: S = the magnitude a value's rounding errors are proportional to,
conditions computed in float64 per (view, Gaussian); device division, reciprocal and sqrtf counted as 2 u).
  comp, rec[.., 7]   S = value * (k0 + k1) / 2 with k1 = k_pt k_cov k_det, the condition product of the conic slots (project64), and
                     k0 = k_pt k_cov k_det0, k_det0 = (c00' c11' + c01^2) / det0: the condition of det0 with respect to the covariance
                     entries, which the Kahan form does not remove -- it only keeps det0's OWN rounding at 2 u instead of k_det0 u.  The
                     square root halves the radicand's relative error, hence the mean.  On the floor comp = sqrtf(2.5e-5f): S = value.
                     AA_FWD_BOUND = 81 u: the forward's PROJ_FWD_BOUND (74 u: the chain to c / det1, which counts det1 and 1 / det1)
                     + det0 2 + the division 2 + sqrtf 2 + the product with the opacity 1.
  backward           every term of dense_raster_bwd64.project_bwd64 with its scale; the opacity slot's pull-back through comp into means,
                     covariance and pose is weighted by k_pt k_cov (k_det + k_det0) -- the term divides by det1 twice and by comp, whose
                     radicand carries k_det0 -- and g_opac = sum_v comp_v grad_v[OP] by (k0 + k1) / 2 as comp itself.
                     AA_BWD_BOUND = 200 u: PROJ_BOUND (164 u) + the added chain, det0 4, r 2, sqrtf 2, 0.5 / comp 2, grad opacity 1,
                     its product 1, B / det 2 + 1, / det 1, the bracket 3, the product 1, the add into d00 1: 18 roundings (reciprocals
                     included), counted once more for the sums' other inputs: 36.
  filter             S = sqrt(variance) S_z / focal, S_z = sum_j |W_2j m_j| + |t_2| of the view that gives d (the world->camera row is
                     derived in fp64 and rounded once).  FILTER_BOUND = 16 u: the row's rounding 1, z 6 (three products, three adds),
                     fx = K00 W 1 (in focal), sqrtf 2, the product 1, the division 2: 13, rounded up.  A view SEES a Gaussian by four
                     comparisons; a row is DECIDED when every compared quantity (z - z_near; the pixel against the four frame limits) is
                     farther than 1e-4 of its scale from the threshold, three orders above the fp32 error of the pixel (about 20 u).
  apply              scales_f: s^2 1, f^2 1, the sum 1, halved by the root, sqrtf 2: 3.5 u -> APPLY_S_BOUND = 4 u of |scales_f|.
                     opac_f: q_i = |s_i| / scales_f_i 3.5 + 2 each, three of them, two products, the product with o: 19.5 u ->
                     APPLY_O_BOUND = 20 u of |opac_f|.
  apply backward     g_scales_i = T1 + T2, S = |T1| + |T2|: T1 = g_i (s_i / sf_i): 5.5 + 1; T2 = ((go o) rest_i) ((f / sf_i)^2 / sf_i): 1 +
                     (11 + 1) + 1 + (2 (3.5 + 2) + 1 + 3.5 + 2) + 1 = 32.5, the add 1 -> APPLY_BWD_BOUND = 34 u.  g_opac = go q0 q1 q2: 20 u.

COVERAGE.  As for the backward stages: a bound weighted by a condition product is only worth something while the product is small.  On
the crafted set both products, k_pt k_cov k_det and k_pt k_cov k_det0, stay <= 16 on every row that is compared
(test_antialias_ref.py::test_condition_products_of_the_crafted_set).

Not a test module."""
import functools
import math

import numpy as np
import torch

import dense_raster_bwd64 as B

U24 = B.U24
DD = torch.float64
F32 = np.float32
AA_FLOOR = 2.5e-5
AA_FWD_BOUND = 81 * U24
AA_BWD_BOUND = 200 * U24
FILTER_BOUND = 16 * U24
APPLY_S_BOUND = 4 * U24
APPLY_O_BOUND = 20 * U24
APPLY_BWD_BOUND = 34 * U24
DECIDED = 1e-4
MX, MY, CA, CB, CC, OP, RR, GG, BB, ZZ = range(10)


# ---- the anti-aliased record ---------------------------------------------------------------------------------------------------------------
def aa_terms64(cam, rec):
    """project64's record -> comp and what the scales need, all [G] float64 (differentiable where rec is)"""
    a, b, c = rec[:, CA], rec[:, CB], rec[:, CC]
    det1 = 1.0 / (a * c - b * b)
    c00, c01, c11 = c * det1, -b * det1, a * det1
    blur = float(cam.dilation)
    c00p, c11p = c00 - blur, c11 - blur
    det0 = c00p * c11p - c01 * c01
    r = det0 / det1
    comp = torch.sqrt(torch.clamp(r, min=AA_FLOOR))  # (the clamp passes no gradient below the floor)
    with torch.no_grad():
        k_det0 = (c00p * c11p + c01 * c01) / det0.abs()
    return dict(comp=comp, r=r.detach(), det0=det0.detach(), det1=det1.detach(), c00p=c00p.detach(), c01=c01.detach(), c11p=c11p.detach(), k_det0=k_det0,
                floor=(r.detach() <= AA_FLOOR))


def aa_record64(cam, means, cov6, opac, colors, pose=None):
    """the anti-aliased record of one mode-0 view: project64's with slot OP = opacity * comp.  -> rec [G,10], aux (project64's + aa_terms64's)"""
    rec, aux = B.project64(0, cam, means, cov6, opac, colors, pose)
    t = aa_terms64(cam, rec)
    out = torch.cat([rec[:, :OP], (rec[:, OP] * t["comp"])[:, None], rec[:, OP + 1:]], -1)
    return out, dict(aux, **t)


def comp_scale(aux):
    """S / value of comp (and of the record's opacity slot): (k0 + k1) / 2, 1 on the floor -> float64 [G]"""
    kc = aux["k_pt"] * aux["k_cov"]
    k = 0.5 * kc * (aux["k_det0"] + aux["k_det"])
    return torch.where(aux["floor"], torch.ones_like(k), k)


def comp_emul32(cam, means, cov6):
    """comp of one mode-0 view in numpy float32 in the kernel's expression order (project_cov2d, then the sums c00', c11' formed again
    without the blur, conic_det with its fma through float64, the division, fmaxf, sqrtf) -> comp [G] f32, r [G] f32"""
    with np.errstate(all="ignore"):
        m, S6 = np.asarray(means, F32), np.asarray(cov6, F32)
        V = np.asarray(list(cam.w2c), F32)
        W, H = cam.width, cam.height
        tx = V[0] * m[:, 0] + V[1] * m[:, 1] + V[2] * m[:, 2] + V[3]
        ty = V[4] * m[:, 0] + V[5] * m[:, 1] + V[6] * m[:, 2] + V[7]
        tz = V[8] * m[:, 0] + V[9] * m[:, 1] + V[10] * m[:, 2] + V[11]
        tanx, tany = F32(cam.tanfovx), F32(cam.tanfovy)
        fx, fy = F32(W) / (F32(2) * tanx), F32(H) / (F32(2) * tany)
        lx, ly = F32(1.3) * tanx, F32(1.3) * tany
        blur = F32(cam.dilation)
        rz = F32(1) / tz
        txz, tyz = tx * rz, ty * rz
        cxz, cyz = np.minimum(lx, np.maximum(-lx, txz)), np.minimum(ly, np.maximum(-ly, tyz))
        ctx, cty = cxz * tz, cyz * tz
        j00, j02, j11, j12 = fx * rz, -(fx * ctx) * rz * rz, fy * rz, -(fy * cty) * rz * rz
        t0 = [j00 * V[i] + j02 * V[8 + i] for i in range(3)]
        t1 = [j11 * V[4 + i] + j12 * V[8 + i] for i in range(3)]
        S = [S6[:, i] for i in range(6)]
        a = [t0[0] * S[0] + t0[1] * S[1] + t0[2] * S[2], t0[0] * S[1] + t0[1] * S[3] + t0[2] * S[4], t0[0] * S[2] + t0[1] * S[4] + t0[2] * S[5]]
        b = [t1[0] * S[0] + t1[1] * S[1] + t1[2] * S[2], t1[0] * S[1] + t1[1] * S[3] + t1[2] * S[4], t1[0] * S[2] + t1[1] * S[4] + t1[2] * S[5]]
        c00p = a[0] * t0[0] + a[1] * t0[1] + a[2] * t0[2]
        c01 = a[0] * t1[0] + a[1] * t1[1] + a[2] * t1[2]
        c11p = b[0] * t1[0] + b[1] * t1[1] + b[2] * t1[2]
        c00, c11 = c00p + blur, c11p + blur
        det = c00 * c11 - c01 * c01
        fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(F32)
        w = c01 * c01
        e = fma(-c01, c01, w)
        det0 = fma(c00p, c11p, -w) + e
        r = det0 / det
        return np.sqrt(np.fmax(F32(AA_FLOOR), r)).astype(F32), r.astype(F32)


def project_bwd_aa64(cams, means, cov6, opac, colors, rect, grad):
    """grad [V,G,10] pulled back through aa_record64 over the (view, Gaussian) pairs whose rect [V,G,4] is non-empty (the structure of
    dense_raster_bwd64.project_bwd64, mode 0, precomputed or degree-0 colours).  -> dict name -> (value, S): g_means, g_cov, g_opac, g_colors,
    pose [V,6], pose_g [V,G,6]; "comp" [V,G], "floor" [V,G] and the per-view aux"""
    V, G = len(cams), means.shape[0]
    grad, rect = torch.as_tensor(grad).to(DD), torch.as_tensor(rect).long()
    leaves = [t.detach().to(DD).requires_grad_() for t in (means, cov6, opac, colors)]
    names = ["g_means", "g_cov", "g_opac", "g_colors"]
    val = {n: torch.zeros_like(l) for n, l in zip(names, leaves)}
    S = {n: torch.zeros_like(l) for n, l in zip(names, leaves)}
    pose_g, pose_gS, auxs = torch.zeros((V, G, 6), dtype=DD), torch.zeros((V, G, 6), dtype=DD), []
    for v, cam in enumerate(cams):
        live = ((rect[v, :, 2] - rect[v, :, 0]) * (rect[v, :, 3] - rect[v, :, 1]) != 0)
        pose = torch.zeros((G, 6), dtype=DD).requires_grad_()
        rec, aux = aa_record64(cam, *leaves, pose)
        auxs.append(aux)
        kc = aux["k_pt"] * aux["k_cov"]
        for k in range(10):
            go = torch.zeros((G, 10), dtype=DD)
            go[live, k] = grad[v, live, k]
            rec_live = torch.where(live[:, None], rec, torch.zeros_like(rec))  # (a culled row's record may be NaN: it takes no part)
            gs = torch.autograd.grad(rec_live, leaves + [pose], go, retain_graph=True, allow_unused=True)
            gs = [None if g is None else torch.where(live.reshape((G,) + (1,) * (g.dim() - 1)), g, torch.zeros_like(g)) for g in gs]
            kap = torch.ones(G, dtype=DD)
            if k in (MX, MY, ZZ):
                kap = aux["k_pt"]
            elif k in (CA, CB, CC):
                kap = kc * aux["k_det"]
            elif k == OP:
                kap = torch.where(aux["floor"], torch.ones(G, dtype=DD), kc * (aux["k_det"] + aux["k_det0"]))
            kap = torch.where(live, kap, torch.ones_like(kap))
            for n, g in zip(names, gs[:-1]):
                if g is None:
                    continue
                val[n] += g
                if n in ("g_means", "g_cov"):
                    S[n] += (g.norm(dim=-1, keepdim=True) * kap[:, None]).expand_as(g)
                elif n == "g_opac":
                    S[n] += g.abs() * torch.where(live, comp_scale(aux), torch.ones(G, dtype=DD))
                else:
                    S[n] += g.abs()
            gp = gs[-1]
            if gp is not None:
                pose_g[v] += gp
                pose_gS[v] += torch.cat([gp[:, :3].norm(dim=-1, keepdim=True).expand(G, 3), gp[:, 3:].norm(dim=-1, keepdim=True).expand(G, 3)], -1) * kap[:, None]
    out = {n: (val[n], S[n]) for n in names}
    out["pose"] = (pose_g.sum(1), pose_gS.sum(1))
    out["pose_g"] = (pose_g, pose_gS)
    out["comp"] = torch.stack([a["comp"].detach() for a in auxs])
    out["floor"] = torch.stack([a["floor"] for a in auxs])
    out["aux"] = auxs
    return out


# ---- the crafted set -----------------------------------------------------------------------------------------------------------------------
SPECIAL = dict(floor=57, thin=58, cover=59, clamp=60, behind=61, offscreen=62, nan=63)


@functools.lru_cache(maxsize=None)
def aa_case():
    """V = 2 views of 64 x 48, G = 64: rows 0 .. 56 ordinary (about a pixel wide, all over the frame), then one far below a pixel (the floor
    branch), one long thin splat on the image diagonal (variance ratio 9), one covering the frame, one on the Jacobian clamp (its mean off
    the frame, its footprint on it), one behind the camera, one off the screen, one NaN mean.  fp32 CPU tensors; c2w / Kn: the poses as
    siu3r_raster_project_c2w_aa takes them (the host blocks hold the same cameras)."""
    rng = np.random.default_rng(2024)
    W, H, G, V = 64, 48, 64, 2
    c2w0 = B._c2w(rng)
    c2w1 = c2w0.clone()
    c2w1[:3, :3] = c2w0[:3, :3] @ B._rotation(rng, 0.05)
    c2w1[:3, 3] = c2w0[:3, 3] + torch.from_numpy(rng.normal(size=3) * 0.1)
    c2ws = [c2w0, c2w1]
    cams = [B.k2_cam(W, H, c, deg=-1) for c in c2ws]
    _, _, (xn, xp, yn, yp), _ = B.lens_limits(0, cams[0])
    tanx, tany = cams[0].tanfovx, cams[0].tanfovy
    txz, tyz = rng.uniform(-0.8, 0.8, G) * tanx, rng.uniform(-0.8, 0.8, G) * tany
    tz = rng.uniform(1.5, 4.0, G)
    sc = rng.uniform(0.04, 0.12, (G, 3))
    q = rng.normal(size=(G, 4))
    s = SPECIAL
    txz[s["floor"]], tyz[s["floor"]], tz[s["floor"]], sc[s["floor"]] = 0.1, -0.1, 3.0, 1e-4
    txz[s["thin"]], tyz[s["thin"]], tz[s["thin"]] = 0.0, 0.0, 2.5
    txz[s["cover"]], tyz[s["cover"]], tz[s["cover"]], sc[s["cover"]] = 0.05, 0.05, 3.0, 1.5
    txz[s["clamp"]], tyz[s["clamp"]], tz[s["clamp"]], sc[s["clamp"]] = xp * 1.2, 0.1, 2.0, 0.4
    tz[s["behind"]] = -2.0
    txz[s["offscreen"]], tyz[s["offscreen"]], tz[s["offscreen"]], sc[s["offscreen"]] = 3.0 * xp, 0.0, 2.0, 0.02
    pc = torch.from_numpy(np.stack([txz * tz, tyz * tz, tz, np.ones(G)], -1))
    means = (pc @ c2w0.T)[:, :3].float()
    cov6 = B.DG.quat_scale_to_cov6(torch.from_numpy(q), torch.from_numpy(sc))
    # the thin splat: standard deviations 0.24 and 0.08 along the image diagonals of view 0, 0.08 in depth, taken to world space
    Rz = torch.tensor([[math.sqrt(0.5), -math.sqrt(0.5), 0.0], [math.sqrt(0.5), math.sqrt(0.5), 0.0], [0.0, 0.0, 1.0]], dtype=DD)
    Sc = Rz @ torch.diag(torch.tensor([0.24 ** 2, 0.08 ** 2, 0.08 ** 2], dtype=DD)) @ Rz.T
    Sw = c2w0[:3, :3] @ Sc @ c2w0[:3, :3].T
    cov6[s["thin"]] = torch.stack([Sw[0, 0], Sw[0, 1], Sw[0, 2], Sw[1, 1], Sw[1, 2], Sw[2, 2]])
    cov6 = cov6.float()
    means[s["nan"], 1] = float("nan")
    opac = torch.from_numpy(rng.uniform(0.05, 0.95, G)).float()
    colors = torch.from_numpy(rng.uniform(-0.25, 1.25, (G, 1, 3))).float()
    grad = torch.from_numpy(rng.uniform(0.1, 1.0, (V, G, 10)) * np.where(rng.random((V, G, 10)) < 0.5, -1.0, 1.0)).float()
    Kn = torch.tensor([[0.5 / tanx, 0.0, 0.5], [0.0, 0.5 / tany, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return dict(W=W, H=H, G=G, V=V, cams=cams, c2w=torch.stack(c2ws).float(), Kn=Kn[None].repeat(V, 1, 1), means=means, cov6=cov6, opac=opac, colors=colors,
                grad=grad, expect_culled=(s["behind"], s["offscreen"], s["nan"]))


def aa_forward_ref(cams, c):
    """per view of `cams` (the blocks the projection used): comp, its S / value, the floor flags and the aux -> list of dicts (float64)"""
    out = []
    for cam in cams:
        with torch.no_grad():
            rec, aux = aa_record64(cam, c["means"], c["cov6"], c["opac"], c["colors"])
        out.append(dict(comp=aux["comp"], rel=comp_scale(aux), floor=aux["floor"], rec7=rec[:, OP], aux=aux))
    return out


# ---- the 3-D filter ------------------------------------------------------------------------------------------------------------------------
def filter3d64(means, c2w, Kn, width, height, z_near=0.2, margin=0.15, variance=0.2):
    """siu3r_mip_filter3d in float64 from the fp32 inputs -> dict: filter [G], S [G], seen [V,G] bool, decided [G] bool (every comparison
    of the row farther than DECIDED of its scale from its threshold, and so is the row that gives the largest depth), d [G] (0: unseen), dmax, focal"""
    m = torch.as_tensor(means).to(DD)
    E = torch.as_tensor(c2w).to(DD)
    K = torch.as_tensor(Kn).to(DD)
    V, G = E.shape[0], m.shape[0]
    Wm = torch.linalg.inv(E)
    R, t = Wm[:, :3, :3], Wm[:, :3, 3]
    pc = torch.einsum("vij,gj->vgi", R, m) + t[:, None, :]
    x, y, z = pc.unbind(-1)
    Sz = torch.einsum("vj,gj->vg", R[:, 2].abs(), m.abs()) + t[:, 2].abs()[:, None]
    fx, fy, cx, cy = K[:, 0, 0] * width, K[:, 1, 1] * height, K[:, 0, 2] * width, K[:, 1, 2] * height
    px, py = fx[:, None] * x / z + cx[:, None], fy[:, None] * y / z + cy[:, None]
    xl, xh, yl, yh = -margin * width, (1 + margin) * width, -margin * height, (1 + margin) * height
    seen = (z > z_near) & (px >= xl) & (px <= xh) & (py >= yl) & (py <= yh)
    seen = seen & ~torch.isnan(z)
    gaps = torch.stack([(z - z_near).abs() / z.abs().clamp_min(z_near), (px - xl).abs() / width, (px - xh).abs() / width, (py - yl).abs() / height,
                        (py - yh).abs() / height])
    front = z > z_near  # (behind the near plane only the depth test matters)
    gap = torch.where(front, gaps.min(0).values, gaps[0])
    decided = (torch.nan_to_num(gap, nan=1.0) > DECIDED).all(0)
    zs = torch.where(seen, z, torch.full_like(z, math.inf))
    d, arg = zs.min(0)
    any_seen = seen.any(0)
    d = torch.where(any_seen, d, torch.zeros_like(d))
    Szd = Sz.gather(0, arg[None])[0]
    focal = float(fx.max())
    if bool(any_seen.any()):
        far = int(torch.where(any_seen, d, torch.full_like(d, -1.0)).argmax())
        dmax, Sfar = float(d[far]), float(Szd[far])
        dd = torch.where(any_seen, d, torch.full_like(d, dmax))
        SS = torch.where(any_seen, Szd, torch.full_like(d, Sfar))
        filt, S = math.sqrt(variance) * dd / focal, math.sqrt(variance) * SS / focal
        decided = torch.where(any_seen, decided, decided & decided[far])
    else:
        dmax, filt, S = 0.0, torch.zeros(G, dtype=DD), torch.zeros(G, dtype=DD)
    return dict(filter=filt, S=S, seen=seen, decided=decided, d=d, dmax=dmax, focal=focal)


def apply64(scales, opac, filt):
    """siu3r_mip_apply in float64 (differentiable): -> scales_f [G,3], opac_f [G]"""
    s, o, f = scales.to(DD), opac.to(DD), filt.to(DD)
    sf = torch.sqrt(s * s + (f * f)[:, None])
    q = s.abs() / sf
    return sf, o * q.prod(-1)


def apply_bwd64(scales, opac, filt, g_sf, g_of):
    """-> (g_scales, S), (g_opac, S): float64 autograd of apply64, the scales from the two terms of the header's formula"""
    s, o = scales.detach().to(DD).requires_grad_(), opac.detach().to(DD).requires_grad_()
    f, g_sf, g_of = filt.to(DD), torch.as_tensor(g_sf).to(DD), torch.as_tensor(g_of).to(DD)
    sf, of = apply64(s, o, f)
    gs, go = torch.autograd.grad([sf, of], [s, o], [g_sf, g_of])
    with torch.no_grad():
        t1 = (g_sf * s / sf).abs()
        t2 = (gs - g_sf * s / sf).abs()
    return (gs, t1 + t2), (go, go.abs())


@functools.lru_cache(maxsize=None)
def filter_case():
    """V = 3 cameras of 64 x 48 on a small arc looking down +z, G = 256 means: rows 0 .. 239 in front of the cameras (most seen by all, some by
    one), then hand-placed rows: 240-243 behind every camera, 244-247 inside the margin but outside the frame (seen), 248-251 beyond the margin
    in every view (unseen: the global maximum), 252 a NaN mean (unseen), 253 the farthest seen point (it defines the maximum), 254 just in
    front of z_near (seen, the smallest depth), 255 between the cameras and z_near (unseen).  The principal point is off the centre."""
    rng = np.random.default_rng(77)
    W, H, V, G = 64, 48, 3, 256
    c2w = torch.eye(4, dtype=DD).repeat(V, 1, 1)
    for v in range(V):
        c2w[v, :3, :3] = B._rotation(rng, 0.03)
        c2w[v, 0, 3] = 0.1 * (v - 1)
    fxn, fyn, cxn, cyn = 0.9, 1.2, 0.45, 0.55
    Kn = torch.tensor([[fxn, 0, cxn], [0, fyn, cyn], [0, 0, 1]], dtype=torch.float32).repeat(V, 1, 1)
    Kn[1, 0, 0] = 0.95  # (the views' focal lengths differ: focal is the largest)
    z = rng.uniform(1.0, 6.0, G)
    u, w = rng.uniform(-0.2, 1.2, G), rng.uniform(-0.2, 1.2, G)  # normalised pixel of the middle camera (a band of them beyond the margin)
    u[244:248], w[244:248] = [-0.09, 1.09, 0.5, 0.5], [0.5, 0.5, -0.09, 1.09]
    u[248:252], w[248:252] = [-0.6, 1.6, 0.5, 0.5], [0.5, 0.5, -0.6, 1.6]
    z[240:244] = [-1.0, -3.0, -0.5, -6.0]
    u[253], w[253], z[253] = 0.5, 0.5, 9.0
    u[254], w[254], z[254] = 0.5, 0.5, 0.25
    u[255], w[255], z[255] = 0.5, 0.5, 0.1
    means = np.stack([(u - cxn) / fxn * z, (w - cyn) / fyn * z, z], -1)
    means[252] = [0.0, float("nan"), 2.0]
    return dict(W=W, H=H, V=V, G=G, c2w=c2w.float(), Kn=Kn, means=torch.from_numpy(means).float())


@functools.lru_cache(maxsize=None)
def apply_case(G=300):
    rng = np.random.default_rng(5)
    s = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (G, 3)))
    f = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), G))
    s[0], f[0] = 1e-12, 0.05      # a point: the product of the three ratios would flush, the result does not have to be exact zero
    s[1], f[1] = 0.3, 0.0         # no filter: the input back
    s[2], f[2] = (1e15, 1e-15, 1.0), 1.0
    o = rng.uniform(0.01, 0.99, G)
    g_sf, g_of = rng.normal(size=(G, 3)), rng.normal(size=G)
    t = lambda a: torch.from_numpy(np.asarray(a)).float()
    return dict(G=G, scales=t(s), opac=t(o), filt=t(f), g_sf=t(g_sf), g_of=t(g_of))
