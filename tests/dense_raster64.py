"""Float64 dense reference of the K2 forward (3DGS / diff_gaussian_rasterization conventions, mode 0 cameras), differentiable with autograd.

Every Gaussian is evaluated at every pixel: same projection, Jacobian clamp (limx / limy), 0.3 px dilation, alpha_min / alpha_max / t_min
tests and front-to-back order by (fp32 depth key, index) as siu3r_amd/csrc/raster.hip.  What the tile binning decides (culling and the
tile rect of every Gaussian) is taken from the forward as a fixed mask: tile_mask [G, T] bool.  The gradient of this function is the
reference for the HIP backward (tests/test_raster_backward_*.py); a pose perturbation xi = (rho, theta) acts on the left of
world->camera, with the full projection moving with it (P' = P w2c^-1 exp(xi^) w2c).  Not a test module (no test_ prefix)."""
from __future__ import annotations

import math

import torch

SH_C0, SH_C1 = 0.28209479177387814, 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277, -0.5900435899266435]
SH_C4 = [2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
         0.47308734787878004, -1.7701307697799304, 0.6258357354491761]
TILE = 16


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """xi [6] = (rho, theta) -> 4x4 exp(xi^)"""
    rho, th = xi[:3], xi[3:]
    z = xi.new_zeros(())
    hat = torch.stack([torch.stack([z, -th[2], th[1], rho[0]]), torch.stack([th[2], z, -th[0], rho[1]]),
                       torch.stack([-th[1], th[0], z, rho[2]]), torch.stack([z, z, z, z])])
    return torch.linalg.matrix_exp(hat)


def sh_basis(d: torch.Tensor, deg: int, band4: bool):
    x, y, z = d.unbind(-1)
    b = [torch.full_like(x, SH_C0)]
    if deg > 0:
        b += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
        if deg > 2:
            b += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy), SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                  SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)]
            if deg > 3 and band4:
                b += [SH_C4[0] * xy * (xx - yy), SH_C4[1] * yz * (3 * xx - yy), SH_C4[2] * xy * (7 * zz - 1), SH_C4[3] * yz * (7 * zz - 3),
                      SH_C4[4] * (zz * (35 * zz - 30) + 3), SH_C4[5] * xz * (7 * zz - 3), SH_C4[6] * (xx - yy) * (7 * zz - 1),
                      SH_C4[7] * xz * (xx - 3 * yy), SH_C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(b, -1)  # [G, ncoef]


def tile_mask_from_rect(rect: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """rect [G,4] int (tx0, ty0, tx1, ty1; all zero when culled) -> [G, T] bool"""
    gw, gh = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    tx = torch.arange(gw).repeat(gh)
    ty = torch.arange(gh).repeat_interleave(gw)
    r = rect.long().cpu()
    return (tx[None] >= r[:, :1]) & (tx[None] < r[:, 2:3]) & (ty[None] >= r[:, 1:2]) & (ty[None] < r[:, 3:4])


def tile_mask_from_lists(tile_start, ids, G: int) -> torch.Tensor:
    """the oracle's per-tile id lists -> [G, T] bool"""
    ts = torch.as_tensor(tile_start).long()
    T = ts.numel() - 1
    m = torch.zeros((G, T), dtype=torch.bool)
    ids = torch.as_tensor(ids).long()
    for t in range(T):
        m[ids[ts[t]:ts[t + 1]], t] = True
    return m


def cam_tensors(cam):
    w2c = torch.tensor(list(cam.w2c), dtype=torch.float64).reshape(4, 4)
    P = torch.tensor(list(cam.proj), dtype=torch.float64).reshape(4, 4)
    return w2c, P


def render(cam, means, cov, colors, opacities, tile_mask, sh_degree=None, sh_band4=None, sh_planar=False, xi=None, w2c=None, P=None,
           depth_key=None, mean2d_offset=None):
    """cam: RasterCam (mode 0).  means [G,3]; cov [G,6] upper triangle or [G,3,3] (entries 0,1,2,4,5,8 read); colors: SH [G,n,3] (or planar
    [G,3,25]) or, with sh_degree < 0, precomputed [G,1,3]; opacities [G]; tile_mask [G,T].  xi [6] optional pose perturbation.
    depth_key [G] fp32 optional: the sort keys (default: the fp32 rounding of this function's depths).  mean2d_offset [G,2] optional: added
    to the projected means in pixels (its gradient is the pixel-space mean gradient).
    Returns image [3,H,W] (with background), depth [H,W], opacity [H,W] in float64."""
    dd = torch.float64
    H, W = cam.height, cam.width
    deg = cam.sh_degree if sh_degree is None else sh_degree
    band4 = bool(cam.sh_band4 if sh_band4 is None else sh_band4)
    m = means.to(dd)
    if w2c is None:
        w2c, P = cam_tensors(cam)
    w2c, P = w2c.to(dd), P.to(dd)
    if xi is not None:
        E = se3_exp(xi.to(dd))
        P = P @ torch.linalg.inv(w2c) @ E @ w2c
        w2c = E @ w2c
    Wr = w2c[:3, :3]
    pc = m @ Wr.T + w2c[:3, 3]
    tx, ty, tz = pc.unbind(-1)
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    limx, limy = 1.3 * cam.tanfovx, 1.3 * cam.tanfovy
    cxz = torch.clamp(tx / tz, -limx, limx)
    cyz = torch.clamp(ty / tz, -limy, limy)
    z0 = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, z0, -fx * cxz * tz / tz ** 2], -1), torch.stack([z0, fy / tz, -fy * cyz * tz / tz ** 2], -1)], -2)
    Tm = J @ Wr  # [G,2,3]
    if cov.dim() == 2:
        c6 = cov.to(dd)
    else:
        c = cov.to(dd)
        c6 = torch.stack((c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]), -1)
    S = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], -1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], -1),
                     torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], -1)], -2)
    S2 = Tm @ S @ Tm.transpose(1, 2)
    c00, c01, c11 = S2[:, 0, 0] + cam.dilation, S2[:, 0, 1], S2[:, 1, 1] + cam.dilation
    det = c00 * c11 - c01 * c01
    ca, cb, cc = c11 / det, -c01 / det, c00 / det
    hom = torch.cat([m, torch.ones_like(m[:, :1])], -1) @ P.T
    pw = 1.0 / (hom[:, 3] + 1e-7)
    mx = ((hom[:, 0] * pw + 1.0) * W - 1.0) * 0.5
    my = ((hom[:, 1] * pw + 1.0) * H - 1.0) * 0.5
    if mean2d_offset is not None:
        mx, my = mx + mean2d_offset[:, 0].to(dd), my + mean2d_offset[:, 1].to(dd)
    if deg < 0:
        col = colors.to(dd).reshape(-1, 3)
    else:
        campos = torch.tensor(list(cam.campos), dtype=dd)
        d = m - campos
        d = d / d.norm(dim=-1, keepdim=True)
        B = sh_basis(d, deg, band4)  # [G, k]
        sh = colors.to(dd)
        sh = sh.transpose(1, 2) if sh_planar else sh  # [G, n, 3]
        col = torch.clamp((B[:, :, None] * sh[:, :B.shape[1], :]).sum(1) + 0.5, min=0.0)
    op = opacities.to(dd).reshape(-1)
    key = (tz.detach().float() if depth_key is None else depth_key.float().cpu()).numpy()
    visible = tile_mask.any(1).numpy()
    order = sorted((i for i in range(m.shape[0]) if visible[i]), key=lambda i: (key[i], i))
    gw = (W + TILE - 1) // TILE
    py, px = torch.meshgrid(torch.arange(H, dtype=dd), torch.arange(W, dtype=dd), indexing="ij")
    ptile = ((py.long() // TILE) * gw + px.long() // TILE)
    T = torch.ones((H, W), dtype=dd)
    C = torch.zeros((3, H, W), dtype=dd)
    Dm = torch.zeros((H, W), dtype=dd)
    O = torch.zeros((H, W), dtype=dd)
    done = torch.zeros((H, W), dtype=torch.bool)
    for g in order:
        cover = tile_mask[g][ptile]
        dx, dy = mx[g] - px, my[g] - py
        sig = 0.5 * (ca[g] * dx * dx + cc[g] * dy * dy) + cb[g] * dx * dy
        a = torch.clamp(op[g] * torch.exp(-sig), max=cam.alpha_max)
        reach = cover & ~done & (sig >= 0) & (a >= cam.alpha_min)
        nT = T * (1 - a)
        sat = reach & (nT < cam.t_min)
        done = done | sat
        bl = reach & ~sat
        w = torch.where(bl, a * T, torch.zeros_like(T))
        C = C + col[g][:, None, None] * w
        Dm = Dm + tz[g] * w
        O = O + w
        T = torch.where(bl, nT, T)
    bg = torch.tensor(list(cam.bg), dtype=dd)
    return C + T * bg[:, None, None], Dm, O
