"""Float64 dense reference of the K3 forward (gsplat.rasterization conventions, mode 1 cameras), differentiable with autograd.

Every Gaussian is evaluated at every pixel: the same pinhole projection (mean2d = (fx x / z + cx, fy y / z + cy)), the Jacobian clamp
(limx / limy of the forward), eps2d added to the 2-D covariance, pixel centres at +0.5, the sigma < 0 skip, alpha_min / alpha_max, the
saturation test nT <= t_min and front-to-back order by (fp32 depth key, index) as siu3r_amd/csrc/raster.hip.  What the tile binning decides
(culling and the tile rect of every Gaussian) is taken from the forward as a fixed mask: tile_mask [G, T] bool.  The world->camera matrix
may be a tensor (its gradient is gsplat's v_viewmats); quaternion + scale covariances, SH colours and the background blend are the viewer
helpers of the same seam.  The gradient of this function is the reference for the HIP backward (tests/test_raster_k3_backward_*.py).
Not a test module (no test_ prefix)."""
from __future__ import annotations

import torch

import dense_raster64 as DR

TILE = DR.TILE
tile_mask_from_rect = DR.tile_mask_from_rect
tile_mask_from_lists = DR.tile_mask_from_lists


def cov6_of(cov: torch.Tensor) -> torch.Tensor:
    """[G,6] upper triangle, or [G,3,3] (entries 0, 1, 2, 4, 5, 8 read) -> [G,6] float64"""
    c = cov.double()
    if c.dim() == 2:
        return c
    return torch.stack((c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]), -1)


def quat_scale_to_cov6(quats: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """[G,4] (w,x,y,z; normalised here) + [G,3] -> [G,6] (R diag(s)^2 R^T, upper triangle)"""
    q = quats.double()
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).view(-1, 3, 3)
    M = R * scales.double()[:, None, :]
    return cov6_of(M @ M.transpose(1, 2))


def sh_eval(means: torch.Tensor, campos: torch.Tensor, sh: torch.Tensor, degree: int) -> torch.Tensor:
    """means [G,3], campos [3], sh [G,K,3] -> rgb [G,3] = max(SH(normalise(means - campos)) . sh + 0.5, 0)"""
    d = means.double() - campos.double()
    d = d / d.norm(dim=-1, keepdim=True)
    B = DR.sh_basis(d, degree, True)  # [G, (degree + 1)^2]
    return torch.clamp((B[:, :, None] * sh.double()[:, :B.shape[1], :]).sum(1) + 0.5, min=0.0)


def cam_w2c(cam) -> torch.Tensor:
    return torch.tensor(list(cam.w2c), dtype=torch.float64).reshape(4, 4)


def project(cam, means, cov, viewmat=None):
    """-> (mx, my, conic a, b, c, depth) per Gaussian, float64"""
    W, H = cam.width, cam.height
    w2c = cam_w2c(cam) if viewmat is None else viewmat.double()
    m = means.double()
    R = w2c[:3, :3]
    pc = m @ R.T + w2c[:3, 3]
    tx, ty, tz = pc.unbind(-1)
    fx, fy, cx, cy = cam.fx, cam.fy, cam.cx, cam.cy
    tfx, tfy = 0.5 * W / fx, 0.5 * H / fy
    limx_pos, limx_neg = (W - cx) / fx + 0.3 * tfx, cx / fx + 0.3 * tfx
    limy_pos, limy_neg = (H - cy) / fy + 0.3 * tfy, cy / fy + 0.3 * tfy
    cxz = torch.clamp(tx / tz, -limx_neg, limx_pos)
    cyz = torch.clamp(ty / tz, -limy_neg, limy_pos)
    z0 = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, z0, -fx * cxz / tz], -1), torch.stack([z0, fy / tz, -fy * cyz / tz], -1)], -2)
    Tm = J @ R  # [G,2,3]
    c6 = cov6_of(cov)
    S = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], -1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], -1),
                     torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], -1)], -2)
    S2 = Tm @ S @ Tm.transpose(1, 2)
    c00, c01, c11 = S2[:, 0, 0] + cam.eps2d, S2[:, 0, 1], S2[:, 1, 1] + cam.eps2d
    det = c00 * c11 - c01 * c01
    return fx * tx / tz + cx, fy * ty / tz + cy, c11 / det, -c01 / det, c00 / det, tz


def render(cam, means, cov, feats, opacities, tile_mask, viewmat=None, depth_key=None, bg=None):
    """cam: RasterCam (mode 1).  means [G,3]; cov [G,6] or [G,3,3]; feats [G,C]; opacities [G]; tile_mask [G,T]; viewmat [4,4] optional
    (default: the camera block's); depth_key [G] fp32 optional (default: the fp32 rounding of this function's depths); bg [C] optional.
    Returns colors [H,W,C] (with the background when given), alphas [H,W] in float64."""
    dd = torch.float64
    H, W = cam.height, cam.width
    mx, my, ca, cb, cc, tz = project(cam, means, cov, viewmat)
    f = feats.to(dd)
    op = opacities.to(dd).reshape(-1)
    key = (tz.detach().float() if depth_key is None else depth_key.float().cpu()).numpy()
    visible = tile_mask.any(1).numpy()
    order = sorted((i for i in range(means.shape[0]) if visible[i]), key=lambda i: (key[i], i))
    gw = (W + TILE - 1) // TILE
    py, px = torch.meshgrid(torch.arange(H, dtype=dd), torch.arange(W, dtype=dd), indexing="ij")
    ptile = ((py.long() // TILE) * gw + px.long() // TILE)
    pxc, pyc = px + 0.5, py + 0.5
    T = torch.ones((H, W), dtype=dd)
    ws = []  # blending weights per Gaussian in order; the colours are one contraction at the end (no [H,W,C] tensor per step)
    O = torch.zeros((H, W), dtype=dd)
    done = torch.zeros((H, W), dtype=torch.bool)
    for g in order:
        cover = tile_mask[g][ptile]
        dx, dy = mx[g] - pxc, my[g] - pyc
        sig = 0.5 * (ca[g] * dx * dx + cc[g] * dy * dy) + cb[g] * dx * dy
        a = torch.clamp(op[g] * torch.exp(-sig), max=cam.alpha_max)
        reach = cover & ~done & (sig >= 0) & (a >= cam.alpha_min)
        nT = T * (1 - a)
        sat = reach & (nT <= cam.t_min)
        done = done | sat
        bl = reach & ~sat
        w = torch.where(bl, a * T, torch.zeros_like(T))
        ws.append(w)
        O = O + w
        T = torch.where(bl, nT, T)
    Cm = torch.einsum("khw,kc->hwc", torch.stack(ws), f[order]) if order else torch.zeros((H, W, f.shape[1]), dtype=dd)
    if bg is not None:
        Cm = Cm + (1 - O)[..., None] * bg.to(dd)
    return Cm, O
