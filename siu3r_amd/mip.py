"""Alias-free refinement (Mip-Splatting, Yu et al. 2024) on the K2 path: the control refine.refine_gaussians takes as `antialias=`, the 3-D
smoothing filter (csrc/mip_filter.hip) and its application to scales and opacities, and `bake`, which fuses a refined set's filter into the
fields for consumers that know nothing of it (PLY export, the viewer).  The 2-D half, the opacity compensation of the screen-space dilation,
lives in the projection kernels: raster.rasterize_views_k2(antialiased=True)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _gpu, _p, _stream


@dataclass
class MipFilter:
    """What refine.refine_gaussians' `antialias=` switches on.  filter_2d: render (and take the pruning statistics) with antialiased=True.
    filter_3d: bound every Gaussian's size by the training cameras' sampling rate -- the filter is recomputed from the current means and
    poses before the first render, every `every` iterations and after every event that changed or moved rows, with variance_3d the filter's
    variance in pixels^2 at the training resolution (Mip-Splatting: 0.2)."""
    filter_2d: bool = True
    filter_3d: bool = True
    variance_3d: float = 0.2
    every: int = 100

    def validate(self):
        if not (self.filter_2d or self.filter_3d):
            raise ValueError("MipFilter: a control that enables neither filter does nothing (pass antialias=None)")
        if int(self.every) <= 0:
            raise ValueError(f"MipFilter: every must be positive, got {self.every}")
        if not 0.0 < float(self.variance_3d) < float("inf"):
            raise ValueError(f"MipFilter: variance_3d must be positive and finite, got {self.variance_3d}")


def compute_filter3d(means: torch.Tensor, c2w: torch.Tensor, Kn: torch.Tensor, width: int, height: int, z_near: float = 0.2, margin: float = 0.15,
                     variance: float = 0.2) -> torch.Tensor:
    """filter [G] of siu3r_mip_filter3d: means [G,3], c2w [V,4,4] camera-to-world and Kn [V,3,3] (or [3,3]) normalised intrinsics of the
    TRAINING views, all on the GPU (no pose value is read on the host), width x height the training frame.  sqrt(variance) * d / focal with d
    the smallest depth over the views that see the Gaussian (z > z_near, pixel inside the frame grown by `margin`), the largest such depth
    for a Gaussian no view sees, focal the largest fx; zeros when nothing is seen.  Bit-reproducible.  No gradient."""
    _gpu(means, c2w, Kn)
    m = means.detach().contiguous().float()
    c = c2w.detach().float().contiguous()
    V = c.shape[0]
    K = Kn.detach().float()
    K = (K[None].expand(V, 3, 3) if K.dim() == 2 else K).contiguous()
    if tuple(c.shape) != (V, 4, 4) or tuple(K.shape) != (V, 3, 3) or m.dim() != 2 or m.shape[1] != 3:
        raise ValueError(f"compute_filter3d: means [G,3], c2w [V,4,4], Kn [V,3,3] expected, got {tuple(m.shape)}, {tuple(c.shape)}, {tuple(K.shape)}")
    lib = _lib.lib()
    out = torch.empty((m.shape[0],), dtype=torch.float32, device=m.device)
    ws = torch.empty((max(int(lib.siu3r_mip_filter3d_ws(V)) // 4, 1),), dtype=torch.float32, device=m.device)
    check(lib.siu3r_mip_filter3d(_p(c), _p(K), V, int(width), int(height), _p(m), m.shape[0], float(z_near), float(margin), float(variance), _p(out), _p(ws),
                                 _stream()))
    return out


class _ApplyFilter3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, opacities, filt):
        s, o, f = (t.detach().contiguous().float() for t in (scales, opacities, filt))
        ctx.save_for_backward(s, o, f)
        ctx.dtypes = (scales.dtype, opacities.dtype)
        sf, of = torch.empty_like(s), torch.empty_like(o)
        check(_lib.lib().siu3r_mip_apply(_p(s), _p(o), _p(f), s.shape[0], _p(sf), _p(of), _stream()))
        return sf, of

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sf, g_of):
        s, o, f = ctx.saved_tensors
        g_sf = torch.zeros_like(s) if g_sf is None else g_sf.detach().float().contiguous()
        g_of = torch.zeros_like(o) if g_of is None else g_of.detach().float().contiguous()
        gs, go = torch.empty_like(s), torch.empty_like(o)
        check(_lib.lib().siu3r_mip_apply_bwd(_p(s), _p(o), _p(f), _p(g_sf), _p(g_of), s.shape[0], _p(gs), _p(go), _stream()))
        return (gs.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None, go.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None, None)


def apply_filter3d(scales: torch.Tensor, opacities: torch.Tensor, filt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ACTIVATED scales [G,3] and opacities [G] with the filter [G] fused in (siu3r_mip_apply): scales_f = sqrt(s^2 + f^2), opac_f =
    o * prod_i s_i / scales_f_i -- the Gaussian convolved with an isotropic one of radius f, its peak lowered so that its integral stays.
    Differentiable w.r.t. scales and opacities (siu3r_mip_apply_bwd); the filter gets no gradient."""
    _gpu(scales, opacities, filt)
    if scales.dim() != 2 or scales.shape[1] != 3 or opacities.shape != scales.shape[:1] or filt.shape != scales.shape[:1]:
        raise ValueError(f"apply_filter3d: scales [G,3], opacities [G], filter [G] expected, got {tuple(scales.shape)}, {tuple(opacities.shape)}, {tuple(filt.shape)}")
    return _ApplyFilter3D.apply(scales, opacities, filt)


def bake(result: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """refine_gaussians' result dict with its "filter_3d" fused into "scales", "opacities" and "covariances" (a new dict; the other entries
    are the input's, "filter_3d" is dropped): what the last render used, for PLY export and viewers that know nothing of the filter.  A
    dict without "filter_3d" is returned as it is."""
    if "filter_3d" not in result:
        return result
    from .refine import covariances_from

    with torch.no_grad():
        scales_f, opac_f = apply_filter3d(result["scales"], result["opacities"], result["filter_3d"])
        out = {k: v for k, v in result.items() if k != "filter_3d"}
        out["scales"], out["opacities"] = scales_f, opac_f
        out["covariances"] = covariances_from(result["rotations"], scales_f)
    return out
