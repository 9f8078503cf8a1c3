"""Photometric losses on the GPU: the objective of splat refinement, (1 - lambda) * L1 + lambda * (1 - SSIM), as ONE fused HIP kernel
(csrc/photo_loss.hip: value and gradient of all views in one launch) behind torch autograd.

SSIM is `metrics.ssim` with an explicit data_range (separable 11-tap Gaussian window, sigma 1.5, per channel, variances clamped at 0,
averaged over the valid (H - 10) x (W - 10) region, then over channels and views); L1 is the mean of |pred - target| over everything.
Images are read as stored: [V, C, H, W] (the K2 render), [V, H, W, C] with channels_last=True (the gsplat seam), sliced views of either;
only a layout the kernel's four strides cannot express (an expanded dimension of a differentiated `pred`) costs a `.contiguous()`.

`depth_loss` is the depth term of the same refinement (csrc/depth_loss.hip): weighted L1 or per-view Pearson correlation of the K2 render's
depth / opacity against a target depth, value and the gradients w.r.t. both render outputs from one call.
`depth_smoothness` is the instance-aware smoothness term on the same two maps (csrc/depth_smooth.hip): first or second differences of the
depth, switched off across segment boundaries and at void pixels, value and both gradients from one stencil pass.
`apply_exposure` is the per-view affine colour transform of camera optimisation (csrc/camera.hip), differentiable w.r.t. the image and M.
`apply_bilagrid` / `bilagrid_tv` are the per-view bilateral grid of colour transforms and its total-variation regulariser (csrc/bilagrid.hip).
There is no CPU path and nothing here synchronises with the host."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _gpu, _p, _stream

WINDOW = 11  # the SSIM window; H and W must reach it wherever SSIM is computed


def _as_vchw(x: torch.Tensor, channels_last: bool) -> torch.Tensor:
    """a [V, C, H, W] VIEW of an image batch stored as [V,C,H,W] / [C,H,W] or, channels_last, [V,H,W,C] / [H,W,C]"""
    if x.dim() == 3:
        x = x.unsqueeze(0)
    return x.permute(0, 3, 1, 2) if channels_last else x


def _check(pred: torch.Tensor, target: torch.Tensor, need_ssim: bool, channels_last: bool):
    for name, t in (("pred", pred), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    _gpu(pred, target)
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"photometric losses take float32 images, got {pred.dtype} and {target.dtype}")
    if pred.dim() not in (3, 4):
        raise ValueError(f"images must be [V,C,H,W], [V,H,W,C] or one image without V, got {tuple(pred.shape)}")
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pred.device != target.device:
        raise ValueError(f"pred is on {pred.device}, target on {target.device}")
    if pred.numel() == 0:
        raise ValueError(f"empty images {tuple(pred.shape)}")
    H, W = (pred.shape[-3], pred.shape[-2]) if channels_last else (pred.shape[-2], pred.shape[-1])
    if need_ssim and min(H, W) < WINDOW:
        raise ValueError(f"SSIM needs at least {WINDOW} x {WINDOW} pixels, got {H} x {W}")


def _launch(pred4: torch.Tensor, target4: torch.Tensor, lambda_dssim: float, data_range: float, want_grad: bool):
    """One siu3r_photo_loss call on [V,C,H,W] views with arbitrary non-negative strides.  Returns (out [3] = loss, L1, SSIM; grad in
    pred4's layout or None; partials [tiles, 2] = the per-workgroup (L1, SSIM) sums, view-major)."""
    lib = _lib.lib()
    V, Cn, H, W = pred4.shape
    dev = pred4.device
    n = int(lib.siu3r_photo_loss_partials(V, Cn, H, W))
    partials = torch.empty((n, 2), dtype=torch.float32, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    grad = torch.empty_strided(tuple(pred4.shape), tuple(pred4.stride()), dtype=torch.float32, device=dev) if want_grad else None
    ps, ts = (C.c_int64 * 4)(*pred4.stride()), (C.c_int64 * 4)(*target4.stride())
    with torch.cuda.device(dev):
        check(lib.siu3r_photo_loss(_p(pred4), _p(target4), V, Cn, H, W, ps, ts, float(lambda_dssim), float(data_range), _p(grad), _p(partials), _p(out),
                                   _stream()))
    return out, grad, partials


def _expressible(x4: torch.Tensor, written: bool) -> torch.Tensor:
    """strides the kernel takes: non-negative; a tensor whose layout also receives the gradient must not overlap itself (no expanded dimension)"""
    if written and any(st == 0 and sz > 1 for st, sz in zip(x4.stride(), x4.shape)):
        return x4.contiguous()
    return x4


class _PhotoLoss(torch.autograd.Function):
    """The fused kernel: the forward already produces d loss / d pred for a loss gradient of 1, the backward is one multiply."""

    @staticmethod
    def forward(ctx, pred, target, lambda_dssim, data_range, channels_last):
        p4 = _expressible(_as_vchw(pred.detach(), channels_last), True)
        t4 = _as_vchw(target.detach(), channels_last)
        out, grad, _ = _launch(p4, t4, lambda_dssim, data_range, True)
        ctx.save_for_backward(grad)
        ctx.channels_last, ctx.shape = channels_last, pred.shape
        loss, l1_, ssim_ = out[0], out[1], out[2]
        ctx.mark_non_differentiable(l1_, ssim_)
        return loss, l1_, ssim_

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_l1, _g_ssim):
        (grad,) = ctx.saved_tensors
        g = grad * g_loss
        if ctx.channels_last:
            g = g.permute(0, 2, 3, 1)
        return g.reshape(ctx.shape), None, None, None, None


def _terms(pred, target, lambda_dssim, data_range, channels_last) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    lambda_dssim, data_range = float(lambda_dssim), float(data_range)
    if not 0.0 <= lambda_dssim <= 1.0:
        raise ValueError(f"lambda_dssim must lie in [0, 1], got {lambda_dssim}")
    if not data_range > 0.0:
        raise ValueError(f"data_range must be positive, got {data_range}")
    _check(pred, target, lambda_dssim != 0.0, channels_last)
    if torch.is_grad_enabled() and pred.requires_grad:
        return _PhotoLoss.apply(pred, target, lambda_dssim, data_range, channels_last)
    out, _, _ = _launch(_as_vchw(pred.detach(), channels_last), _as_vchw(target.detach(), channels_last), lambda_dssim, data_range, False)
    return out[0], out[1], out[2]


def photometric_loss(pred: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, data_range: float = 1.0, channels_last: bool = False,
                     return_terms: bool = False):
    """(1 - lambda_dssim) * L1 + lambda_dssim * (1 - SSIM) of float32 GPU images [V,C,H,W] (channels_last: [V,H,W,C]; a single image may
    drop V), as a 0-d tensor on the device.  Differentiable w.r.t. `pred` (the subgradient of |x| at 0 and the gradient through a clamped
    variance are 0); `target` receives no gradient.  return_terms: (loss, L1, SSIM), the two terms detached; a term that lambda_dssim = 0
    or 1 switches off is not computed and comes back as NaN.  Every lambda_dssim other than 0 needs H, W >= 11."""
    loss, l1_, ssim_ = _terms(pred, target, lambda_dssim, data_range, channels_last)
    return (loss, l1_, ssim_) if return_terms else loss


def ssim(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, channels_last: bool = False, reduction: str = "mean") -> torch.Tensor:
    """`metrics.ssim(..., data_range=data_range)` on the GPU: the mean over views and channels as a 0-d tensor (differentiable w.r.t. `pred`),
    or with reduction="none" one value per view [V] (not differentiable)."""
    if reduction not in ("mean", "none"):
        raise ValueError(f'reduction must be "mean" or "none", got {reduction!r}')
    if reduction == "mean":
        if torch.is_grad_enabled() and isinstance(pred, torch.Tensor) and pred.requires_grad:
            return 1.0 - photometric_loss(pred, target, 1.0, data_range, channels_last)
        return _terms(pred, target, 1.0, data_range, channels_last)[2]
    _check(pred, target, True, channels_last)
    p4, t4 = _as_vchw(pred.detach(), channels_last), _as_vchw(target.detach(), channels_last)
    _, _, partials = _launch(p4, t4, 1.0, float(data_range), False)
    V, Cn, H, W = p4.shape
    per_view = partials.view(V, -1, 2)[:, :, 1].sum(1, dtype=torch.float64) / float(Cn * (H - WINDOW + 1) * (W - WINDOW + 1))
    return per_view.float()


def l1(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean |pred - target| over everything as a 0-d device tensor (differentiable w.r.t. `pred`); any of the layouts above"""
    return photometric_loss(pred, target, 0.0)


# ---- depth loss (csrc/depth_loss.hip) ----------------------------------------------------------------------------
DEPTH_MODES = {"l1": 0, "pearson": 1}
DEPTH_SPACES = {"depth": 0, "inverse": 1}


def _check_depth(depth, opacity, target, weight, mode, space, min_opacity):
    if mode not in DEPTH_MODES:
        raise ValueError(f"mode must be one of {tuple(DEPTH_MODES)}, got {mode!r}")
    if space not in DEPTH_SPACES:
        raise ValueError(f"space must be one of {tuple(DEPTH_SPACES)}, got {space!r}")
    if not 0.0 <= min_opacity < float("inf"):
        raise ValueError(f"min_opacity must be finite and >= 0, got {min_opacity}")
    named = [("depth", depth), ("opacity", opacity), ("target", target)] + ([("weight", weight)] if weight is not None else [])
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    _gpu(*(t for _, t in named))
    if depth.dim() not in (2, 3) or depth.numel() == 0:
        raise ValueError(f"depth must be [V,H,W] or one [H,W] image, got {tuple(depth.shape)}")
    for name, t in named:
        if t.dtype != torch.float32:
            raise ValueError(f"the depth loss takes float32 maps, {name} is {t.dtype}")
        if t.shape != depth.shape:
            raise ValueError(f"depth {tuple(depth.shape)} and {name} {tuple(t.shape)} differ in shape")
        if t.device != depth.device:
            raise ValueError(f"depth is on {depth.device}, {name} on {t.device}")


def _launch_depth(depth3, opacity3, target3, weight3, mode: str, space: str, min_opacity: float, want_grad: bool):
    """One siu3r_depth_loss call on contiguous [V,H,W] maps.  Returns (out [4] = loss, N or counted views, the factor the gradient maps
    still owe, 0; per_view [V]; valid [V] int32; g_depth, g_opacity or None, None)."""
    lib = _lib.lib()
    V, H, W = depth3.shape
    dev = depth3.device
    nbytes = int(lib.siu3r_depth_loss_ws(V, H, W))
    if nbytes <= 0:
        raise ValueError(f"depth maps {tuple(depth3.shape)} are too large for the depth loss kernel")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    per_view = torch.empty(V, dtype=torch.float32, device=dev)
    valid = torch.empty(V, dtype=torch.int32, device=dev)
    gd = torch.empty_like(depth3) if want_grad else None
    go = torch.empty_like(depth3) if want_grad else None
    with torch.cuda.device(dev):
        check(lib.siu3r_depth_loss(_p(depth3), _p(opacity3), _p(target3), _p(weight3), V, H, W, DEPTH_MODES[mode], DEPTH_SPACES[space],
                                   float(min_opacity), _p(gd), _p(go), _p(ws), _p(out), _p(per_view), _p(valid), _stream()))
    return out, per_view, valid, gd, go


def _as_vhw(x: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """contiguous [V,H,W] storage of a [V,H,W] / [H,W] map, detached (a copy only where the input is not contiguous)"""
    if x is None:
        return None
    x = x.detach()
    return (x.unsqueeze(0) if x.dim() == 2 else x).contiguous()


class _DepthLoss(torch.autograd.Function):
    """The fused kernel: the forward call already produces d loss / d depth and d loss / d opacity for a loss gradient of 1 (mode l1: up
    to the device scalar 1 / N), the backward is one multiply per map."""

    @staticmethod
    def forward(ctx, depth, opacity, target, weight, mode, space, min_opacity):
        out, per_view, valid, gd, go = _launch_depth(_as_vhw(depth), _as_vhw(opacity), _as_vhw(target), _as_vhw(weight), mode, space, min_opacity, True)
        ctx.save_for_backward(gd, go, out[2])
        ctx.shape = depth.shape
        ctx.mark_non_differentiable(per_view, valid)
        return out[0], per_view, valid

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_per_view, _g_valid):
        gd, go, owed = ctx.saved_tensors
        s = g_loss * owed
        g_depth = (gd * s).reshape(ctx.shape) if ctx.needs_input_grad[0] else None
        g_opacity = (go * s).reshape(ctx.shape) if ctx.needs_input_grad[1] else None
        return g_depth, g_opacity, None, None, None, None, None


def depth_loss(depth: torch.Tensor, opacity: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, mode: str = "l1",
               space: str = "depth", min_opacity: float = 0.5, return_terms: bool = False):
    """Depth term of splat refinement on the K2 render's own outputs, as a 0-d device tensor: `depth` is the render's sum w z, `opacity` its
    sum w, `target` the depth to match, `weight` an optional per-pixel confidence; all float32 [V,H,W] (or one [H,W] image) on the GPU.

    A pixel is valid iff opacity > min_opacity, depth > 0, target > 0, weight > 0 and all of them are finite (a NaN or an infinity makes
    the pixel invalid); an invalid pixel contributes nothing and receives a zero gradient.  space="depth" compares the expected depth
    depth / opacity with the target, space="inverse" compares opacity / depth with 1 / target.
    mode="l1" (a metric target: sensor depth, an earlier render): sum w |x - y| / sum w over the valid pixels of all views; no valid pixel
    gives 0.  mode="pearson" (a monocular prior, invariant to scale and shift): the mean over the counted views of 1 - rho_v, rho_v the
    weighted Pearson correlation of the view's valid pixels; a view counts when it has at least two valid pixels and neither x nor y is
    constant over them; no counted view gives 0.

    Differentiable w.r.t. `depth` and `opacity` (the subgradient of |x| at 0 is 0); `target` and `weight` receive no gradient.
    return_terms: (loss, per_view [V], valid [V] int32), the last two detached: per view the l1 mean or 1 - rho_v (NaN where the view has
    nothing to report) and the exact count of valid pixels.  Non-contiguous inputs cost a `.contiguous()`.  There is no CPU path, and
    nothing here synchronises with the host."""
    min_opacity = float(min_opacity)
    _check_depth(depth, opacity, target, weight, mode, space, min_opacity)
    if torch.is_grad_enabled() and (depth.requires_grad or opacity.requires_grad):
        loss, per_view, valid = _DepthLoss.apply(depth, opacity, target, weight, mode, space, min_opacity)
    else:
        out, per_view, valid, _, _ = _launch_depth(_as_vhw(depth), _as_vhw(opacity), _as_vhw(target), _as_vhw(weight), mode, space, min_opacity, False)
        loss = out[0]
    return (loss, per_view, valid) if return_terms else loss


# ---- instance-aware depth smoothness (csrc/depth_smooth.hip) -----------------------------------------------------
SMOOTH_ORDERS = (1, 2)
SMOOTH_SPACES = {"render": 0, "expected": 1}


def _check_smooth(depth, opacity, segments, order, space, min_opacity):
    if isinstance(order, bool) or order not in SMOOTH_ORDERS:
        raise ValueError(f"order must be one of {SMOOTH_ORDERS}, got {order!r}")
    if space not in SMOOTH_SPACES:
        raise ValueError(f"space must be one of {tuple(SMOOTH_SPACES)}, got {space!r}")
    if not 0.0 <= min_opacity < float("inf"):
        raise ValueError(f"min_opacity must be finite and >= 0, got {min_opacity}")
    if space == "expected" and opacity is None:
        raise ValueError('space="expected" needs the opacity map')
    named = [("depth", depth)] + ([("opacity", opacity)] if opacity is not None else []) + ([("segments", segments)] if segments is not None else [])
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    _gpu(*(t for _, t in named))
    if depth.dim() not in (2, 3) or depth.numel() == 0:
        raise ValueError(f"depth must be [V,H,W] or one [H,W] image, got {tuple(depth.shape)}")
    for name, t in named:
        if name == "segments":
            if t.dtype == torch.bool or t.is_complex():
                raise ValueError(f"segments must hold integer ids (any integer dtype, or a float map of whole numbers), got {t.dtype}")
        elif t.dtype != torch.float32:
            raise ValueError(f"the depth smoothness takes float32 maps, {name} is {t.dtype}")
        if t.shape != depth.shape:
            raise ValueError(f"depth {tuple(depth.shape)} and {name} {tuple(t.shape)} differ in shape")
        if t.device != depth.device:
            raise ValueError(f"depth is on {depth.device}, {name} on {t.device}")


def _launch_smooth(depth3, opacity3, segments3, order: int, space: str, min_opacity: float, want_grad: bool):
    """One siu3r_depth_smooth call on contiguous [V,H,W] maps (segments3: int32 or None).  Returns (out [4] = loss, x-axis part, y-axis
    part, 0; per_view [V]; active [V,2] int32; g_depth, g_opacity or None; g_opacity is None in the render space)."""
    lib = _lib.lib()
    V, H, W = depth3.shape
    dev = depth3.device
    nbytes = int(lib.siu3r_depth_smooth_ws(V, H, W))
    if nbytes <= 0:
        raise ValueError(f"depth maps {tuple(depth3.shape)} are too large for the depth smoothness kernel")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    per_view = torch.empty(V, dtype=torch.float32, device=dev)
    active = torch.empty((V, 2), dtype=torch.int32, device=dev)
    expected = SMOOTH_SPACES[space] == 1
    gd = torch.empty_like(depth3) if want_grad else None
    go = torch.empty_like(depth3) if want_grad and expected else None
    with torch.cuda.device(dev):
        check(lib.siu3r_depth_smooth(_p(depth3), _p(opacity3) if expected else None, _p(segments3), V, H, W, int(order), SMOOTH_SPACES[space],
                                     float(min_opacity), _p(gd), _p(go), _p(ws), _p(out), _p(per_view), _p(active), _stream()))
    return out, per_view, active, gd, go


def _segments_i32(segments: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """contiguous int32 [V,H,W] ids of a [V,H,W] / [H,W] map of any integer dtype or of whole-number floats (one conversion at the most)"""
    if segments is None:
        return None
    s = segments.detach()
    return (s.unsqueeze(0) if s.dim() == 2 else s).to(torch.int32).contiguous()


class _DepthSmooth(torch.autograd.Function):
    """The fused kernel: the forward call already produces d loss / d depth and d loss / d opacity for a loss gradient of 1, the backward
    is one multiply per needed map."""

    @staticmethod
    def forward(ctx, depth, opacity, segments3, order, space, min_opacity):
        out, per_view, active, gd, go = _launch_smooth(_as_vhw(depth), _as_vhw(opacity), segments3, order, space, min_opacity, True)
        ctx.save_for_backward(gd, go if ctx.needs_input_grad[1] else None)  # (an opacity map nobody differentiates is not kept)
        ctx.shape = depth.shape
        ctx.mark_non_differentiable(per_view, active)
        return out[0], per_view, active

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_per_view, _g_active):
        gd, go = ctx.saved_tensors
        g_depth = (gd * g_loss).reshape(ctx.shape) if ctx.needs_input_grad[0] else None
        g_opacity = None
        if ctx.needs_input_grad[1]:  # (the render space does not read the opacity: its derivative is zero)
            g_opacity = (go * g_loss).reshape(ctx.shape) if go is not None else torch.zeros(ctx.shape, dtype=gd.dtype, device=gd.device)
        return g_depth, g_opacity, None, None, None, None


def depth_smoothness(depth: torch.Tensor, opacity: Optional[torch.Tensor] = None, segments: Optional[torch.Tensor] = None, order: int = 1,
                     space: str = "render", min_opacity: float = 0.5, return_terms: bool = False):
    """Instance-aware depth smoothness on the K2 render's own outputs, as a 0-d device tensor: `depth` is the render's sum w z, `opacity`
    its sum w (needed only for space="expected"), both float32 [V,H,W] (or one [H,W] image) on the GPU; `segments` holds a segment id per
    pixel in the same shape (any integer dtype, or a float map of whole numbers such as the all -1.0 map of an empty panoptic result; it is
    converted to int32 once), any negative id is void; None is one segment with nothing void: plain, ungated smoothness.

    space="render" smooths x = depth (the form of the SIU3R training objective), a pixel is usable iff depth is finite; space="expected"
    smooths x = depth / opacity, usable iff opacity > min_opacity, depth > 0 and both are finite (depth_loss's rule).  order=1 takes the
    forward differences x[j+1] - x[j] along both image axes, order=2 the second differences x[j-1] - 2 x[j] + x[j+1], which leave a slanted
    plane alone.  A difference counts iff all its pixels are usable, none is void and all carry the same segment id: depth may jump between
    segments and is pulled flat (order 1) or planar (order 2) inside one.  The loss is the sum over the two axes of sum |difference| /
    number of difference positions of that axis over all views (V H (W - order) and V (H - order) W; gated positions count as zeros, as
    in the training objective); an axis too short to have a position adds 0 (where the training objective would give NaN).

    Differentiable w.r.t. `depth` and `opacity` (the subgradient of |x| at 0 is 0; an unusable or void pixel receives a zero gradient);
    `segments` receives none.  return_terms: (loss, per_view [V], active [V,2] int32), the last two detached: per view the same loss over
    the view's own positions, and the exact number of counted differences along x and along y.  Non-contiguous inputs cost a
    `.contiguous()`.  Deterministic; there is no CPU path, and nothing here synchronises with the host."""
    min_opacity = float(min_opacity)
    _check_smooth(depth, opacity, segments, order, space, min_opacity)
    seg3 = _segments_i32(segments)
    if torch.is_grad_enabled() and (depth.requires_grad or (opacity is not None and opacity.requires_grad)):
        loss, per_view, active = _DepthSmooth.apply(depth, opacity, seg3, order, space, min_opacity)
    else:
        out, per_view, active, _, _ = _launch_smooth(_as_vhw(depth), _as_vhw(opacity), seg3, order, space, min_opacity, False)
        loss = out[0]
    return (loss, per_view, active) if return_terms else loss


# ---- per-view exposure (csrc/camera.hip) -------------------------------------------------------------------------
def _launch_exposure(img4: torch.Tensor, M3: torch.Tensor) -> torch.Tensor:
    """One siu3r_exposure_apply call on a [V,3,H,W] view with arbitrary non-negative strides -> contiguous [V,3,H,W]"""
    V, _, H, W = img4.shape
    out = torch.empty((V, 3, H, W), dtype=torch.float32, device=img4.device)
    with torch.cuda.device(img4.device):
        check(_lib.lib().siu3r_exposure_apply(_p(img4), (C.c_int64 * 4)(*img4.stride()), _p(M3), V, H, W, _p(out), _stream()))
    return out


class _ApplyExposure(torch.autograd.Function):
    """The two exposure kernels: the backward computes the gradients that are asked for, g_img in the image's stored layout."""

    @staticmethod
    def forward(ctx, img, M, channels_last):
        i4 = _expressible(_as_vchw(img.detach(), channels_last), img.requires_grad)
        M3 = M.detach().reshape(-1, 3, 4).contiguous()
        ctx.save_for_backward(i4, M3)
        ctx.channels_last, ctx.img_shape, ctx.m_shape = channels_last, img.shape, M.shape
        return _launch_exposure(i4, M3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        i4, M3 = ctx.saved_tensors
        want_img, want_m = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_img or want_m):
            return None, None, None
        lib = _lib.lib()
        V, _, H, W = i4.shape
        dev = i4.device
        g_out = g_out.contiguous()
        g_img = torch.empty_strided(tuple(i4.shape), tuple(i4.stride()), dtype=torch.float32, device=dev) if want_img else None
        g_m = torch.empty((V, 3, 4), dtype=torch.float32, device=dev) if want_m else None
        ws = torch.empty(int(lib.siu3r_exposure_ws(V, H, W)) // 8, dtype=torch.float64, device=dev) if want_m else None
        with torch.cuda.device(dev):
            check(lib.siu3r_exposure_apply_bwd(_p(i4), (C.c_int64 * 4)(*i4.stride()), _p(M3), _p(g_out), V, H, W, _p(g_img), _p(g_m), _p(ws), _stream()))
        if want_img:
            g_img = (g_img.permute(0, 2, 3, 1) if ctx.channels_last else g_img).reshape(ctx.img_shape)
        return g_img, g_m.reshape(ctx.m_shape) if want_m else None, None


def apply_exposure(img: torch.Tensor, M: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
    """Per-view affine colour transform out[v,c] = sum_k M[v,c,k] img[v,k] + M[v,c,3] of float32 GPU images with 3 channels: img [V,3,H,W]
    (channels_last: [V,H,W,3]; a single image may drop V), read as stored; M [V,3,4] ([3,4] for a single image).  Returns a contiguous
    [V,3,H,W] tensor, the layout photometric_loss then reads (V = 1 for a single image).  Differentiable w.r.t. `img` (the gradient comes
    back in img's stored layout) and w.r.t. `M` (deterministic fixed-order sums); only the gradients that are needed are computed.  An
    identity M returns the bits of the input.  There is no CPU path and nothing here synchronises with the host."""
    for name, t in (("img", img), ("M", M)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    _gpu(img, M)
    if img.dtype != torch.float32 or M.dtype != torch.float32:
        raise ValueError(f"apply_exposure takes a float32 image and a float32 M, got {img.dtype} and {M.dtype}")
    if img.dim() not in (3, 4) or img.numel() == 0 or img.shape[-1 if channels_last else -3] != 3:
        raise ValueError(f"img must be [V,3,H,W], [V,H,W,3] with channels_last, or one such image without V, got {tuple(img.shape)}")
    V = 1 if img.dim() == 3 else img.shape[0]
    if tuple(M.shape) != (V, 3, 4) and not (img.dim() == 3 and tuple(M.shape) == (3, 4)):
        raise ValueError(f"M must be [{V}, 3, 4] for an image batch {tuple(img.shape)}, got {tuple(M.shape)}")
    if M.device != img.device:
        raise ValueError(f"img is on {img.device}, M on {M.device}")
    if torch.is_grad_enabled() and (img.requires_grad or M.requires_grad):
        return _ApplyExposure.apply(img, M, channels_last)
    return _launch_exposure(_as_vchw(img.detach(), channels_last), M.detach().reshape(-1, 3, 4).contiguous())


# ---- per-view bilateral grid (csrc/bilagrid.hip) -----------------------------------------------------------------
def _grid_dims(grids5: torch.Tensor) -> Tuple[int, int, int, int]:
    V, _, L, Gh, Gw = grids5.shape
    return int(V), int(L), int(Gh), int(Gw)


def _launch_bilagrid(img4: torch.Tensor, grids5: torch.Tensor) -> torch.Tensor:
    """One siu3r_bilagrid_apply call on a [V,3,H,W] view with arbitrary non-negative strides -> contiguous [V,3,H,W]"""
    V, _, H, W = img4.shape
    _, L, Gh, Gw = _grid_dims(grids5)
    out = torch.empty((V, 3, H, W), dtype=torch.float32, device=img4.device)
    with torch.cuda.device(img4.device):
        check(_lib.lib().siu3r_bilagrid_apply(_p(img4), (C.c_int64 * 4)(*img4.stride()), _p(grids5), V, H, W, L, Gh, Gw, _p(out), _stream()))
    return out


class _ApplyBilagrid(torch.autograd.Function):
    """The slice and its two backward kernels: the backward computes the gradients that are asked for, g_img in the image's stored layout."""

    @staticmethod
    def forward(ctx, img, grids, channels_last):
        i4 = _expressible(_as_vchw(img.detach(), channels_last), img.requires_grad)
        g5 = grids.detach().reshape(-1, *grids.shape[-4:]).contiguous()
        ctx.save_for_backward(i4, g5)
        ctx.channels_last, ctx.img_shape, ctx.grids_shape = channels_last, img.shape, grids.shape
        return _launch_bilagrid(i4, g5)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        i4, g5 = ctx.saved_tensors
        want_img, want_grids = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_img or want_grids):
            return None, None, None
        V, _, H, W = i4.shape
        _, L, Gh, Gw = _grid_dims(g5)
        dev = i4.device
        g_out = g_out.contiguous()
        g_img = torch.empty_strided(tuple(i4.shape), tuple(i4.stride()), dtype=torch.float32, device=dev) if want_img else None
        g_grids = torch.empty_like(g5) if want_grids else None
        with torch.cuda.device(dev):
            check(_lib.lib().siu3r_bilagrid_apply_bwd(_p(i4), (C.c_int64 * 4)(*i4.stride()), _p(g5), _p(g_out), V, H, W, L, Gh, Gw, _p(g_img), _p(g_grids),
                                                      _stream()))
        if want_img:
            g_img = (g_img.permute(0, 2, 3, 1) if ctx.channels_last else g_img).reshape(ctx.img_shape)
        return g_img, g_grids.reshape(ctx.grids_shape) if want_grids else None, None


def _check_grids(grids: torch.Tensor, who: str):
    if not isinstance(grids, torch.Tensor):
        raise TypeError(f"grids must be a tensor, got {type(grids).__name__}")
    _gpu(grids)
    if grids.dtype != torch.float32:
        raise ValueError(f"{who} takes float32 grids, got {grids.dtype}")
    if grids.dim() not in (4, 5) or grids.numel() == 0 or grids.shape[-4] != 12 or min(grids.shape[-3:]) < 2 or grids.shape[-3] > 16:
        raise ValueError(f"grids must be [V,12,L,Gh,Gw] (or [12,L,Gh,Gw]) with 2 <= L <= 16 and Gh, Gw >= 2, got {tuple(grids.shape)}")


def apply_bilagrid(img: torch.Tensor, grids: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
    """Per-view bilateral grid of affine colour transforms (Wang et al. 2024; the `use_bilateral_grid` option of 3DGS trainers) applied to
    float32 GPU images with 3 channels: img [V,3,H,W] (channels_last: [V,H,W,3]; a single image may drop V), read as stored; grids
    [V,12,L,Gh,Gw] ([12,L,Gh,Gw] for a single image), channel 4c + k = entry (c, k) of a 3 x 4 matrix.  Each pixel's matrix is the trilinear
    interpolation of the grid at ((x + 0.5) / W * (Gw - 1), (y + 0.5) / H * (Gh - 1), clamp(luminance, 0, 1) * (L - 1)), luminance =
    0.299 r + 0.587 g + 0.114 b of the pixel itself (torch's grid_sample with align_corners=True and border padding).  Returns a contiguous
    [V,3,H,W] tensor, as apply_exposure does.  Differentiable w.r.t. `img` (through the matrix and through the luminance; a clamped
    luminance passes no guidance gradient; the gradient comes back in img's stored layout) and w.r.t. `grids` (deterministic gather); only
    the gradients that are needed are computed.  An identity grid returns the bits of the input.  There is no CPU path and nothing here
    synchronises with the host."""
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"img must be a tensor, got {type(img).__name__}")
    _check_grids(grids, "apply_bilagrid")
    _gpu(img)
    if img.dtype != torch.float32:
        raise ValueError(f"apply_bilagrid takes a float32 image, got {img.dtype}")
    if img.dim() not in (3, 4) or img.numel() == 0 or img.shape[-1 if channels_last else -3] != 3:
        raise ValueError(f"img must be [V,3,H,W], [V,H,W,3] with channels_last, or one such image without V, got {tuple(img.shape)}")
    V = 1 if img.dim() == 3 else img.shape[0]
    if not (grids.dim() == 5 and grids.shape[0] == V) and not (img.dim() == 3 and grids.dim() == 4):
        raise ValueError(f"grids must be [{V}, 12, L, Gh, Gw] for an image batch {tuple(img.shape)}, got {tuple(grids.shape)}")
    if grids.device != img.device:
        raise ValueError(f"img is on {img.device}, grids on {grids.device}")
    if torch.is_grad_enabled() and (img.requires_grad or grids.requires_grad):
        return _ApplyBilagrid.apply(img, grids, channels_last)
    return _launch_bilagrid(_as_vchw(img.detach(), channels_last), grids.detach().reshape(-1, *grids.shape[-4:]).contiguous())


def _launch_tv(grids5: torch.Tensor, want_grad: bool):
    """One siu3r_bilagrid_tv call -> (value [1], d tv / d grids or None)"""
    lib = _lib.lib()
    V, L, Gh, Gw = _grid_dims(grids5)
    dev = grids5.device
    ws = torch.empty(int(lib.siu3r_bilagrid_tv_ws(V, L, Gh, Gw)) // 8, dtype=torch.float64, device=dev)
    value = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.zeros_like(grids5) if want_grad else None
    with torch.cuda.device(dev):
        check(lib.siu3r_bilagrid_tv(_p(grids5), V, L, Gh, Gw, 1.0, _p(grad), _p(ws), _p(value), _stream()))
    return value, grad


class _BilagridTV(torch.autograd.Function):
    """The forward call already produces d tv / d grids, the backward is one multiply."""

    @staticmethod
    def forward(ctx, grids):
        value, grad = _launch_tv(grids.detach().reshape(-1, *grids.shape[-4:]).contiguous(), True)
        ctx.save_for_backward(grad)
        ctx.shape = grids.shape
        return value[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value):
        (grad,) = ctx.saved_tensors
        return (grad * g_value).reshape(ctx.shape)


def bilagrid_tv(grids: torch.Tensor) -> torch.Tensor:
    """Total variation of bilateral grids [V,12,L,Gh,Gw] (or one [12,L,Gh,Gw]) as a 0-d device tensor: the mean over views of the sum over
    the z, y and x axes of the mean squared forward difference along that axis.  Differentiable w.r.t. `grids`; deterministic."""
    _check_grids(grids, "bilagrid_tv")
    if torch.is_grad_enabled() and grids.requires_grad:
        return _BilagridTV.apply(grids)
    return _launch_tv(grids.detach().reshape(-1, *grids.shape[-4:]).contiguous(), False)[0][0]
