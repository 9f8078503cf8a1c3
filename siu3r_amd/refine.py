"""Per-scene refinement: optimise the Gaussians themselves against posed target images (the second inference-time use of the HIP rasterizer
backward; the first is pose_align.align_pose).  Every iteration is ONE multi-view K2 render (cuda_splatting.render_cuda), ONE fused photometric
loss (losses.photometric_loss) and one backward; the optimiser is torch's Adam or, with optimizer="hip", the fused visibility-aware Adam of
optim.GaussianAdam (one HIP launch per iteration for all fields).  A caller whose views are unposed aligns them first (align_pose) and
refines second."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import raster
from .cameras import CameraControl, CameraState, exposure_mode, identity_grids
from .cuda_splatting import render_cuda
from .density import FIELDS, DensityControl, DensityStats, densify_and_prune, scene_extent
from .losses import DEPTH_MODES, DEPTH_SPACES, apply_bilagrid, apply_exposure, bilagrid_tv, depth_loss, depth_smoothness, photometric_loss
from .mcmc import MCMCControl, event as mcmc_event, inject_noise, regularize
from .mip import MipFilter, apply_filter3d, compute_filter3d
from .optim import GaussianAdam, TorchAdam, log_linear, means_lr_schedule
from .prune import ContributionPrune, gaussian_contributions, prune_by_contribution
from .smooth import DepthSmoothness

# Adam steps per field, those of the 3DGS training recipe (Kerbl et al. 2023): position 1.6e-4, scaling 5e-3, rotation 1e-3, opacity 5e-2,
# SH 2.5e-3.  The recipe also multiplies the position rate by the scene extent and decays it, and steps the higher SH bands at a twentieth:
# refine_gaussians does so with optimizer="hip" (means_lr_extent_scale, means_lr_final, sh_rest_lr_scale); the default torch path does not.
DEFAULT_LRS = {"means": 1.6e-4, "scales": 5e-3, "rotations": 1e-3, "opacities": 5e-2, "harmonics": 2.5e-3}
_COV33 = (0, 1, 2, 1, 3, 4, 2, 4, 5)  # [G,6] upper triangle -> [G,3,3]
# a field <-> the unconstrained form that is optimised (and that the density kernels read)
_TO_PARAM = {"means": lambda x: x.clone(), "scales": torch.log, "rotations": lambda x: x.clone(),
             "opacities": lambda x: torch.logit(x.clamp(1e-6, 1 - 1e-6)), "harmonics": lambda x: x.clone()}
_FROM_PARAM = {"means": lambda x: x, "scales": torch.exp, "rotations": lambda x: x, "opacities": torch.sigmoid, "harmonics": lambda x: x}


def covariances_from(rotations_xyzw: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """[G,3,3] covariances R diag(scales^2) R^T of RAW (x, y, z, w) quaternions (normalised inside the kernel), no further transform"""
    cov6 = raster.quat_scale_to_cov6(torch.roll(rotations_xyzw, 1, dims=-1), scales)
    return cov6[:, list(_COV33)].view(-1, 3, 3)


def depth_weight_schedule(lambda_depth, iters: int) -> List[float]:
    """The weight of the depth term at every iteration.  A float is constant; a (start, end) pair of positive numbers decays exponentially,
    lambda_t = start * (end / start) ** (t / (iters - 1)) with both endpoints exact (the schedule of 3DGS's depth regulariser);
    iters == 1 gives [start]."""
    n = max(int(iters), 0)
    if isinstance(lambda_depth, (tuple, list)):
        if len(lambda_depth) != 2:
            raise ValueError(f"lambda_depth must be a number or a (start, end) pair, got {lambda_depth!r}")
        a, b = float(lambda_depth[0]), float(lambda_depth[1])
        if not (0.0 < a < math.inf and 0.0 < b < math.inf):
            raise ValueError(f"lambda_depth (start, end) must both be positive and finite, got {lambda_depth!r}")
        return log_linear(a, b, n)
    lam = float(lambda_depth)
    if not math.isfinite(lam):
        raise ValueError(f"lambda_depth must be finite, got {lambda_depth!r}")
    return [lam] * n


def _check_depth_args(images, depths, depth_weights, lambda_depth, depth_mode, depth_space, depth_min_opacity, iters) -> Optional[List[float]]:
    """host-side validation of refine_gaussians' depth keywords, before any device work; the schedule, or None when the term is off"""
    schedule = depth_weight_schedule(lambda_depth, iters)
    off = not isinstance(lambda_depth, (tuple, list)) and float(lambda_depth) == 0.0
    if depths is None:
        if not off:
            raise ValueError("lambda_depth is non-zero but no `depths` were given")
        if depth_weights is not None:
            raise ValueError("depth_weights without `depths`")
        return None
    if depth_mode not in DEPTH_MODES:
        raise ValueError(f"depth_mode must be one of {tuple(DEPTH_MODES)}, got {depth_mode!r}")
    if depth_space not in DEPTH_SPACES:
        raise ValueError(f"depth_space must be one of {tuple(DEPTH_SPACES)}, got {depth_space!r}")
    if not 0.0 <= float(depth_min_opacity) < math.inf:
        raise ValueError(f"depth_min_opacity must be finite and >= 0, got {depth_min_opacity}")
    want = (images.shape[0], images.shape[-2], images.shape[-1])
    for name, t in (("depths", depths), ("depth_weights", depth_weights)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
            raise ValueError(f"{name} must be a [V,H,W] tensor matching images: expected {want}, got {tuple(getattr(t, 'shape', ()))}")
    if depth_weights is not None and bool((depth_weights < 0).any()):  # (device weights: the one host read of the depth keywords)
        raise ValueError("depth_weights must be >= 0")
    return None if off else schedule


def _check_smooth_args(images, smooth, segments, iters) -> Optional[List[float]]:
    """host-side validation of refine_gaussians' smoothness keywords, before any device work; the schedule, or None without a control"""
    if smooth is None:
        if segments is not None:
            raise ValueError("segments without a `smooth` control: pass smooth=DepthSmoothness(...)")
        return None
    if not isinstance(smooth, DepthSmoothness):
        raise ValueError(f"smooth must be a smooth.DepthSmoothness or None, got {type(smooth).__name__}")
    smooth.validate()
    if segments is not None:
        want = (images.shape[0], images.shape[-2], images.shape[-1])
        if not isinstance(segments, torch.Tensor) or tuple(segments.shape) != want:
            raise ValueError(f"segments must be a [V,H,W] tensor matching images: expected {want}, got {tuple(getattr(segments, 'shape', ()))}")
        if segments.dtype == torch.bool or segments.is_complex():
            raise ValueError(f"segments must hold integer ids, got {segments.dtype}")
    return smooth.weights(iters)


OPTIMIZERS = ("torch", "hip")


def _aux_cat(aux: List[dict], key: str) -> torch.Tensor:
    """one field of render_cuda's aux (a dict per view group) over all views"""
    return aux[0][key] if len(aux) == 1 else torch.cat([a[key] for a in aux])


def _check_optim_args(optimizer, sparse, means_lr_final, means_lr_extent_scale, sh_rest_lr_scale) -> bool:
    """host-side validation of refine_gaussians' optimiser keywords, before any device work; True for the HIP optimiser"""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
    if means_lr_final is not None and not 0.0 < float(means_lr_final) < math.inf:
        raise ValueError(f"means_lr_final must be positive and finite (or None), got {means_lr_final!r}")
    if not 0.0 <= float(sh_rest_lr_scale) < math.inf:
        raise ValueError(f"sh_rest_lr_scale must be finite and >= 0, got {sh_rest_lr_scale!r}")
    if optimizer == "torch":
        asked = [name for name, on in (("sparse", bool(sparse)), ("means_lr_final", means_lr_final is not None),
                                       ("means_lr_extent_scale", bool(means_lr_extent_scale)), ("sh_rest_lr_scale", float(sh_rest_lr_scale) != 1.0)) if on]
        if asked:
            raise ValueError(f'{", ".join(asked)}: only optimizer="hip" implements this (optimizer="torch" is plain torch.optim.Adam)')
    return optimizer == "hip"


@dataclass
class _Strategy:
    """what refine_gaussians' loop needs to know of its control, made once before the loop (the defaults: no control)"""
    events: Sequence[int] = ()            # iterations that begin with a density event
    resets: Sequence[int] = ()            # iterations that begin with an opacity reset (clone / split / prune only)
    stats: Optional[DensityStats] = None  # what every backward accumulates into (clone / split / prune only; renewed at each event)
    reg_o: float = 0.0                    # MCMC: the regulariser weight of the free opacities; > 0 (or reg_s): that step follows the backward
    reg_s: float = 0.0                    # ... of the free scales
    noise_lr: float = 0.0                 # MCMC: > 0: the noise step follows the optimiser's


def refine_gaussians(means, scales, rotations, opacities, harmonics, images, c2w, Kn, near, far, bg, iters: int = 200, lambda_dssim: float = 0.2,
                     lrs: Optional[Dict[str, float]] = None, params: Sequence[str] = FIELDS, log_every: int = 1,
                     density: Union[DensityControl, MCMCControl, None] = None, depths=None, depth_weights=None, lambda_depth=0.0, depth_mode: str = "l1",
                     depth_space: str = "depth", depth_min_opacity: float = 0.5, optimizer: str = "torch", sparse: bool = False,
                     means_lr_final: Optional[float] = None, means_lr_extent_scale: bool = False,
                     sh_rest_lr_scale: float = 1.0, cameras: Optional[CameraControl] = None,
                     prune: Optional[ContributionPrune] = None,
                     antialias: Optional[MipFilter] = None, smooth: Optional[DepthSmoothness] = None,
                     segments=None) -> Tuple[Dict[str, torch.Tensor], List[float]]:
    """means [G,3], scales [G,3], rotations [G,4], opacities [G], harmonics [G,3,n] (n = (deg+1)^2): what `Gaussians` carries, on the GPU.
    images [V,3,H,W]: the posed target views; c2w [V,4,4] camera-to-world, Kn [V,3,3] (or [3,3]) normalised intrinsics, near / far floats
    (or [V]), bg 3 floats: render_cuda's conventions.

    `rotations` are the adapter's RAW quaternions in (x, y, z, w) order, as `Gaussians.rotations` holds them; the covariance is built from
    their normalised form and `scales` with no further transform.  raster.quat_scale_to_cov6 takes (w, x, y, z): the reordering happens in
    here, and the returned `rotations` are in the input's order again.

    Optimised is the usual unconstrained parametrisation: means, log-scales, raw quaternions, logit opacities (the inputs clamped into
    [1e-6, 1 - 1e-6] before the logit), SH coefficients; covariances are rebuilt from quaternions and scales every step.  `params` names the
    fields that move; the others stay frozen, receive no gradient and are returned bit-identical.  One torch.optim.Adam with a parameter
    group per field; `lrs` overrides DEFAULT_LRS per field.  iters = 0 moves nothing.

    Returns ({"means", "scales", "rotations", "opacities", "harmonics", "covariances" [G,3,3]}: new tensors, the inputs are not modified;
    the losses of the logged iterations: every `log_every`-th, each costing one host read; log_every = 0 reads nothing).

    density: a density.DensityControl turns on adaptive density control (3DGS section 5.2); None, the default, is the path above and
    returns the same bits as a call without the keyword.  With a control every backward also accumulates the densification statistics
    (density.DensityStats), and at the iterations control.events(iters) names, before that iteration's render, ALL five fields in their
    unconstrained form and the Adam moments of the free ones go through density.densify_and_prune: Gaussians are cloned, split and
    pruned in memory order, survivors keep their exp_avg / exp_avg_sq, new rows start from zero moments, the optimiser is rebuilt on the
    new leaves with each group's step count preserved, and the statistics start over.  One host read per event (the new row count).
    `params` only governs what Adam moves: a control together with frozen geometry still clones and prunes, and the children of a split
    still get their own means and the smaller scale.  Frozen means, rotations and harmonics keep the bits of the rows that survive;
    frozen scales / opacities make one round trip through log / logit at the first event.  An opacity reset clamps the free logit
    opacities to at most logit(control.reset_opacity) and zeroes their moments (frozen opacities could never recover and are left
    alone).  Every returned tensor then has the new row count, and the dict gains "density_events": one info dict per event
    (densify_and_prune's counts plus "iteration").  control.scene_extent = None costs one host read of the camera centres.
    control.absgrad = True keeps the absolute-gradient statistics of AbsGS instead (DensityStats(absgrad=True), at the start and after
    every event); the events, their info dicts and the threshold the control names are used as they are.

    density may instead be a mcmc.MCMCControl: the budgeted strategy of Kheradmand et al. 2024 (3DGS as Markov-chain Monte Carlo).  No
    statistics are kept (the render gets density_stats=None).  At the iterations control.events(iters) names, before that iteration's
    render, mcmc.relocate moves every dead Gaussian (opacity <= min_opacity) onto a live one IN PLACE and mcmc.grow adds
    int(grow_factor * G) - G rows, never past cap_max, over all five fields, free or frozen; the optimiser is rebound when the row count
    changed (step count kept).  One host read per event (the number of dead rows).  After every backward mcmc.regularize adds the
    gradients of opacity_reg * mean(opacity) and scale_reg * mean(scale) to the FREE opacity / scale leaves (a frozen field's term is a
    constant and is left out), and `losses` logs the objective including both values.  After every optimiser step, when `means` is free and
    noise_lr > 0, mcmc.inject_noise moves the means by covariance-shaped noise scaled by noise_lr * (this iteration's `means` rate,
    schedule included), for every Gaussian (sparse=True skips no row here).  "density_events" then holds one dict per event: iteration,
    rows_in, rows_out, relocated, added.  A cap_max below the starting row count, a non-finite or negative field and every <= 0 raise
    ValueError before any device work.

    depths [V,H,W] with a non-zero lambda_depth adds a depth term: the objective of iteration t is photometric + lambda_t *
    losses.depth_loss(render depth, render opacity, depths, depth_weights, depth_mode, depth_space, depth_min_opacity) on the same
    render's depth (sum w z) and opacity (sum w) maps, both of which carry gradients.  depth_weights [V,H,W] (>= 0) is a per-pixel
    confidence; pixels where depths <= 0 are holes.  lambda_depth is a float or a (start, end) pair decayed exponentially over the
    iterations (depth_weight_schedule).  `losses` then logs the total objective and the returned dict gains "depth_losses": the
    unweighted depth term at the logged iterations.  depths=None or lambda_depth == 0 never calls depth_loss: the loop is the one above.
    `density=` works unchanged with a depth term; its statistics see the gradient of the total objective.

    optimizer: "torch" (the default: the loop above, bit for bit) or "hip": optim.GaussianAdam, one fused launch per iteration for all free
    fields with the same arithmetic per element.  Only "hip" takes the remaining keywords (with "torch" they raise ValueError):
    sparse=True asks every iteration's render for its radii and skips the Gaussians no training view saw (parameters and moments keep their
    bits; the bias correction still uses the global step count);  means_lr_final decays the `means` rate log-linearly from its `lrs` value
    to this over `iters` (optim.means_lr_schedule);  means_lr_extent_scale=True multiplies both ends by the scene extent
    (density.scene_extent of the control when it names one, else density.scene_extent(c2w): one host read);  sh_rest_lr_scale steps the SH
    coefficients above DC at that fraction of the `harmonics` rate (3DGS: 0.05).  `density=` and the depth keywords work as above; the
    returned dict gains "optimizer_steps", the optimiser's step count (== iters, also across density events).

    cameras: a cameras.CameraControl also optimises the per-view pose and / or a per-view affine colour transform ("exposure"); None, the
    default, is the loop above and returns the same bits as a call without the keyword.  With a control, every iteration from
    control.start on renders with the current poses (a copy of `c2w` held by a cameras.CameraState; the caller's tensor is not modified)
    and, when control.pose, with the state's gradient holders as cam_rot_delta / cam_trans_delta; when control.exposure the image goes
    through losses.apply_exposure before photometric_loss (the depth term keeps reading the render's own depth and opacity).  After the
    Gaussians' optimiser step the camera step runs: one fused launch (Adam and the se(3) retraction, csrc/camera.hip) whatever `optimizer`
    says, its rates decayed by control.lr_final_scale over the iterations from control.start on.  The views of control.fixed keep the
    bits of their pose and an exactly identity exposure.  `density=`, `depths=` and `sparse=` work unchanged; a classic control's scene
    extent is still taken from the starting cameras.  params=() with a control is multi-view pose / exposure alignment against frozen
    Gaussians (without a control params=() runs no iteration).  The returned dict gains "c2w" [V,4,4], "exposure" [V,3,4] (identity where
    it is not optimised) and "camera_steps".  A control that moves nothing, a fixed index out of range, every view fixed and a
    non-positive rate raise ValueError before any device work.

    control.exposure = "bilagrid" (True and "affine" are the transform above) replaces the one matrix per view by a bilateral grid of them
    (control.bilagrid_shape = (Gh, Gw, L); csrc/bilagrid.hip): from control.start on the render goes through losses.apply_bilagrid, the
    objective gains control.lambda_tv * losses.bilagrid_tv(grids), which `losses` logs with the rest, and after the Gaussians' optimiser step
    the grids take an Adam step of their own (optim.GaussianAdam, rate control.lr_bilagrid decayed like the others; fixed views keep the
    bits of the identity grid) before the camera launch steps the poses.  The returned dict gains "bilagrid" [V,12,L,Gh,Gw]; "exposure"
    stays the identity.  An unknown exposure string raises ValueError before any device work.

    prune: a prune.ContributionPrune removes the Gaussians that contribute to no training view; None, the default, is the loop above: nothing
    is launched, allocated or read that is not without the keyword.  At the iterations prune.events(iters) names, before that iteration's
    render and after a density event of the same iteration, prune.gaussian_contributions renders the blend statistics of ALL training views
    with the current parameters and the current poses (the cameras' when a CameraControl moves them) and prune.prune_by_contribution drops
    the rows whose largest blending weight stays below prune.min_weight (or that fewer than min_views views blend, or beyond the
    keep_at_most largest weight sums), over all five fields, free or frozen, and the free ones' Adam moments; kept rows keep their bits and
    their order, the optimiser moves to the new leaves with its step count, and a classic control's statistics start over at the new size.
    One host read per event.  prune.final = True runs one more event after the last iteration, so the returned set is pruned.  The returned
    dict gains "prune_events": one info dict per event (prune_by_contribution's counts plus "iteration"; the final one carries `iters`).
    An event that would leave no Gaussian raises RuntimeError.  An MCMCControl keeps an exact row count and relocates its dead rows itself:
    prune= together with it, and a schedule with every <= 0, raise ValueError before any device work.

    antialias: a mip.MipFilter refines alias-free (Mip-Splatting, Yu et al. 2024), so that the result also holds at another image size or
    distance; None, the default, is the loop above: nothing is launched, allocated or read that is not without the keyword, and the returned
    bits are identical.  With antialias.filter_3d the 3-D smoothing filter (mip.compute_filter3d at the training frame size, variance
    antialias.variance_3d) is computed from the current means and the current poses (the cameras' when a CameraControl moves them) before
    the first render, every antialias.every iterations and after every density, MCMC or pruning event that changed or moved rows, and every
    iteration sends exp(log-scales) and sigmoid(logit opacities) through mip.apply_filter3d before the covariance is built: the optimised
    scales and opacities stay the raw ones, gradients reach them through the filter, the filter itself gets none.  With
    antialias.filter_2d the render, and the contribution renders of `prune=`, run with antialiased=True (raster.rasterize_views_k2).  The
    density rules keep looking at the raw scales, as Mip-Splatting's do.  Returned: "scales" / "opacities" stay the raw optimised ones,
    "covariances" is what the last render would use (the filtered scales), and with filter_3d the dict gains "filter_3d" [G] in the final
    row count; mip.bake fuses it into the fields for consumers that know nothing of it.  A control that enables neither filter, every <= 0
    and variance_3d <= 0 raise ValueError before any device work.

    smooth: a smooth.DepthSmoothness adds the instance-aware depth smoothness of the SIU3R training objective; None, the default, is the loop
    above: depth_smoothness is never called, nothing is launched, allocated or read that is not without the keyword, and no new keyword
    reaches render_cuda.  With a control the objective of iteration t gains weight_t * losses.depth_smoothness(render depth, render
    opacity, segments, smooth.order, smooth.space, smooth.min_opacity) on the same render (space="expected" asks the render for its
    opacity map, as the depth term does); smooth.weight is a float or a (start, end) pair decayed exponentially over the iterations
    (depth_weight_schedule).  segments [V,H,W] are the segment ids of the TRAINING views (any integer dtype, negative = void: the
    `segmentation` SIU3RModel.forward returns for its context views); they are converted to int32 once and stay fixed.  segments=None with
    a control is plain, ungated smoothness.  `losses` then logs the total objective and the returned dict gains "smooth_losses": the
    unweighted term at the logged iterations.  `density=`, `depths=`, `cameras=`, `prune=`, `antialias=` and optimizer="hip" work
    unchanged; the density statistics see the gradient of the total objective.  segments without a control, segments of another shape
    than the views, a weight that is not positive and finite and an unknown order or space raise ValueError before any device work."""
    if antialias is not None:
        antialias.validate()
    lambdas_smooth = _check_smooth_args(images, smooth, segments, iters)
    lambdas_depth = _check_depth_args(images, depths, depth_weights, lambda_depth, depth_mode, depth_space, depth_min_opacity, iters)
    hip = _check_optim_args(optimizer, sparse, means_lr_final, means_lr_extent_scale, sh_rest_lr_scale)
    params = tuple(params)
    for p in params:
        if p not in FIELDS:
            raise ValueError(f"params: unknown field {p!r} (one of {FIELDS})")
    lr = dict(DEFAULT_LRS)
    for k, v in (lrs or {}).items():
        if k not in FIELDS:
            raise ValueError(f"lrs: unknown field {k!r} (one of {FIELDS})")
        lr[k] = float(v)
    if cameras is not None:
        cameras.validate(images.shape[0])
    budgeted = isinstance(density, MCMCControl)  # which of the two strategies a control is: said here, read where they differ
    if budgeted:
        density.validate(means.shape[0])
    if prune is not None and budgeted:
        raise ValueError("prune= cannot be combined with an MCMCControl: the budgeted strategy keeps an exact row count and relocates its dead rows itself")
    prune_at = () if prune is None else tuple(prune.events(int(iters)))
    if int(iters) <= 0:
        params = ()
    dev = means.device
    start = {"means": means, "scales": scales, "rotations": rotations, "opacities": opacities, "harmonics": harmonics}
    start = {k: v.detach().float() for k, v in start.items()}
    target = images.detach().float().to(dev)
    V, _, H, W = target.shape
    c2w = c2w.detach().float().to(dev)
    Kn = Kn.detach().float().to(dev)
    Kn = Kn[None].expand(V, 3, 3) if Kn.dim() == 2 else Kn
    as_v = lambda x: x.detach().float().cpu().reshape(-1).expand(V) if isinstance(x, torch.Tensor) else torch.full((V,), float(x))
    near_t, far_t = as_v(near), as_v(far)
    bg_t = torch.tensor([[float(b) for b in bg]]).expand(V, 3)

    # the free fields in their unconstrained form (an event may replace the leaves); `value` reads any field in the form the render takes
    free = {k: _TO_PARAM[k](start[k]).requires_grad_(True) for k in FIELDS if k in params}
    value = lambda k: _FROM_PARAM[k](free[k]) if k in free else start[k]
    cov_moves = "scales" in free or "rotations" in free
    cov6_of = lambda: raster.quat_scale_to_cov6(torch.roll(value("rotations"), 1, dims=-1), value("scales"))
    aa_kw = dict(antialiased=True) if antialias is not None and antialias.filter_2d else {}  # (no control: the calls carry no keyword)
    mip3d = antialias is not None and antialias.filter_3d
    filter3d = None  # [G], of the current rows; None: to be computed before the next render
    if mip3d:  # the covariance is built from the filtered scales, which follow the means: nothing of it is fixed
        cov_moves, cov6_fixed = True, None
    else:
        cov6_fixed = None if cov_moves else cov6_of()

    if lambdas_depth is not None:
        depth_target = depths.detach().float().to(dev).contiguous()
        depth_conf = None if depth_weights is None else depth_weights.detach().float().to(dev).contiguous()
    smooth_opacity = lambdas_smooth is not None and smooth.space == "expected"  # (the render space reads the depth map alone)
    if lambdas_smooth is not None:
        segment_ids = None if segments is None else segments.detach().to(dev).to(torch.int32).contiguous()
    want_aux = lambdas_depth is not None or bool(sparse) or smooth_opacity  # (it selects want_n_touched: off for the plain path)
    losses: List[float] = []
    depth_losses: List[float] = []
    smooth_losses: List[float] = []
    events: List[dict] = []
    prune_events: List[dict] = []
    classic = density is not None and not budgeted
    extent = None  # of the scene: one host read unless the control names it
    if (classic and free) or (means_lr_extent_scale and "means" in free):
        extent = float(density.scene_extent) if classic and density.scene_extent is not None else scene_extent(c2w)
    strategy = _Strategy()  # (no control, or nothing free: no events, no statistics, no extra steps)
    if density is not None and free:
        noise_gen = torch.Generator(device=dev).manual_seed(int(density.seed))  # the events' split noise, or their random words and every iteration's noise
        if classic:
            density.thresholds(extent)  # (a bad extent raises here, not at the first event)
            strategy = _Strategy(*density.events(int(iters)), stats=DensityStats(means.shape[0], dev, absgrad=density.absgrad))
        else:  # (a frozen field's regulariser term is a constant: neither added nor logged; frozen means take no noise)
            strategy = _Strategy(density.events(int(iters)), reg_o=float(density.opacity_reg) if "opacities" in free else 0.0,
                                 reg_s=float(density.scale_reg) if "scales" in free else 0.0, noise_lr=float(density.noise_lr) if "means" in free else 0.0)
    frozen = {}  # the frozen fields in the form the density / MCMC kernels read, each made when `unc` first asks for it

    def unc(k: str) -> torch.Tensor:
        """field k in unconstrained form: the free leaf, or a frozen field through log / logit, made when first asked for and kept (an event
        replaces it by its output).  Only an event and the MCMC regulariser / noise ask, so without a control nothing is ever computed here;
        `start`, which the render reads and the caller gets back, keeps the input's bits until the first event that runs (then, not before,
        frozen scales / opacities make their round trip)."""
        if k not in free and k not in frozen:
            frozen[k] = _TO_PARAM[k](start[k])
        return free[k].detach() if k in free else frozen[k]

    means_lrs = None  # the `means` rate per iteration, where it is not the constant lr["means"] (optimizer="hip" only: _check_optim_args)
    if "means" in free and (means_lr_final is not None or means_lr_extent_scale):
        lr_scale = extent if means_lr_extent_scale else 1.0
        means_lrs = means_lr_schedule(lr["means"] * lr_scale, (lr["means"] if means_lr_final is None else float(means_lr_final)) * lr_scale, int(iters))
    opt = None
    if free:
        free_lrs = {k: lr[k] for k in free}
        opt = GaussianAdam(free, free_lrs, eps=1e-15, sh_rest_lr_scale=float(sh_rest_lr_scale)) if hip else TorchAdam(free, free_lrs, eps=1e-15)

    def event(it: int):
        """one density event before iteration `it`'s render: all five fields in unconstrained form and the free ones' moments go through the
        strategy's one function (clone / split / prune, or relocate in place and grow); where it hands back new tensors they become the
        leaves and the optimiser moves to them (its step count stays); the frozen fields, cov6_fixed and the classic statistics follow"""
        nonlocal cov6_fixed, filter3d
        fields = {k: unc(k) for k in FIELDS}
        if classic:
            noise = torch.randn((strategy.stats.G, 2, 3), generator=noise_gen, device=dev, dtype=torch.float32)
            new_p, new_m, info = densify_and_prune(fields, opt.moments, strategy.stats, density, extent, noise)
            if info["rows_out"] == 0:
                raise RuntimeError(f"density control pruned every Gaussian at iteration {it}: {info}")
            strategy.stats = DensityStats(info["rows_out"], dev, absgrad=density.absgrad)
        else:
            new_p, new_m, info = mcmc_event(fields, opt.moments, density, generator=noise_gen)
        events.append(dict(info, iteration=it))
        if new_p is not fields:  # (MCMC with nothing to add keeps its leaves)
            adopt(new_p, new_m)
        frozen.update({k: new_p[k] for k in FIELDS if k not in free})
        start.update({k: _FROM_PARAM[k](v) for k, v in frozen.items()})
        cov6_fixed = None if cov_moves else cov6_of()
        filter3d = None  # (rows changed or moved)

    def adopt(new_p, new_m):
        """the new tensors of an event become the leaves and the optimiser moves to them (its step count stays)"""
        nonlocal free
        free = {k: new_p[k].requires_grad_(True) for k in free}
        opt.rebind(free, new_m)

    def prune_event(it: int):
        """one contribution-pruning event before iteration `it`'s render (after the last one: it == iters): the statistics of all training
        views under the current poses, then the row selection over all five fields and the free ones' moments, then event()'s hand-over"""
        nonlocal cov6_fixed, filter3d
        sc_v, op_v = filtered()
        stats = gaussian_contributions(value("means"), sc_v, value("rotations"), op_v, c2w if cam is None else cam.c2w, Kn, near_t,
                                       far_t, (H, W), **aa_kw)
        fields = {k: unc(k) for k in FIELDS}
        new_p, new_m, info = prune_by_contribution(fields, stats, prune.min_weight, prune.min_views, prune.keep_at_most, opt.moments if free else None)
        if info["rows_out"] == 0:
            raise RuntimeError(f"contribution pruning removed every Gaussian at iteration {it}: {info}")
        prune_events.append(dict(info, iteration=it))
        if free:
            adopt(new_p, new_m)
        frozen.update({k: new_p[k] for k in FIELDS if k not in free})
        start.update({k: _FROM_PARAM[k](v) for k, v in frozen.items()})
        cov6_fixed = None if cov_moves else cov6_of()
        filter3d = None  # (rows left)
        if strategy.stats is not None:
            strategy.stats = DensityStats(info["rows_out"], dev, absgrad=density.absgrad)

    def filtered(it: Optional[int] = None):
        """the scales and opacities the render takes: the fields' values, or with a 3-D filter those through mip.apply_filter3d, the filter
        recomputed first when an event dropped it or iteration `it` is one of its schedule"""
        nonlocal filter3d
        if not mip3d:
            return value("scales"), value("opacities")
        if filter3d is None or (it is not None and it % int(antialias.every) == 0):
            filter3d = compute_filter3d(value("means"), c2w if cam is None else cam.c2w, Kn, W, H, variance=float(antialias.variance_3d))
        return apply_filter3d(value("scales"), value("opacities"), filter3d)

    cam = cam_rates = None  # the cameras' state and their (lr_trans, lr_rot, lr_exposure) per iteration from cameras.start on
    grid_on = cameras is not None and exposure_mode(cameras.exposure) == "bilagrid"
    if cameras is not None and int(iters) > 0:
        cam = CameraState(c2w, cameras.pose, cameras.exposure, cameras.fixed, bilagrid_shape=cameras.bilagrid_shape)
        cam_rates = cameras.rates(int(iters))
        grid_rates = cameras.bilagrid_rates(int(iters)) if grid_on else None
    for it in range(int(iters) if free or cam is not None else 0):
        cam_on = cam is not None and it >= int(cameras.start)
        if not (free or cam_on):
            continue  # (frozen Gaussians before the cameras start: nothing moves)
        if cam_on:
            cam.zero_grad()
        if it in strategy.events:
            with torch.no_grad():
                event(it)
        if it in prune_at:
            with torch.no_grad():
                prune_event(it)
        if it in strategy.resets and "opacities" in free:
            with torch.no_grad():
                p = float(density.reset_opacity)
                free["opacities"].clamp_(max=math.log(p / (1.0 - p)))
                opt.zero_moments("opacities")
        if opt is not None:
            opt.zero_grad(set_to_none=True)
        if mip3d:
            scales_r, opac_r = filtered(it)
            cov6 = raster.quat_scale_to_cov6(torch.roll(value("rotations"), 1, dims=-1), scales_r)
        else:
            cov6, opac_r = cov6_of() if cov_moves else cov6_fixed, None  # (None: the field's own value, formed where it always was)
        pose_holders = dict(cam_rot_delta=cam.rot_delta, cam_trans_delta=cam.trans_delta) if cam_on and cam.pose else {}
        rendered = render_cuda(cam.c2w if cam_on else c2w, Kn, near_t, far_t, (H, W), bg_t, value("means")[None].expand(V, -1, -1), cov6[None].expand(V, -1, -1),
                               value("harmonics")[None].expand(V, -1, -1, -1), (value("opacities") if opac_r is None else opac_r)[None].expand(V, -1),
                               density_stats=strategy.stats, return_aux=want_aux, **pose_holders, **aa_kw)
        img, dep = rendered[0], rendered[1]
        if cam_on and cam.exposure:
            img = apply_exposure(img, cam.M)
        elif cam_on and grid_on:
            img = apply_bilagrid(img, cam.grids)
        opa = _aux_cat(rendered[2], "opacity") if lambdas_depth is not None or smooth_opacity else None
        radii = _aux_cat(rendered[2], "radii") if sparse else None
        if lambdas_depth is None:
            loss = photometric_loss(img, target, lambda_dssim)
        else:
            d_loss = depth_loss(dep, opa, depth_target, depth_conf, depth_mode, depth_space, depth_min_opacity)
            loss = photometric_loss(img, target, lambda_dssim) + lambdas_depth[it] * d_loss
        if lambdas_smooth is not None:
            s_loss = depth_smoothness(dep, opa if smooth_opacity else None, segment_ids, smooth.order, smooth.space, smooth.min_opacity)
            loss = loss + lambdas_smooth[it] * s_loss
        if cam_on and grid_on and float(cameras.lambda_tv) > 0.0:
            loss = loss + float(cameras.lambda_tv) * bilagrid_tv(cam.grids)
        loss.backward()
        if strategy.reg_o > 0.0 or strategy.reg_s > 0.0:
            reg = regularize(unc("opacities"), unc("scales"), strategy.reg_o, strategy.reg_s, free["opacities"].grad if strategy.reg_o > 0.0 else None,
                             free["scales"].grad if strategy.reg_s > 0.0 else None)
            loss = loss.detach() + reg.sum()
        if opt is not None:
            opt.step(visible=radii, lrs=None if means_lrs is None else {"means": means_lrs[it]})
        if cam_on:
            cam.step(cam.step_count + 1, cam_rates[it - int(cameras.start)], grid_rates[it - int(cameras.start)] if grid_on else None)
        if strategy.noise_lr > 0.0:
            scaler = strategy.noise_lr * (lr["means"] if means_lrs is None else means_lrs[it])
            noise = torch.randn((free["means"].shape[0], 3), generator=noise_gen, device=dev, dtype=torch.float32)
            inject_noise(unc("means"), unc("scales"), unc("rotations"), unc("opacities"), scaler, noise)
        if log_every and it % int(log_every) == 0:
            losses.append(float(loss.detach()))
            if lambdas_depth is not None:
                depth_losses.append(float(d_loss.detach()))
            if lambdas_smooth is not None:
                smooth_losses.append(float(s_loss.detach()))
    with torch.no_grad():
        if prune is not None and prune.final and int(iters) > 0:
            prune_event(int(iters))
        out = {k: value(k).detach().clone() for k in FIELDS}
        if mip3d:  # what the last render would use; the filter in the final row count (after a final pruning event: of the kept rows)
            out["covariances"] = covariances_from(out["rotations"], filtered()[0])
            out["filter_3d"] = filter3d.clone()
        else:
            out["covariances"] = covariances_from(out["rotations"], out["scales"])
        if density is not None:
            out["density_events"] = events
        if prune is not None:
            out["prune_events"] = prune_events
        if lambdas_depth is not None:
            out["depth_losses"] = depth_losses
        if lambdas_smooth is not None:
            out["smooth_losses"] = smooth_losses
        if hip:
            out["optimizer_steps"] = opt.step_count if free else 0
        if cameras is not None:
            out["c2w"] = cam.c2w.clone() if cam is not None else c2w.clone()
            out["exposure"] = cam.M.detach().clone() if cam is not None else torch.eye(3, 4, device=dev).repeat(V, 1, 1)
            out["camera_steps"] = cam.step_count if cam is not None else 0
            if grid_on:
                out["bilagrid"] = cam.grids.detach().clone() if cam is not None else identity_grids(V, cameras.bilagrid_shape, dev)
    return out, losses
