"""Adaptive density control of per-scene refinement (Kerbl et al. 2023, section 5.2) on top of csrc/density.hip: Gaussians whose
screen-space position gradient is large are cloned when small and split when large, transparent or oversized ones are pruned, and the
Adam moments of every survivor are carried through.  The set keeps its memory order (an order-preserving scan places the output rows).

Everything here works on the UNCONSTRAINED parameters refine.refine_gaussians optimises: means [G,3], "scales" = log-scales [G,3],
"rotations" = raw (x, y, z, w) quaternions [G,4], "opacities" = logit opacities [G], harmonics [G,3,n]."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _gpu, _p, _stream

FIELDS = ("means", "scales", "rotations", "opacities", "harmonics")
PRUNE, KEEP, CLONE, SPLIT = 0, 1, 2, 3  # action codes of siu3r_density_plan; output rows = min(action, 2)
_COPY, _MEANS, _LOG_SCALES = 0, 1, 2    # modes of siu3r_density_apply


def _f32(x: float) -> float:
    """x rounded to float32 (what the kernel compares against), as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


class DensityStats:
    """The running statistics of G Gaussians between two density events: grad_accum [G] f32 (sum over the views that saw the Gaussian of
    the norm of its NDC-space mean gradient), seen [G] i32 (how many views did), max_radius [G] i32 (largest screen radius, pixels).
    Hand it to cuda_splatting.render_cuda / raster.rasterize_views_k2 as `density_stats`: the backward of that render accumulates into it.
    absgrad=True asks that backward for the absolute-gradient statistics of AbsGS (Ye et al. 2024): per view, the sums over the pixels of
    |the pixel's mean x term| and |its mean y term| (siu3r_raster_composite_rgb_bwd_abs) take the place of the signed mean gradient, so
    pulls of opposite sign on the two sides of a footprint add up where the signed sum cancels them.  `accumulate` is the same either way."""

    def __init__(self, G: int, device, absgrad: bool = False):
        self.G = int(G)
        self.absgrad = bool(absgrad)
        self.grad_accum = torch.zeros(self.G, dtype=torch.float32, device=device)
        self.seen = torch.zeros(self.G, dtype=torch.int32, device=device)
        self.max_radius = torch.zeros(self.G, dtype=torch.int32, device=device)

    def reset(self):
        self.grad_accum.zero_()
        self.seen.zero_()
        self.max_radius.zero_()

    def accumulate(self, g_mean2d: torch.Tensor, radii: torch.Tensor, sx: float, sy: float):
        """siu3r_density_accumulate.  g_mean2d [V,G,2] f32: the PIXEL-space mean gradient per view as siu3r_raster_project_bwd writes it
        (rows of culled Gaussians hold anything, NaN included: visibility is radii > 0); radii [V,G,2] i32.  Per visible (view, Gaussian),
        views in index order: grad_accum += hypot(sx gx, sy gy), seen += 1, max_radius = max(max_radius, radii).
        The rasterizer's backward passes sx = V W / 2, sy = V H / 2.  (W / 2, H / 2) turns the pixel gradient into the NDC gradient that
        3DGS thresholds (the convention means2D.grad has, INTEGRATION.md seam 2); V undoes the mean over the views that
        losses.photometric_loss takes, so that the 3DGS threshold 2e-4 keeps the meaning it has in a loop of one view per step."""
        _gpu(g_mean2d, radii, self.grad_accum)
        V = g_mean2d.shape[0]
        if tuple(g_mean2d.shape) != (V, self.G, 2) or tuple(radii.shape) != (V, self.G, 2):
            raise ValueError(f"density statistics of {self.G} Gaussians: g_mean2d {tuple(g_mean2d.shape)} / radii {tuple(radii.shape)} must be [V, {self.G}, 2]")
        if g_mean2d.dtype != torch.float32 or radii.dtype != torch.int32 or not g_mean2d.is_contiguous() or not radii.is_contiguous():
            raise ValueError("density statistics: g_mean2d must be contiguous float32 and radii contiguous int32")
        check(_lib.lib().siu3r_density_accumulate(_p(g_mean2d), _p(radii), V, self.G, float(sx), float(sy), _p(self.grad_accum), _p(self.seen),
                                                  _p(self.max_radius), _stream()))


def event_iterations(start: int, every: int, stop: Optional[int], iters: int, who: str) -> List[int]:
    """the schedule both controls share: start, start + every, ... up to and including stop (None: iters - every), never iteration 0 and
    never an iteration a run of `iters` iterations does not reach.  `who` names the control in the error for every <= 0."""
    if int(every) <= 0:
        raise ValueError(f"{who}.every must be positive, got {every}")
    stop = int(iters) - int(every) if stop is None else int(stop)
    return [i for i in range(int(start), min(stop, int(iters) - 1) + 1, int(every)) if i > 0]


@dataclass
class DensityControl:
    """When and how refine.refine_gaussians changes the set.  grad_threshold (on the average NDC-space position gradient), percent_dense
    (clone below / split above percent_dense x extent), min_opacity, the split factor 1.6 and reset_opacity are the published 3DGS
    values; the schedule (start, every, stop) is scaled to refine_gaussians' default iters = 200, where 3DGS runs 30,000 iterations and
    densifies every 100 from 500 to 15,000.

    max_screen_radius (pixels) and max_world_scale_frac (x extent; 3DGS uses 0.1 after its first reset) are extra prune rules, 0 = off.
    An event at iteration i runs BEFORE the render of iteration i, on the statistics of the iterations since the last event.
    stop = None means iters - every: no event so late that the new Gaussians get no steps.  reset_every > 0 resets the opacities to at
    most reset_opacity every that many iterations, up to `stop`.  max_gaussians caps growth: an event that would exceed it only prunes.
    scene_extent = None takes 1.1 x the largest distance of a camera centre from the centres' mean (the 3DGS cameras_extent).
    absgrad = True thresholds the absolute-gradient statistics (DensityStats(absgrad=True); AbsGS, Ye et al. 2024) in place of the signed
    ones: a large Gaussian over fine detail, whose per-pixel pulls cancel in the signed sum, then reaches the threshold and is split.
    The absolute sums are never smaller than the signed ones; gsplat pairs absgrad with a threshold of 8e-4.  grad_threshold is NOT
    changed automatically: pass it."""
    grad_threshold: float = 2e-4
    percent_dense: float = 0.01
    min_opacity: float = 0.005
    max_screen_radius: int = 0
    max_world_scale_frac: float = 0.0
    start: int = 100
    every: int = 100
    stop: Optional[int] = None
    reset_every: int = 0
    reset_opacity: float = 0.01
    max_gaussians: Optional[int] = None
    scene_extent: Optional[float] = None
    seed: int = 0
    absgrad: bool = False

    def events(self, iters: int) -> Tuple[List[int], List[int]]:
        """(iterations that densify, iterations that reset the opacities) of a run of `iters` iterations: start, start + every, ... up to
        and including stop; resets at the multiples of reset_every up to stop.  Iteration 0 has no statistics and no moments yet and is
        never an event; neither is an iteration the run does not reach."""
        densify = event_iterations(self.start, self.every, self.stop, iters, "DensityControl")
        stop = int(iters) - int(self.every) if self.stop is None else int(self.stop)  # (the resets stop where the events do)
        return densify, event_iterations(self.reset_every, self.reset_every, stop, iters, "DensityControl") if int(self.reset_every) > 0 else []

    def thresholds(self, extent: float) -> Dict[str, float]:
        """the float32 numbers the plan kernel compares against (computed once, on the host)"""
        extent = float(extent)
        if not math.isfinite(extent) or extent <= 0.0:
            raise ValueError(f"scene extent {extent}: must be positive and finite (pass DensityControl.scene_extent)")
        world = float(self.max_world_scale_frac) * extent
        return dict(grad_threshold=_f32(self.grad_threshold), log_dense_scale=_f32(math.log(float(self.percent_dense) * extent)),
                    logit_min_opacity=_f32(math.log(float(self.min_opacity) / (1.0 - float(self.min_opacity)))),
                    max_screen_radius=int(self.max_screen_radius), log_max_world_scale=_f32(math.log(world)) if world > 0.0 else math.inf)


def scene_extent(c2w: torch.Tensor) -> float:
    """1.1 x the largest distance of a camera centre (c2w [V,4,4], its translation column) from the centres' mean: the 3DGS cameras_extent.
    One camera, or cameras that share one centre, have no extent: that raises and asks for an explicit value."""
    centres = c2w.detach().double().cpu()[..., :3, 3].reshape(-1, 3)
    extent = 1.1 * float((centres - centres.mean(0, keepdim=True)).norm(dim=-1).max())
    if not math.isfinite(extent) or extent <= 0.0:
        raise ValueError(f"the camera centres span no extent ({extent}; {centres.shape[0]} camera(s)): pass DensityControl.scene_extent explicitly")
    return extent


def _rows(t: torch.Tensor, G: int, name: str) -> torch.Tensor:
    if t.shape[0] != G or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 tensor of {G} rows, got {tuple(t.shape)} {t.dtype}")
    return t


def _check_params(params, moments, G: Optional[int] = None) -> int:  # (the five FIELDS and the moments given: float32 GPU tensors of G rows)
    G = params["opacities"].shape[0] if G is None else G
    _gpu(*params.values())
    for k in FIELDS:
        _rows(params[k], G, k)
        if k in moments:
            _rows(moments[k][0], G, k + " exp_avg"), _rows(moments[k][1], G, k + " exp_avg_sq")
    return G


def plan(stats: DensityStats, log_scales: torch.Tensor, logit_opacity: torch.Tensor, grad_threshold: float, log_dense_scale: float,
         logit_min_opacity: float, max_screen_radius: int = 0, log_max_world_scale: float = math.inf, grow: bool = True):
    """siu3r_density_plan -> (action [G] i32, offset [G] i32, totals [4] i32 = rows out / pruned / cloned / split), all on the device; no
    host read.  The thresholds are compared as float32 (DensityControl.thresholds)."""
    G = stats.G
    _gpu(stats.grad_accum, log_scales, logit_opacity)
    _rows(log_scales, G, "log_scales"), _rows(logit_opacity, G, "logit_opacity")
    dev = log_scales.device
    lib = _lib.lib()
    action = torch.empty(G, dtype=torch.int32, device=dev)
    offset = torch.empty(G, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.siu3r_density_plan_ws(G)), 1), dtype=torch.int32, device=dev)
    totals = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib.siu3r_density_plan(_p(stats.grad_accum), _p(stats.seen), _p(stats.max_radius), _p(log_scales), _p(logit_opacity), G, float(grad_threshold),
                                 float(log_dense_scale), float(logit_min_opacity), int(max_screen_radius), float(log_max_world_scale), int(bool(grow)),
                                 _p(action), _p(offset), _p(ws), _p(totals), _stream()))
    return action, offset, totals


def apply(params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]], action: torch.Tensor, offset: torch.Tensor,
          rows_out: int, noise: torch.Tensor):
    """siu3r_density_apply, one launch per field of `params` (all five FIELDS, unconstrained), each carrying the field's two Adam moments
    when `moments` has them -> (new params, new moments) of `rows_out` rows."""
    G = action.shape[0]
    _gpu(action, offset, noise)
    _rows(noise, G, "noise")
    if tuple(noise.shape) != (G, 2, 3):
        raise ValueError(f"noise must be [G, 2, 3] unit normals, got {tuple(noise.shape)}")
    _check_params(params, moments, G)
    lib = _lib.lib()
    new_p, new_m = {}, {}
    for k in FIELDS:
        src = params[k]
        r = src[0].numel()
        dst = torch.empty((rows_out, *src.shape[1:]), dtype=torch.float32, device=src.device)
        m = moments.get(k)
        if m is not None:
            dm =(torch.empty_like(dst), torch.empty_like(dst))
            new_m[k] = dm
        new_p[k] = dst
        if rows_out == 0:
            continue
        mode = _MEANS if k == "means" else _LOG_SCALES if k == "scales" else _COPY
        check(lib.siu3r_density_apply(mode, _p(src), _p(m[0]) if m else None, _p(m[1]) if m else None, r, G, _p(action), _p(offset), _p(params["rotations"]),
                                      _p(params["scales"]), _p(noise), _p(dst), _p(dm[0]) if m else None, _p(dm[1]) if m else None, _stream()))
    return new_p, new_m


def densify_and_prune(params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]], stats: DensityStats,
                      control: DensityControl, extent: float, noise: Optional[torch.Tensor] = None):
    """One density event: one plan and one apply (eight launches) and ONE host read, the plan's totals, which size the outputs.
    params: the five FIELDS in unconstrained form (module docstring), free or frozen alike; moments: {field: (exp_avg, exp_avg_sq)} of the
    fields Adam moves (a frozen field has none and is gathered all the same: its kept and cloned rows are the source's bits).
    noise [G,2,3]: unit normals that place the two children of a split (None: drawn here from control.seed).
    If the planned size exceeds control.max_gaussians the event only prunes (the plan runs again with growth off; the number of pruned
    rows does not depend on it, so no second read is needed).
    Returns (new params, new moments, info = {"rows_in", "rows_out", "pruned", "kept", "cloned", "split", "capped"})."""
    G = stats.G
    thr = control.thresholds(extent)
    if noise is None:
        gen = torch.Generator(device=params["means"].device).manual_seed(int(control.seed))
        noise = torch.randn((G, 2, 3), generator=gen, device=params["means"].device, dtype=torch.float32)
    action, offset, totals = plan(stats, params["scales"], params["opacities"], grow=True, **thr)
    rows_out, pruned, cloned, split = (int(v) for v in totals.tolist())
    capped = control.max_gaussians is not None and rows_out > int(control.max_gaussians)
    if capped:
        action, offset, totals = plan(stats, params["scales"], params["opacities"], grow=False, **thr)
        rows_out, cloned, split = G - pruned, 0, 0
    new_p, new_m = apply(params, moments, action, offset, rows_out, noise)
    info = dict(rows_in=G, rows_out=rows_out, pruned=pruned, kept=G - pruned - cloned - split, cloned=cloned, split=split, capped=bool(capped))
    return new_p, new_m, info
