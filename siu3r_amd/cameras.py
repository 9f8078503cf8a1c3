"""The cameras of per-scene refinement: per-view pose and exposure as optimised state (csrc/camera.hip), the exposure
either one affine colour transform per view or a bilateral grid of them (csrc/bilagrid.hip).

The network is pose-free, so every camera refine.refine_gaussians receives is an estimate, and captured images differ in exposure and white
balance.  CameraControl says what moves and how fast; CameraState holds c2w [V,4,4], the per-view colour transform M [V,3,4]
(losses.apply_exposure), their Adam moments and the two gradient holders the K2 render fills, and steps all of it with ONE launch.

Conventions: the pose variable is xi = (rho, theta) = (translation, rotation) of a LEFT perturbation of world->camera, w2c <- exp(xi^) w2c,
taken at 0 (what render_cuda's cam_trans_delta / cam_rot_delta return the gradient of), re-centred after every step as
pose_align.align_pose does: c2w <- c2w exp(-xi^).  There is no CPU path and nothing here synchronises with the host."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import check
from .ops import _gpu, _p, _stream
from .optim import GaussianAdam, means_lr_schedule

EXPOSURE_MODES = ("affine", "bilagrid")


def exposure_mode(exposure) -> Optional[str]:
    """what CameraControl.exposure selects: "affine" (also True), "bilagrid", or None (False); an unknown string raises ValueError"""
    if isinstance(exposure, str):
        if exposure not in EXPOSURE_MODES:
            raise ValueError(f"CameraControl.exposure must be True, False or one of {EXPOSURE_MODES}, got {exposure!r}")
        return exposure
    return "affine" if exposure else None


def identity_grids(V: int, shape: Sequence[int], device) -> torch.Tensor:
    """[V,12,L,Gh,Gw] for shape = (Gh, Gw, L): channels 0, 5 and 10 one, the rest zero"""
    Gh, Gw, L = (int(n) for n in shape)
    g = torch.zeros((int(V), 12, L, Gh, Gw), device=device)
    g[:, (0, 5, 10)] = 1.0
    return g


@dataclass
class CameraControl:
    """Which camera parameters refine.refine_gaussians optimises next to the Gaussians, and how fast.

    pose / exposure switch the two halves.  `fixed` names the views that keep their pose and an identity exposure: joint optimisation of
    Gaussians and cameras has a 7-dof scene gauge (a similarity transform of everything) and a colour gauge against the SH coefficients;
    pinning one view removes both.  lr_trans / lr_rot step rho / theta, lr_exposure every entry of M; each rate decays log-linearly to
    lr_final_scale x itself over the iterations the cameras move (optim.means_lr_schedule).  start is the first iteration at which the
    cameras move; before it the loop is the one without a control.

    exposure is True or "affine" (one 3 x 4 matrix per view, losses.apply_exposure), "bilagrid" (per view a grid of such matrices over pixel
    position and luminance, losses.apply_bilagrid: what vignetting and tone curves need) or False.  Only "bilagrid" reads bilagrid_shape =
    (Gh, Gw, L), lr_bilagrid (the rate of every grid entry, decayed like the others: bilagrid_rates) and lambda_tv (the weight of
    losses.bilagrid_tv in the objective).

    The default rates are starting points, not tuned values: lr_rot and lr_trans are pose_align.align_pose's default step (3e-3), and
    lr_exposure is the exposure rate of the 3DGS training recipe (1e-2).  lr_bilagrid (2e-3) and lambda_tv (10) are, as far as recalled,
    the bilateral-grid defaults of gsplat's trainer without its warm-up.  Nobody has tuned any of them on real captures."""
    pose: bool = True
    exposure: Union[bool, str] = True
    fixed: Sequence[int] = (0,)
    lr_rot: float = 3e-3
    lr_trans: float = 3e-3
    lr_exposure: float = 1e-2
    lr_final_scale: float = 0.1
    start: int = 0
    bilagrid_shape: Tuple[int, int, int] = (16, 16, 8)
    lr_bilagrid: float = 2e-3
    lambda_tv: float = 10.0

    def validate(self, V: int):
        """raises ValueError for a control that cannot run on V views; no device work"""
        mode = exposure_mode(self.exposure)  # (an unknown string raises here)
        if not (self.pose or mode):
            raise ValueError("CameraControl: pose and exposure are both off (pass cameras=None for the loop without cameras)")
        fixed = [int(i) for i in self.fixed]
        bad = [i for i in fixed if not 0 <= i < int(V)]
        if bad:
            raise ValueError(f"CameraControl.fixed: view {bad} outside 0 .. {int(V) - 1}")
        if len(set(fixed)) >= int(V):
            raise ValueError(f"CameraControl.fixed names every one of the {int(V)} views: nothing is left to optimise")
        for name in ("lr_rot", "lr_trans", "lr_exposure", "lr_final_scale", "lr_bilagrid"):
            v = float(getattr(self, name))
            if not 0.0 < v < math.inf:
                raise ValueError(f"CameraControl.{name} must be positive and finite, got {getattr(self, name)!r}")
        if int(self.start) < 0:
            raise ValueError(f"CameraControl.start must be >= 0, got {self.start!r}")
        if not 0.0 <= float(self.lambda_tv) < math.inf:
            raise ValueError(f"CameraControl.lambda_tv must be finite and >= 0, got {self.lambda_tv!r}")
        shape = tuple(self.bilagrid_shape) if isinstance(self.bilagrid_shape, (tuple, list)) else ()
        if len(shape) != 3 or any(isinstance(n, bool) or not isinstance(n, int) for n in shape) or min(shape) < 2 or shape[2] > 16 or max(shape[:2]) > 1024:
            raise ValueError(f"CameraControl.bilagrid_shape must be three integers (Gh, Gw, L) with 2 <= Gh, Gw <= 1024 and 2 <= L <= 16, "
                             f"got {self.bilagrid_shape!r}")

    def rates(self, iters: int) -> List[Tuple[float, float, float]]:
        """(lr_trans, lr_rot, lr_exposure) of every iteration from `start` to iters - 1: entry i belongs to iteration start + i"""
        n = max(int(iters) - int(self.start), 0)
        cols = [means_lr_schedule(float(r), float(r) * float(self.lr_final_scale), n) for r in (self.lr_trans, self.lr_rot, self.lr_exposure)]
        return list(zip(*cols))

    def bilagrid_rates(self, iters: int) -> List[float]:
        """lr_bilagrid of every iteration from `start` to iters - 1, decayed as rates() decays the others"""
        return means_lr_schedule(float(self.lr_bilagrid), float(self.lr_bilagrid) * float(self.lr_final_scale), max(int(iters) - int(self.start), 0))


class CameraState:
    """c2w [V,4,4] and M [V,3,4] (identity) on the GPU with their Adam moments [V,18] (6 of the pose, 12 of the exposure), the per-view
    `free` bytes, and the zero-valued gradient holders rot_delta / trans_delta [V,3] to hand to render_cuda as cam_rot_delta /
    cam_trans_delta.  M is a leaf that requires grad when the affine exposure is on.  The caller's c2w is copied.

    exposure="bilagrid": `exposure` is False and `bilagrid` True; M stays an identity that takes no gradient, and `grids` [V,12,L,Gh,Gw]
    (bilagrid_shape = (Gh, Gw, L)) is an identity leaf stepped by an optim.GaussianAdam of its own (eps 1e-15) whose row mask is `free`, so
    a fixed view keeps the bits of its identity grid and of its moments; the one camera launch then steps the pose half only."""

    def __init__(self, c2w: torch.Tensor, pose: bool = True, exposure: Union[bool, str] = True, fixed: Sequence[int] = (0,),
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, bilagrid_shape: Tuple[int, int, int] = (16, 16, 8)):
        if not isinstance(c2w, torch.Tensor):
            raise TypeError(f"c2w must be a tensor, got {type(c2w).__name__}")
        _gpu(c2w)
        if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4) or c2w.shape[0] == 0:
            raise ValueError(f"c2w must be [V,4,4], got {tuple(c2w.shape)}")
        V, dev = int(c2w.shape[0]), c2w.device
        CameraControl(pose=pose, exposure=exposure, fixed=fixed, bilagrid_shape=bilagrid_shape).validate(V)
        mode = exposure_mode(exposure)
        self.V, self.device, self.pose, self.exposure, self.bilagrid = V, dev, bool(pose), mode == "affine", mode == "bilagrid"
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.c2w = c2w.detach().float().contiguous().clone()
        self.M = torch.eye(3, 4, device=dev).repeat(V, 1, 1).requires_grad_(self.exposure)
        self.exp_avg = torch.zeros((V, 18), device=dev)
        self.exp_avg_sq = torch.zeros((V, 18), device=dev)
        free = torch.ones(V, dtype=torch.uint8)
        for i in fixed:
            free[int(i)] = 0
        self.free = free.to(dev)
        self.rot_delta = torch.zeros((V, 3), device=dev, requires_grad=self.pose)
        self.trans_delta = torch.zeros((V, 3), device=dev, requires_grad=self.pose)
        self.step_count = 0
        self.grids = self.grid_opt = None
        if self.bilagrid:
            self.grids = identity_grids(V, bilagrid_shape, dev).requires_grad_(True)
            self.grid_opt = GaussianAdam({"bilagrid": self.grids}, {"bilagrid": 0.0}, betas=self.betas, eps=1e-15)

    def zero_grad(self):
        self.M.grad = self.rot_delta.grad = self.trans_delta.grad = None
        if self.bilagrid:
            self.grids.grad = None

    def step(self, t: int, rates: Tuple[float, float, float], lr_bilagrid: Optional[float] = None):
        """The one launch: Adam step number t (>= 1, the global count of the bias corrections) of the free views from the gradients the
        backward left in rot_delta / trans_delta / M, with rates = (lr_trans, lr_rot, lr_exposure); the pose is folded into c2w.
        With a bilateral grid its optimiser steps first (lr_bilagrid; one more launch, its own step count runs along with t)."""
        if self.bilagrid:
            if lr_bilagrid is None:
                raise ValueError("CameraState.step: the bilateral grid needs lr_bilagrid")
            self.grid_opt.step_count = int(t) - 1
            self.grid_opt.step(visible=self.free, lrs={"bilagrid": float(lr_bilagrid)})
            if not self.pose:
                self.step_count = int(t)
                return
        g_xi = g_m = None
        if self.pose:
            if self.rot_delta.grad is None or self.trans_delta.grad is None:
                raise RuntimeError("CameraState.step: the pose holders have no gradient (render with cam_rot_delta / cam_trans_delta and call backward)")
            g_xi = torch.cat((self.trans_delta.grad, self.rot_delta.grad), dim=1)
        if self.exposure:
            if self.M.grad is None:
                raise RuntimeError("CameraState.step: M has no gradient (pass the render through losses.apply_exposure and call backward)")
            g_m = self.M.grad.contiguous()
        lr_trans, lr_rot, lr_exposure = (float(r) for r in rates)
        with torch.cuda.device(self.device):
            check(_lib.lib().siu3r_camera_step(_p(self.c2w) if self.pose else None, _p(g_xi), _p(self.M.detach()) if self.exposure else None, _p(g_m),
                                               _p(self.exp_avg), _p(self.exp_avg_sq), _p(self.free), self.V, int(t), lr_trans, lr_rot, lr_exposure,
                                               self.betas[0], self.betas[1], self.eps, _stream()))
        self.step_count = int(t)
