"""The cameras of per-scene refinement: per-view pose and exposure as optimised state (csrc/camera.hip).

The network is pose-free, so every camera refine.refine_gaussians receives is an estimate, and captured images differ in exposure and white
balance.  CameraControl says what moves and how fast; CameraState holds c2w [V,4,4], the per-view colour transform M [V,3,4]
(losses.apply_exposure), their Adam moments and the two gradient holders the K2 render fills, and steps all of it with ONE launch.

Conventions: the pose variable is xi = (rho, theta) = (translation, rotation) of a LEFT perturbation of world->camera, w2c <- exp(xi^) w2c,
taken at 0 (what render_cuda's cam_trans_delta / cam_rot_delta return the gradient of), re-centred after every step as
pose_align.align_pose does: c2w <- c2w exp(-xi^).  There is no CPU path and nothing here synchronises with the host."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _gpu, _p, _stream
from .optim import means_lr_schedule


@dataclass
class CameraControl:
    """Which camera parameters refine.refine_gaussians optimises next to the Gaussians, and how fast.

    pose / exposure switch the two halves.  `fixed` names the views that keep their pose and an identity exposure: joint optimisation of
    Gaussians and cameras has a 7-dof scene gauge (a similarity transform of everything) and a colour gauge against the SH coefficients;
    pinning one view removes both.  lr_trans / lr_rot step rho / theta, lr_exposure every entry of M; each rate decays log-linearly to
    lr_final_scale x itself over the iterations the cameras move (optim.means_lr_schedule).  start is the first iteration at which the
    cameras move; before it the loop is the one without a control.

    The default rates are starting points, not tuned values: lr_rot and lr_trans are pose_align.align_pose's default step (3e-3), and
    lr_exposure is the exposure rate of the 3DGS training recipe (1e-2).  Nobody has tuned them on real captures."""
    pose: bool = True
    exposure: bool = True
    fixed: Sequence[int] = (0,)
    lr_rot: float = 3e-3
    lr_trans: float = 3e-3
    lr_exposure: float = 1e-2
    lr_final_scale: float = 0.1
    start: int = 0

    def validate(self, V: int):
        """raises ValueError for a control that cannot run on V views; no device work"""
        if not (self.pose or self.exposure):
            raise ValueError("CameraControl: pose and exposure are both off (pass cameras=None for the loop without cameras)")
        fixed = [int(i) for i in self.fixed]
        bad = [i for i in fixed if not 0 <= i < int(V)]
        if bad:
            raise ValueError(f"CameraControl.fixed: view {bad} outside 0 .. {int(V) - 1}")
        if len(set(fixed)) >= int(V):
            raise ValueError(f"CameraControl.fixed names every one of the {int(V)} views: nothing is left to optimise")
        for name in ("lr_rot", "lr_trans", "lr_exposure", "lr_final_scale"):
            v = float(getattr(self, name))
            if not 0.0 < v < math.inf:
                raise ValueError(f"CameraControl.{name} must be positive and finite, got {getattr(self, name)!r}")
        if int(self.start) < 0:
            raise ValueError(f"CameraControl.start must be >= 0, got {self.start!r}")

    def rates(self, iters: int) -> List[Tuple[float, float, float]]:
        """(lr_trans, lr_rot, lr_exposure) of every iteration from `start` to iters - 1: entry i belongs to iteration start + i"""
        n = max(int(iters) - int(self.start), 0)
        cols = [means_lr_schedule(float(r), float(r) * float(self.lr_final_scale), n) for r in (self.lr_trans, self.lr_rot, self.lr_exposure)]
        return list(zip(*cols))


class CameraState:
    """c2w [V,4,4] and M [V,3,4] (identity) on the GPU with their Adam moments [V,18] (6 of the pose, 12 of the exposure), the per-view
    `free` bytes, and the zero-valued gradient holders rot_delta / trans_delta [V,3] to hand to render_cuda as cam_rot_delta /
    cam_trans_delta.  M is a leaf that requires grad when exposure is on.  The caller's c2w is copied."""

    def __init__(self, c2w: torch.Tensor, pose: bool = True, exposure: bool = True, fixed: Sequence[int] = (0,),
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        if not isinstance(c2w, torch.Tensor):
            raise TypeError(f"c2w must be a tensor, got {type(c2w).__name__}")
        _gpu(c2w)
        if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4) or c2w.shape[0] == 0:
            raise ValueError(f"c2w must be [V,4,4], got {tuple(c2w.shape)}")
        V, dev = int(c2w.shape[0]), c2w.device
        CameraControl(pose=pose, exposure=exposure, fixed=fixed).validate(V)
        self.V, self.device, self.pose, self.exposure = V, dev, bool(pose), bool(exposure)
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

    def zero_grad(self):
        self.M.grad = self.rot_delta.grad = self.trans_delta.grad = None

    def step(self, t: int, rates: Tuple[float, float, float]):
        """The one launch: Adam step number t (>= 1, the global count of the bias corrections) of the free views from the gradients the
        backward left in rot_delta / trans_delta / M, with rates = (lr_trans, lr_rot, lr_exposure); the pose is folded into c2w."""
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
