"""Test-time pose alignment: refine one target camera against its image with the Gaussians frozen (how novel-view synthesis of pose-free
feed-forward splatting is usually evaluated).  The render and its pose gradient are the HIP rasterizer's (cuda_splatting.render_cuda with
cam_rot_delta / cam_trans_delta); the small se(3) bookkeeping around it is plain torch on 4 x 4 matrices."""
from __future__ import annotations

import math
from typing import List, Tuple

import torch

from .cuda_splatting import render_cuda


def _se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """xi [6] = (rho, theta) -> exp(xi^) [4,4]"""
    rho, th = xi[:3], xi[3:]
    hat = torch.zeros((4, 4), dtype=xi.dtype, device=xi.device)
    hat[0, 1], hat[0, 2], hat[1, 2] = -th[2], th[1], -th[0]
    hat[1, 0], hat[2, 0], hat[2, 1] = th[2], -th[1], th[0]
    hat[:3, 3] = rho
    return torch.linalg.matrix_exp(hat)


def align_pose(means, cov, sh, opacities, image, Kn, c2w_init, near, far, bg, iters: int = 100, lr: float = 3e-3
               ) -> Tuple[torch.Tensor, List[float]]:
    """means [G,3], cov [G,3,3], sh [G,3,n] (n = (deg+1)^2 coefficients per channel), opacities [G]: the frozen Gaussians (GPU).
    image [3,H,W]: the target view; Kn [3,3] normalised intrinsics; c2w_init [4,4] camera-to-world start pose (GPU); near / far floats;
    bg 3 floats.  Photometric L1, Adam (step decayed to a tenth over the iterations) on xi = (rho, theta) of a left perturbation of world->camera, folded into the pose after every
    step (w2c <- exp(xi^) w2c, i.e. c2w <- c2w exp(-xi^)) and reset to 0.  Returns (refined c2w [4,4], loss of every iteration)."""
    dev = means.device
    H, W = image.shape[-2:]
    c2w = c2w_init.detach().float().clone().to(dev)
    Kn = Kn.detach().float().to(dev)[None]
    near_t, far_t = torch.tensor([float(near)]), torch.tensor([float(far)])
    bg_t = torch.tensor([[float(b) for b in bg]])
    m, c, s, o = (t.detach()[None] for t in (means, cov, sh, opacities))
    target = image.detach().float().to(dev)
    rot = torch.zeros((1, 3), device=dev, requires_grad=True)
    trans = torch.zeros((1, 3), device=dev, requires_grad=True)
    opt = torch.optim.Adam([rot, trans], lr=lr)
    # cosine decay of the step to a tenth: the final pose settles instead of oscillating at the scale of lr
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 0.1 + 0.45 * (1 + math.cos(math.pi * min(i, iters) / max(1, iters))))
    losses = []
    for _ in range(int(iters)):
        opt.zero_grad(set_to_none=True)
        img, _ = render_cuda(c2w[None], Kn, near_t, far_t, (H, W), bg_t, m, c, s, o, cam_rot_delta=rot, cam_trans_delta=trans)
        loss = (img[0] - target).abs().mean()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            xi = torch.cat((trans[0], rot[0]))
            c2w = c2w @ _se3_exp(-xi)
            rot.zero_()
            trans.zero_()
    return c2w, losses
