"""Float64 restatement of csrc/camera.hip with torch: the per-view exposure transform and its gradients (autograd), the se(3) exponential
(torch.linalg.matrix_exp of the hat matrix, as pose_align._se3_exp, and the closed form the kernel uses), and one camera step (Adam, then
the retraction c2w <- c2w exp(-xi^)).  `dtype` selects float64 (the reference) or float32 (the composed torch expression whose error sets
the tolerance of tests/test_exposure_gpu.py)."""
import math

import torch

SWITCH = 1e-2  # below this |theta| the closed form uses the three-term series of A, B and C


def exposure(img, M):
    """img [V,3,H,W], M [V,3,4] -> [V,3,H,W]"""
    return torch.einsum("vck,vkhw->vchw", M[:, :, :3], img) + M[:, :, 3, None, None]


def exposure_and_grads(img, M, g_out, dtype=torch.float64):
    """(out, g_img, g_M) of the transform for the upstream gradient g_out, evaluated in `dtype` on the CPU"""
    x = img.detach().cpu().to(dtype).requires_grad_(True)
    m = M.detach().cpu().to(dtype).requires_grad_(True)
    out = exposure(x, m)
    g_img, g_m = torch.autograd.grad(out, (x, m), g_out.detach().cpu().to(dtype))
    return out.detach(), g_img, g_m


def hat(xi):
    """xi [6] = (rho, theta) -> the 4 x 4 matrix xi^"""
    rho, th = xi[:3], xi[3:]
    h = torch.zeros((4, 4), dtype=xi.dtype)
    h[0, 1], h[0, 2], h[1, 2] = -th[2], th[1], -th[0]
    h[1, 0], h[2, 0], h[2, 1] = th[2], -th[1], th[0]
    h[:3, 3] = rho
    return h


def se3_exp(xi):
    """exp(xi^) [4,4] through the matrix exponential"""
    return torch.linalg.matrix_exp(hat(xi))


def se3_coefficients(th):
    """A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3 of a Python float, by their series below SWITCH"""
    t2 = th * th
    if th < SWITCH:
        return 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0
    return math.sin(th) / th, (1.0 - math.cos(th)) / t2, (th - math.sin(th)) / (t2 * th)


def se3_exp_closed(xi):
    """exp(xi^) [4,4] float64 in closed form: R = I + A K + B K^2, t = (I + B K + C K^2) rho"""
    xi = xi.double()
    rho, w = xi[:3], xi[3:]
    A, B, C = se3_coefficients(float(w.norm()))
    K = hat(torch.cat((torch.zeros(3, dtype=torch.float64), w)))[:3, :3]
    I = torch.eye(3, dtype=torch.float64)
    E = torch.eye(4, dtype=torch.float64)
    E[:3, :3] = I + A * K + B * (K @ K)
    E[:3, 3] = (I + B * K + C * (K @ K)) @ rho
    return E


def camera_step(c2w, M, g_xi, g_M, exp_avg, exp_avg_sq, free, t, lrs, betas=(0.9, 0.999), eps=1e-8, pose=True, exposure=True):
    """One step of siu3r_camera_step in float64 from the float32 state.  c2w [V,4,4], M [V,3,4], g_xi [V,6] = (rho, theta), g_M [V,3,4],
    moments [V,18] (6 pose, 12 exposure), free [V] (0 = the view keeps everything), t >= 1, lrs = (lr_trans, lr_rot, lr_exposure).
    Returns (c2w, M, exp_avg, exp_avg_sq, theta) in float64, theta [V] = the rotation angle of each view's update."""
    d = lambda x: x.detach().cpu().double().clone()
    c2w, M, m1, m2 = d(c2w), d(M), d(exp_avg), d(exp_avg_sq)
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    V = c2w.shape[0]
    theta = torch.zeros(V, dtype=torch.float64)

    def adam(g, sl, v, lr):
        m1[v, sl] = b1 * m1[v, sl] + (1.0 - b1) * g
        m2[v, sl] = b2 * m2[v, sl] + ((1.0 - b2) * g) * g
        return ((lr / bc1) * m1[v, sl]) / (m2[v, sl].sqrt() / math.sqrt(bc2) + eps)

    for v in range(V):
        if not bool(free[v]):
            continue
        if pose:
            lr = torch.tensor([lrs[0]] * 3 + [lrs[1]] * 3, dtype=torch.float64)
            u = adam(d(g_xi[v]), slice(0, 6), v, lr)  # u = -xi
            theta[v] = u[3:].norm()
            c2w[v] = c2w[v] @ se3_exp(u)
        if exposure:
            M[v] = M[v] - adam(d(g_M[v]).reshape(12), slice(6, 18), v, lrs[2]).reshape(3, 4)
    return c2w, M, m1, m2, theta
