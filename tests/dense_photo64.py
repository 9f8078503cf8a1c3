"""Dense restatement of the photometric loss (siu3r_amd/losses.py, csrc/photo_loss.hip) in plain torch: depthwise conv2d with the window of
metrics._gauss1d, autograd for the gradient.  float64 is the reference of the GPU tests, float32 (`dtype=`) the 'composed torch loss' their
tolerance is taken from; closed_form_grad is the derivative the kernel implements, checked against autograd on the CPU."""
import torch
import torch.nn.functional as F

from siu3r_amd.metrics import _gauss1d

K1, K2, TAPS = 0.01, 0.03, 11


def _blur(x, g):
    """valid separable 11-tap convolution of [V,C,H,W] per channel"""
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def _window(like):
    return torch.from_numpy(_gauss1d(TAPS, 1.5)).to(device=like.device, dtype=like.dtype)


def ssim_map(pred, target, data_range=1.0):
    """[V,C,H-10,W-10] SSIM of every valid window (variances clamped at 0)"""
    g = _window(pred)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu_p, mu_t = _blur(pred, g), _blur(target, g)
    s_pp = (_blur(pred * pred, g) - mu_p * mu_p).clamp_min(0)
    s_tt = (_blur(target * target, g) - mu_t * mu_t).clamp_min(0)
    s_pt = _blur(pred * target, g) - mu_p * mu_t
    return ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))


def photo_loss(pred, target, lam=0.2, data_range=1.0):
    """(loss, L1, SSIM) of [V,C,H,W] tensors in their own dtype; a term that lam switches off is None"""
    l1 = (pred - target).abs().mean() if lam != 1 else None
    ss = ssim_map(pred, target, data_range).mean() if lam != 0 else None
    loss = 0
    if l1 is not None:
        loss = loss + (1 - lam) * l1
    if ss is not None:
        loss = loss + lam * (1 - ss)
    return loss, l1, ss


def loss_and_grad(pred, target, lam=0.2, data_range=1.0, dtype=torch.float64):
    """the inputs converted to `dtype` (an upcast of float32 inputs is exact) -> ((loss, L1, SSIM) as floats or None, d loss / d pred)"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    t = target.detach().to(dtype)
    loss, l1, ss = photo_loss(p, t, lam, data_range)
    (g,) = torch.autograd.grad(loss, p)
    f = lambda x: None if x is None else float(x.detach())
    return (f(loss), f(l1), f(ss)), g


def closed_form_grad(pred, target, data_range=1.0):
    """d mean(SSIM map) / d pred without autograd: the three derivative maps per window and their transposed blur"""
    g = _window(pred)
    C = pred.shape[1]
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu_p, mu_t = _blur(pred, g), _blur(target, g)
    spp_raw = _blur(pred * pred, g) - mu_p * mu_p
    s_pp, s_tt = spp_raw.clamp_min(0), (_blur(target * target, g) - mu_t * mu_t).clamp_min(0)
    s_pt = _blur(pred * target, g) - mu_p * mu_t
    A1, A2, B1, B2 = 2 * mu_p * mu_t + c1, 2 * s_pt + c2, mu_p * mu_p + mu_t * mu_t + c1, s_pp + s_tt + c2
    d_epp = -A1 * A2 / (B1 * B2 * B2) * (spp_raw > 0)
    d_ept = 2 * A1 / (B1 * B2)
    d_mu = 2 * mu_t * A2 / (B1 * B2) - 2 * mu_p * A1 * A2 / (B1 * B1 * B2) - 2 * mu_p * d_epp - mu_t * d_ept

    def blur_t(x):
        x = F.conv_transpose2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)
        return F.conv_transpose2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)

    return (blur_t(d_mu) + 2 * pred * blur_t(d_epp) + target * blur_t(d_ept)) / d_mu.numel()
