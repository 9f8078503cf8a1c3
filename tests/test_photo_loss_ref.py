"""Pins tests/dense_photo64.py, the reference of the GPU photometric-loss tests, on the CPU: its SSIM is metrics.ssim, its autograd gradient
agrees with central differences, and the closed-form derivative the HIP kernel implements agrees with autograd."""
import numpy as np
import pytest
import torch

from siu3r_amd import metrics

import dense_photo64 as D


@pytest.mark.parametrize("H,W", [(24, 37), (33, 33)])
@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("C", [1, 3])
def test_restated_ssim_is_metrics_ssim(H, W, data_range, C):
    g = torch.Generator().manual_seed(H * 100 + C)
    p = torch.rand(2, C, H, W, generator=g, dtype=torch.float64) * data_range
    t = (p + 0.2 * data_range * torch.randn(2, C, H, W, generator=g, dtype=torch.float64)).clamp(0, data_range)
    m = D.ssim_map(p, t, data_range)
    assert m.shape == (2, C, H - 10, W - 10)
    for v in range(2):
        ref = metrics.ssim(p[v].permute(1, 2, 0).numpy(), t[v].permute(1, 2, 0).numpy(), data_range=data_range)
        assert abs(float(m[v].mean()) - ref) <= 1e-12, (float(m[v].mean()), ref)


def test_autograd_gradient_agrees_with_central_differences():
    g = torch.Generator().manual_seed(5)
    p = torch.rand(1, 2, 14, 15, generator=g, dtype=torch.float64)
    t = torch.rand(1, 2, 14, 15, generator=g, dtype=torch.float64)
    for lam in (0.2, 1.0):
        _, grad = D.loss_and_grad(p, t, lam)
        h = 1e-6
        worst = 0.0
        for idx in [(0, 0, 0, 0), (0, 1, 7, 7), (0, 0, 13, 14), (0, 1, 3, 11), (0, 0, 6, 2)]:
            e = torch.zeros_like(p)
            e[idx] = h
            fd = (float(D.photo_loss(p + e, t, lam)[0]) - float(D.photo_loss(p - e, t, lam)[0])) / (2 * h)
            worst = max(worst, abs(fd - float(grad[idx])))
        assert worst <= 1e-8, worst


@pytest.mark.parametrize("flat", [False, True])
def test_closed_form_derivative_agrees_with_autograd(flat):
    g = torch.Generator().manual_seed(6)
    p = torch.rand(2, 3, 30, 41, generator=g, dtype=torch.float64)
    t = torch.rand(2, 3, 30, 41, generator=g, dtype=torch.float64)
    if flat:  # exactly flat regions: both clamps active
        p[:, :, :16, :20] = 0.5
        t[:, :, 8:, 15:] = 1.0
    _, grad = D.loss_and_grad(p, t, 1.0)  # loss = 1 - SSIM
    cf = D.closed_form_grad(p, t)
    assert float((cf + grad).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))
