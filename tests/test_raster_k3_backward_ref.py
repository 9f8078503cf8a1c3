"""CPU checks of the float64 dense reference of the gsplat-family forward (tests/dense_gsplat64.py) that the K3 HIP backward is measured
against: its forward agrees with the C oracle's mode-1 forward and viewer helpers (oracle/raster_ref.c), and its autograd gradients agree
with float64 central differences, the world->camera matrix, quaternions / scales, SH and backgrounds included."""
import numpy as np
import pytest
import torch

import dense_gsplat64 as DG
from oracle import raster_oracle as RO
from scenes import default_K, look_at_camera, random_scene
from siu3r_amd import raster


def k3_cam(H, W, seed, near=0.2, far=1000.0, **kw):
    c2w = look_at_camera(seed)
    K = default_K()
    return raster.make_cam_k3(torch.linalg.inv(c2w), float(K[0, 0] * W), float(K[1, 1] * H), float(K[0, 2] * W), float(K[1, 2] * H), W, H,
                              near_plane=near, far_plane=far, **kw)


def _close(a, b):
    err = float((a.float() - torch.from_numpy(np.asarray(b))).abs().max())
    assert err <= 1e-5 * max(1.0, float(np.abs(b).max())), err


@pytest.mark.parametrize("seed,C", [(0, 3), (1, 7)])
def test_dense_reference_forward_matches_the_oracle(seed, C):
    H, W, G = 48, 64, 150
    cam = k3_cam(H, W, seed)
    means, cov, opac, _ = random_scene(G, seed=seed)
    cov6 = raster.cov6_from_cov3x3(cov)
    feats = torch.rand(G, C, generator=torch.Generator().manual_seed(seed)) * 2 - 0.5
    o = RO.forward(cam, means.numpy(), cov6.numpy(), opac.numpy(), feats.numpy())
    mask = DG.tile_mask_from_lists(o["tile_start"], o["ids"], G)
    assert mask.any(), "scene left the frame"
    col, alp = DG.render(cam, means, cov6, feats, opac, mask)
    _close(col, o["image"])
    _close(alp, o["alpha"])
    # the 3 x 3 covariance layout reads the same six entries
    col9, _ = DG.render(cam, means, cov, feats, opac, mask)
    assert float((col9 - col).abs().max()) == 0.0


@pytest.mark.parametrize("degree", [0, 2, 4])
def test_dense_reference_sh_route_matches_the_oracle(degree):
    """the viewer's argument list: quats + scales -> covariances, SH -> rgb, three-channel render, background blend"""
    H, W, G = 48, 64, 120
    cam = k3_cam(H, W, 2)
    g = torch.Generator().manual_seed(degree)
    means, _, opac, _ = random_scene(G, seed=4)
    quats = torch.randn(G, 4, generator=g) * 2.0  # not normalised: both sides normalise
    scales = 0.02 + 0.1 * torch.rand(G, 3, generator=g)
    sh = (torch.rand(G, 25, 3, generator=g) * 2 - 1) * 0.5
    campos = torch.linalg.inv(DG.cam_w2c(cam))[:3, 3].float()
    bg = torch.tensor([0.2, 0.5, 1.0])
    cov6_o = RO.quat_scale_to_cov6(quats.numpy(), scales.numpy())
    _close(DG.quat_scale_to_cov6(quats, scales), cov6_o)
    rgb_o = RO.sh_eval(degree, means.numpy(), campos.numpy(), sh.numpy())
    _close(DG.sh_eval(means, campos, sh, degree), rgb_o)
    o = RO.forward(cam, means.numpy(), cov6_o, opac.numpy(), rgb_o)
    mask = DG.tile_mask_from_lists(o["tile_start"], o["ids"], G)
    assert mask.any()
    col, alp = DG.render(cam, means, torch.from_numpy(cov6_o), torch.from_numpy(rgb_o), opac, mask, bg=bg)
    _close(col, RO.blend_background(o["image"], o["alpha"], bg.numpy()))
    _close(alp, o["alpha"])


def _check_fd(loss, args, tol=1e-5, eps=1e-6, dirs=3):
    grads = torch.autograd.grad(loss(*args), args)
    gen = torch.Generator().manual_seed(1)
    for i, (a, g) in enumerate(zip(args, grads)):
        for _ in range(dirs):
            d = torch.randn(a.shape, generator=gen, dtype=torch.float64)
            with torch.no_grad():
                ap = [x.detach() for x in args]
                ap[i] = a.detach() + eps * d
                lp = loss(*ap)
                ap[i] = a.detach() - eps * d
                lm = loss(*ap)
            fd = float((lp - lm) / (2 * eps))
            an = float((g * d).sum())
            assert abs(fd - an) <= tol * max(1.0, abs(fd)), (i, fd, an)


def _fixed_order(cam, means):
    with torch.no_grad():
        return DG.project(cam, means, torch.eye(3).expand(means.shape[0], 3, 3))[5].float()  # depth keys: the differences must not reorder


def test_dense_reference_gradients_match_central_differences():
    torch.manual_seed(0)
    H, W, G, C = 32, 32, 12, 5
    cam = k3_cam(H, W, 5)
    means, cov, opac, _ = random_scene(G, seed=7, scale=(0.05, 0.2), depth=(2.0, 4.0), spread=0.6)
    cov6 = raster.cov6_from_cov3x3(cov).double()
    opac = (opac * 0.5).double()  # away from the alpha_max clamp
    feats = torch.randn(G, C, dtype=torch.float64)
    mask = torch.ones((G, 4), dtype=torch.bool)
    key = _fixed_order(cam, means.double())
    w_c, w_a = torch.randn(H, W, C, dtype=torch.float64), torch.randn(H, W, dtype=torch.float64)

    def loss(m, c, f, o, vm, bg):
        col, a = DG.render(cam, m, c, f, o, mask, viewmat=vm, depth_key=key, bg=bg)
        return (col * w_c).sum() + (a * w_a).sum()

    args = [means.double().requires_grad_(), cov6.requires_grad_(), feats.requires_grad_(), opac.requires_grad_(),
            DG.cam_w2c(cam).requires_grad_(), torch.rand(C, dtype=torch.float64).requires_grad_()]
    _check_fd(loss, args)


def test_dense_reference_sh_route_gradients_match_central_differences():
    """quats / scales, SH of degree 3, the camera centre through inverse(viewmat), the background"""
    H, W, G = 32, 32, 10
    cam = k3_cam(H, W, 3)
    g = torch.Generator().manual_seed(2)
    means, _, opac, _ = random_scene(G, seed=9, depth=(2.0, 4.0), spread=0.6)
    quats = torch.randn(G, 4, generator=g, dtype=torch.float64)
    scales = 0.05 + 0.15 * torch.rand(G, 3, generator=g, dtype=torch.float64)
    sh = (torch.rand(G, 16, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.5
    opac = (opac * 0.5).double()
    mask = torch.ones((G, 4), dtype=torch.bool)
    key = _fixed_order(cam, means.double())
    w_c, w_a = torch.randn(H, W, 3, dtype=torch.float64), torch.randn(H, W, dtype=torch.float64)

    def loss(m, q, s, shc, vm, bg):
        rgb = DG.sh_eval(m, torch.linalg.inv(vm)[:3, 3], shc, 3)
        col, a = DG.render(cam, m, DG.quat_scale_to_cov6(q, s), rgb, opac, mask, viewmat=vm, depth_key=key, bg=bg)
        return (col * w_c).sum() + (a * w_a).sum()

    args = [means.double().requires_grad_(), quats.requires_grad_(), scales.requires_grad_(), sh.requires_grad_(),
            DG.cam_w2c(cam).requires_grad_(), torch.rand(3, dtype=torch.float64).requires_grad_()]
    _check_fd(loss, args)
