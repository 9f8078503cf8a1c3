"""CPU checks of the float64 dense reference (tests/dense_raster64.py) that the HIP backward is measured against: its forward agrees with
the C oracle of the K2 forward (oracle/raster_ref.c) and its autograd gradients agree with float64 central differences."""
import numpy as np
import pytest
import torch

import dense_raster64 as DR
from oracle import raster_oracle as RO
from scenes import default_K, look_at_camera, random_scene
from siu3r_amd import cuda_splatting as cs
from siu3r_amd import raster


def _cam(H, W, seed, degree, band4=False):
    c2w = look_at_camera(seed)
    K = default_K()[None]
    fov = cs.get_fov(K)
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([0.2]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(c2w)
    return raster.make_cam_k2(w2c, proj @ w2c, float(tan[0]), float(tan[1]), c2w[:3, 3].tolist(), [0.1, 0.2, 0.3], W, H, sh_degree=degree,
                              sh_band4=band4)


@pytest.mark.parametrize("seed,degree", [(0, 0), (1, 1), (2, 3)])
def test_dense_reference_forward_matches_the_oracle(seed, degree):
    H, W, G = 48, 64, 150
    cam = _cam(H, W, seed, degree)
    means, cov, opac, sh = random_scene(G, seed=seed, n_sh=16)
    cov6 = raster.cov6_from_cov3x3(cov)
    sh_i = sh.permute(0, 2, 1).contiguous()  # [G, 16, 3]
    o = RO.forward(cam, means.numpy(), cov6.numpy(), opac.numpy(), sh_i.numpy())
    mask = DR.tile_mask_from_lists(o["tile_start"], o["ids"], G)
    assert mask.any(), "scene left the frame"
    img, dep, alp = DR.render(cam, means, cov6, sh_i, opac, mask)
    for a, b in ((img, o["image"]), (dep, o["depth"]), (alp, o["alpha"])):
        err = float((a.float() - torch.from_numpy(b)).abs().max())
        assert err <= 1e-5 * max(1.0, float(np.abs(b).max())), err


def test_dense_reference_gradients_match_central_differences():
    torch.manual_seed(0)
    H, W, G = 32, 32, 12
    cam = _cam(H, W, 5, 3)
    means, cov, opac, sh = random_scene(G, seed=7, n_sh=16, scale=(0.05, 0.2), depth=(2.0, 4.0), spread=0.6)
    cov6 = raster.cov6_from_cov3x3(cov).double()
    sh_i = sh.permute(0, 2, 1).contiguous().double()
    opac = (opac * 0.5).double()  # away from the alpha_max clamp
    mask = torch.ones((G, 4), dtype=torch.bool)
    w_img, w_d, w_o = torch.randn(3, H, W, dtype=torch.float64), torch.randn(H, W, dtype=torch.float64), torch.randn(H, W, dtype=torch.float64)
    key = None
    with torch.no_grad():
        m0 = means.double()
        pc = m0 @ DR.cam_tensors(cam)[0][:3, :3].T + DR.cam_tensors(cam)[0][:3, 3]
        key = pc[:, 2].float()  # a fixed order: the finite differences must not reorder the splats

    def loss(m, c, s, o, xi):
        img, d, a = DR.render(cam, m, c, s, o, mask, xi=xi, depth_key=key)
        return (img * w_img).sum() + (d * w_d).sum() + (a * w_o).sum()

    args = [means.double().requires_grad_(), cov6.requires_grad_(), sh_i.requires_grad_(), opac.requires_grad_(),
            torch.zeros(6, dtype=torch.float64, requires_grad=True)]
    grads = torch.autograd.grad(loss(*args), args)
    gen = torch.Generator().manual_seed(1)
    for i, (a, g) in enumerate(zip(args, grads)):
        for _ in range(3):
            d = torch.randn(a.shape, generator=gen, dtype=torch.float64)
            eps = 1e-6
            with torch.no_grad():
                ap = [x.detach() for x in args]
                ap[i] = a.detach() + eps * d
                lp = loss(*ap)
                ap[i] = a.detach() - eps * d
                lm = loss(*ap)
            fd = float((lp - lm) / (2 * eps))
            an = float((g * d).sum())
            assert abs(fd - an) <= 1e-5 * max(1.0, abs(fd)), (i, fd, an)
