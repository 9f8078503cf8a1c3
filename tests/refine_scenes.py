"""What the tests of refine.refine_gaussians (tests/test_refine*_gpu.py) share: the scene family, its cameras, a plain render and the PSNR."""
import torch

from scenes import default_K, look_at_camera, random_scene

H = W = 128
NEAR, FAR, BG = 0.5, 100.0, (0.0, 0.0, 0.0)
FIELDS = ("means", "scales", "rotations", "opacities", "harmonics")


def _truth(G=20000, seed=0, scale=(0.01, 0.12)):
    """random_scene's means / opacities / SH, with seeded scales and RAW (x, y, z, w) quaternions in place of its covariances"""
    means, _, opac, sh = random_scene(G, seed=seed, n_sh=4)
    g = torch.Generator().manual_seed(seed + 500)
    scales = scale[0] + torch.rand(G, 3, generator=g) * (scale[1] - scale[0])
    rot = torch.randn(G, 4, generator=g) * (0.5 + torch.rand(G, 1, generator=g))  # not normalised
    return dict(means=means.cuda(), scales=scales.cuda(), rotations=rot.cuda(), opacities=opac.cuda(), harmonics=sh.cuda())


def _cams(seeds):
    c2w = torch.stack([look_at_camera(seed=s) for s in seeds]).cuda()
    return c2w, default_K()[None].repeat(len(seeds), 1, 1).cuda()


def _render(c2w, K, means, cov, sh, opac, aux=False):
    from siu3r_amd.cuda_splatting import render_cuda

    V = c2w.shape[0]
    e = lambda x: x[None].expand(V, *x.shape)
    with torch.no_grad():
        return render_cuda(c2w, K, torch.full((V,), NEAR), torch.full((V,), FAR), (H, W), torch.zeros(V, 3), e(means), e(cov), e(sh), e(opac),
                           return_aux=aux)


def _psnr(a, b):
    from siu3r_amd import metrics

    return metrics.psnr(a.permute(1, 2, 0).cpu().numpy(), b.permute(1, 2, 0).cpu().numpy(), data_range=1.0)
