"""refine.refine_gaussians: per-scene refinement of the Gaussians through the HIP render, its backward and the fused photometric loss."""
import numpy as np
import pytest
import torch

from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _psnr, _render, _truth

pytestmark = pytest.mark.gpu


def _host_covariances(rotations_xyzw, scales):
    """R(q / |q|) diag(scales^2) R^T on the host with the `Gaussians.rotations` convention (x, y, z, w): numpy float32 (correctly rounded
    divide and square root), written in the operation order of the library's quaternion kernel so that the two agree to the bit"""
    q, s = rotations_xyzw.cpu().numpy().astype(np.float32), scales.cpu().numpy().astype(np.float32)
    x, y, z, w = (q[:, k] for k in range(4))
    one, two = np.float32(1), np.float32(2)
    inv = one / np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w * inv, x * inv, y * inv, z * inv
    x2, y2, z2, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [one - two * (y2 + z2), two * (xy - wz), two * (xz + wy), two * (xy + wz), one - two * (x2 + z2), two * (yz - wx),
         two * (xz - wy), two * (yz + wx), one - two * (x2 + y2)]
    M = [[R[3 * r + k] * s[:, k] for k in range(3)] for r in range(3)]
    cov = np.empty((len(s), 3, 3), np.float32)
    for r in range(3):
        for c in range(3):
            a, b = min(r, c), max(r, c)
            cov[:, r, c] = M[a][0] * M[b][0] + M[a][1] * M[b][1] + M[a][2] * M[b][2]
    return torch.from_numpy(cov)


@pytest.mark.parametrize("variant", ["appearance", "everything"])
def test_refinement_recovers_perturbed_gaussians(variant):
    from siu3r_amd.refine import covariances_from, refine_gaussians

    truth = _truth()
    train, Kt = _cams([0, 1, 2, 3])
    held, Kh = _cams([4])
    cov_true = covariances_from(truth["rotations"], truth["scales"])
    targets = _render(train, Kt, truth["means"], cov_true, truth["harmonics"], truth["opacities"])[0]
    held_target = _render(held, Kh, truth["means"], cov_true, truth["harmonics"], truth["opacities"])[0][0]
    g = torch.Generator().manual_seed(77)
    n = lambda *s: torch.randn(*s, generator=g).cuda()
    G = truth["means"].shape[0]
    start = dict(truth)
    start["harmonics"] = truth["harmonics"] + 0.15 * n(G, 3, 4)
    start["opacities"] = torch.sigmoid(torch.logit(truth["opacities"]) + 0.7 * n(G))
    start["scales"] = torch.exp(torch.log(truth["scales"]) + 0.2 * n(G, 3))
    start = {k: v.clone() for k, v in start.items()}
    keep = {k: v.clone() for k, v in start.items()}
    params = ("scales", "opacities", "harmonics") if variant == "appearance" else FIELDS
    before = _psnr(_render(held, Kh, start["means"], covariances_from(start["rotations"], start["scales"]), start["harmonics"], start["opacities"])[0][0],
                   held_target)
    out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=60, params=params)
    after = _psnr(_render(held, Kh, out["means"], out["covariances"], out["harmonics"], out["opacities"])[0][0], held_target)
    print(f"\nrefine ({variant}): training loss {losses[0]:.5f} -> {losses[-1]:.5f}, held-out PSNR {before:.3f} -> {after:.3f} dB")
    assert len(losses) == 60 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert after > before
    for k in FIELDS:
        assert torch.equal(start[k], keep[k]), f"input {k} was modified"
        assert start[k].grad is None and not start[k].requires_grad
        assert out[k].data_ptr() != start[k].data_ptr() and out[k].shape == start[k].shape
        if k in params:
            assert not torch.equal(out[k], start[k]), f"{k} is free and did not move"
        else:
            assert torch.equal(out[k], start[k]), f"{k} is frozen and moved"
    assert out["covariances"].shape == (G, 3, 3) and torch.equal(out["covariances"], covariances_from(out["rotations"], out["scales"]))


def test_one_sh_step_moves_only_what_the_render_touched():
    from siu3r_amd.refine import covariances_from, refine_gaussians

    s = _truth(seed=3)
    train, Kt = _cams([0, 1, 2, 3])
    targets = torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    _, _, aux = _render(train, Kt, s["means"], covariances_from(s["rotations"], s["scales"]), s["harmonics"], s["opacities"], aux=True)
    radii = torch.cat([a["radii"] for a in aux])  # [V,G,2]
    touched = (radii > 0).any(-1).any(0)
    out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=1, lambda_dssim=0.0, params=("harmonics",))
    moved = (out["harmonics"] != s["harmonics"]).flatten(1).any(1)
    print(f"\none SH step: {int(moved.sum())} Gaussians moved, {int(touched.sum())} of {len(touched)} touched by the render")
    assert len(losses) == 1 and int(moved.sum()) > 0
    assert not bool((moved & ~touched).any())
    for k in ("means", "scales", "rotations", "opacities"):
        assert torch.equal(out[k], s[k])


def test_quaternion_order_of_the_returned_covariances():
    """strongly anisotropic Gaussians: a (w, x, y, z) / (x, y, z, w) mix-up turns every splat"""
    from siu3r_amd.refine import refine_gaussians

    s = _truth(G=5000, seed=8, scale=(0.005, 0.25))
    cams, K = _cams([0, 5])
    targets = torch.zeros(2, 3, H, W).cuda()
    out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, cams, K, NEAR, FAR, BG, iters=0)
    assert losses == [] and all(torch.equal(out[k], s[k]) for k in FIELDS)
    host = _host_covariances(s["rotations"], s["scales"]).cuda()
    a = _render(cams, K, s["means"], out["covariances"], s["harmonics"], s["opacities"])[0]
    b = _render(cams, K, s["means"], host, s["harmonics"], s["opacities"])[0]
    wrong = _host_covariances(torch.roll(s["rotations"], 1, dims=-1), s["scales"]).cuda()  # the quaternions read as (w, x, y, z)
    c = _render(cams, K, s["means"], wrong, s["harmonics"], s["opacities"])[0]
    print(f"\ncovariances kernel vs host: max |d| {float((out['covariances'] - host).abs().max()):.3e}; image max |d| {float((a - b).abs().max()):.3e}; "
          f"with the other quaternion order {float((a - c).abs().max()):.3e}")
    assert float(a.abs().max()) > 0.05 and float((a - c).abs().max()) > 0.05
    assert torch.equal(a, b)
