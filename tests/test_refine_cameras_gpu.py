"""refine.refine_gaussians with cameras=CameraControl(...): per-view pose and exposure optimised next to (or instead of) the Gaussians.
The scene family is tests/refine_scenes.py at 128 x 128; where poses are involved the scene, the true camera and the perturbation are those
of test_raster_backward_gpu.py::test_align_pose_recovers_a_perturbed_camera."""
import math

import numpy as np
import pytest
import torch

from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _render, _truth
from scenes import random_scene

pytestmark = pytest.mark.gpu


def _pose_scene():
    """the align_pose test's Gaussians (seed 61, spread 1.5, scales 0.02 .. 0.1) in the form refine_gaussians takes"""
    G = 20000
    means, _, opac, sh = random_scene(G, seed=61, n_sh=4, spread=1.5, scale=(0.02, 0.1))
    g = torch.Generator().manual_seed(561)
    scales = 0.02 + torch.rand(G, 3, generator=g) * 0.08
    rot = torch.randn(G, 4, generator=g) * (0.5 + torch.rand(G, 1, generator=g))
    return dict(means=means.cuda(), scales=scales.cuda(), rotations=rot.cuda(), opacities=opac.cuda(), harmonics=sh.cuda())


def _xi0():
    axis = torch.tensor([0.3, -0.8, 0.5])
    axis = axis / axis.norm()
    return torch.cat((torch.tensor([0.03, -0.03, 0.029]), axis * math.radians(3.0))).cuda()


def _pose_errors(c2w, true):
    d = torch.linalg.inv(true) @ c2w
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (float(torch.trace(d[:3, :3])) - 1) / 2))))
    return ang, float((c2w[:3, 3] - true[:3, 3]).norm())


def _m_true(V, seed=7):
    """gains in 0.8 .. 1.2, off-diagonals and offsets up to 0.05, view 0 the identity"""
    g = torch.Generator().manual_seed(seed)
    M = torch.zeros(V, 3, 4)
    M[:, :, :3] = (torch.rand(V, 3, 3, generator=g) * 2 - 1) * 0.05
    for c in range(3):
        M[:, c, c] = 0.8 + 0.4 * torch.rand(V, generator=g)
    M[:, :, 3] = (torch.rand(V, 3, generator=g) * 2 - 1) * 0.05
    M[0] = torch.eye(3, 4)
    return M.cuda()


def test_cameras_none_is_the_call_without_the_keyword():
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.refine import refine_gaussians

    s = _truth(G=5000, seed=8)
    cams, K = _cams([0, 5])
    targets = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    for kw in (dict(iters=0), dict(iters=3, params=())):
        a, la = refine_gaussians(*(s[k] for k in FIELDS), targets, cams, K, NEAR, FAR, BG, **kw)
        b, lb = refine_gaussians(*(s[k] for k in FIELDS), targets, cams, K, NEAR, FAR, BG, cameras=None, **kw)
        assert la == lb == [] and set(a) == set(b) and "c2w" not in b
        for k in a:
            assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="both off"):
        refine_gaussians(*(s[k] for k in FIELDS), targets, cams, K, NEAR, FAR, BG, cameras=CameraControl(pose=False, exposure=False))
    # a control and iters = 0: nothing moves, the camera keys are there
    out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, cams, K, NEAR, FAR, BG, iters=0, cameras=CameraControl())
    assert losses == [] and torch.equal(out["c2w"], cams) and out["camera_steps"] == 0
    assert torch.equal(out["exposure"], torch.eye(3, 4).repeat(2, 1, 1).cuda())


def test_pose_only_alignment_against_frozen_gaussians():
    """V = 3, view 0 at its true pose and fixed, views 1 and 2 perturbed by the align_pose test's xi0 (3 degrees, 0.03) and by half of it;
    400 iterations of L1.  The yardstick is pose_align.align_pose on each perturbed view alone (400 iterations, lr 5e-3): every free view
    must end with rotation and translation error <= max(initial / 10, 2 x align_pose's final error for that view)."""
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.pose_align import _se3_exp, align_pose
    from siu3r_amd.refine import covariances_from, refine_gaussians

    s = _pose_scene()
    true, K = _cams([3, 0, 1])
    cov = covariances_from(s["rotations"], s["scales"])
    targets = _render(true, K, s["means"], cov, s["harmonics"], s["opacities"])[0]
    start = true.clone()
    start[1] = true[1] @ _se3_exp(_xi0())
    start[2] = true[2] @ _se3_exp(0.5 * _xi0())
    keep = start.clone()
    out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, start, K, NEAR, FAR, BG, iters=400, lambda_dssim=0.0, params=(), log_every=50,
                                   cameras=CameraControl(exposure=False, lr_rot=5e-3, lr_trans=5e-3))
    assert torch.equal(start, keep), "the caller's c2w was modified"
    assert out["camera_steps"] == 400 and len(losses) == 8 and all(np.isfinite(losses))
    assert torch.equal(out["c2w"][0], true[0]), "the fixed view moved"
    assert torch.equal(out["exposure"], torch.eye(3, 4).repeat(3, 1, 1).cuda())
    for k in FIELDS:
        assert torch.equal(out[k], s[k]), f"{k} is frozen and moved"
    for v in (1, 2):
        r0, t0 = _pose_errors(start[v], true[v])
        r1, t1 = _pose_errors(out["c2w"][v], true[v])
        alone, _ = align_pose(s["means"], cov, s["harmonics"], s["opacities"], targets[v], K[v], start[v], NEAR, FAR, BG, iters=400, lr=5e-3)
        ra, ta = _pose_errors(alone, true[v])
        print(f"\nview {v}: rotation {r0:.3f} -> {r1:.4f} deg (align_pose alone {ra:.4f}), translation {t0:.4f} -> {t1:.5f} (align_pose alone {ta:.5f}); "
              f"loss {losses[0]:.4f} -> {losses[-1]:.5f}")
        assert r1 <= max(r0 / 10, 2 * ra), (v, r0, r1, ra)
        assert t1 <= max(t0 / 10, 2 * ta), (v, t0, t1, ta)


def test_exposure_only_recovers_the_colour_transforms():
    """targets = M_true applied to the true render; 300 iterations with frozen Gaussians and poses: max |M - M_true| over the free views is at
    most a tenth of max |I - M_true|, and view 0's M is exactly the identity"""
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.losses import apply_exposure
    from siu3r_amd.refine import covariances_from, refine_gaussians

    s = _truth()
    cams, K = _cams([0, 1, 2, 3])
    cov = covariances_from(s["rotations"], s["scales"])
    M_true = _m_true(4)
    targets = apply_exposure(_render(cams, K, s["means"], cov, s["harmonics"], s["opacities"])[0], M_true)
    control = CameraControl(pose=False)
    out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, cams, K, NEAR, FAR, BG, iters=300, params=(), log_every=50, cameras=control)
    eye = torch.eye(3, 4).cuda()
    err = float((out["exposure"][1:] - M_true[1:]).abs().max())
    off = float((eye - M_true[1:]).abs().max())
    print(f"\nexposure only, lr_exposure {control.lr_exposure:g}: max |M - M_true| {err:.5f}, max |I - M_true| {off:.5f}; loss {losses[0]:.5f} -> {losses[-1]:.6f}")
    assert torch.equal(out["exposure"][0], eye), "the fixed view's exposure is not exactly the identity"
    assert torch.equal(out["c2w"], cams) and out["camera_steps"] == 300
    assert err <= off / 10


@pytest.fixture(scope="module")
def joint():
    """Gaussians perturbed as the "appearance" variant of test_refinement_recovers_perturbed_gaussians, the poses of views 1-3 by
    1 degree / 0.01, and targets that carry a per-view exposure"""
    from siu3r_amd.losses import apply_exposure
    from siu3r_amd.pose_align import _se3_exp
    from siu3r_amd.refine import covariances_from

    truth = _truth()
    true, K = _cams([0, 1, 2, 3])
    cov = covariances_from(truth["rotations"], truth["scales"])
    targets = apply_exposure(_render(true, K, truth["means"], cov, truth["harmonics"], truth["opacities"])[0], _m_true(4))
    g = torch.Generator().manual_seed(77)
    n = lambda *s: torch.randn(*s, generator=g).cuda()
    G = truth["means"].shape[0]
    start = dict(truth)
    start["harmonics"] = truth["harmonics"] + 0.15 * n(G, 3, 4)
    start["opacities"] = torch.sigmoid(torch.logit(truth["opacities"]) + 0.7 * n(G))
    start["scales"] = torch.exp(torch.log(truth["scales"]) + 0.2 * n(G, 3))
    start = {k: v.clone() for k, v in start.items()}
    c2w = true.clone()
    for v in (1, 2, 3):
        axis = torch.randn(3, generator=g)
        xi = torch.cat((0.01 * torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0), math.radians(1.0) * axis / axis.norm())).cuda()
        c2w[v] = true[v] @ _se3_exp(xi)
    return dict(start=start, c2w=c2w, K=K, targets=targets, true=true)


def _run(j, **kw):
    from siu3r_amd.refine import refine_gaussians

    return refine_gaussians(*(j["start"][k] for k in FIELDS), j["targets"], j["c2w"], j["K"], NEAR, FAR, BG, iters=60, params=("scales", "opacities", "harmonics"), **kw)


def test_joint_refinement_beats_the_run_without_cameras(joint):
    from siu3r_amd.cameras import CameraControl

    keep = {k: v.clone() for k, v in joint["start"].items()}
    keep_c2w = joint["c2w"].clone()
    _, plain = _run(joint)
    out, losses = _run(joint, cameras=CameraControl())
    print(f"\njoint, 60 iterations: loss without cameras {plain[0]:.5f} -> {plain[-1]:.5f}, with {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert len(losses) == len(plain) == 60 and all(np.isfinite(losses)) and all(np.isfinite(plain))
    assert losses[-1] < plain[-1]
    for k in FIELDS:
        assert torch.equal(joint["start"][k], keep[k]), f"input {k} was modified"
    assert torch.equal(joint["c2w"], keep_c2w), "the caller's c2w was modified"
    assert out["c2w"].shape == (4, 4, 4) and out["exposure"].shape == (4, 3, 4) and out["camera_steps"] == 60
    assert torch.equal(out["c2w"][0], joint["c2w"][0]) and torch.equal(out["exposure"][0], torch.eye(3, 4).cuda())
    assert not torch.equal(out["c2w"][1:], joint["c2w"][1:]) and not torch.equal(out["exposure"][1], torch.eye(3, 4).cuda())


@pytest.mark.parametrize("variant", ["density", "hip_sparse", "depth_late_start"])
def test_joint_refinement_with_the_other_keywords(joint, variant):
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.density import DensityControl

    control = CameraControl()
    if variant == "density":
        kw = dict(density=DensityControl(start=20, every=20))
    elif variant == "hip_sparse":
        kw = dict(optimizer="hip", sparse=True)
    else:  # a depth term on the render's own depth / opacity, and cameras that start late
        control = CameraControl(start=30)
        kw = dict(depths=torch.full((4, H, W), 3.0).cuda(), lambda_depth=0.1)
    out, losses = _run(joint, cameras=control, **kw)
    rows = {out[k].shape[0] for k in FIELDS} | {out["covariances"].shape[0]}
    print(f"\njoint + {variant}: loss {losses[0]:.5f} -> {losses[-1]:.5f}, {rows} rows, {out['camera_steps']} camera steps")
    assert len(rows) == 1 and all(np.isfinite(losses)) and len(losses) == 60
    assert out["camera_steps"] == (30 if variant == "depth_late_start" else 60)
    assert out["c2w"].shape == (4, 4, 4) and torch.isfinite(out["c2w"]).all() and torch.isfinite(out["exposure"]).all()
    if variant == "density":
        assert len(out["density_events"]) == 2
    if variant == "hip_sparse":
        assert out["optimizer_steps"] == 60
