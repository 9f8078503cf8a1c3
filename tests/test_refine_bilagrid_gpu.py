"""refine.refine_gaussians with cameras=CameraControl(exposure="bilagrid"): a per-view bilateral grid of colour transforms optimised next to
(or instead of) the Gaussians.  The scene family is tests/refine_scenes.py at 128 x 128 with 4 views; the targets are true renders passed
through a known smooth grid per free view by the float64 reference (dense_bilagrid64.explicit)."""
import json
import os

import numpy as np
import pytest
import torch

import dense_bilagrid64 as D
from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _render, _truth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (8, 8, 4)  # (Gh, Gw, L) of the optimised grids


def true_grids(V, shape=SHAPE, amplitude=0.15, seed=21):
    """identity plus noise bounded by `amplitude`, smooth: a random 2 x 2 x 2 grid resampled trilinearly at the vertices of `shape`, which a grid
    of that shape represents exactly; view 0 is the identity"""
    Gh, Gw, L = shape
    g = torch.Generator().manual_seed(seed)
    coarse = amplitude * (torch.rand(V, 12, 2, 2, 2, generator=g, dtype=torch.float64) * 2 - 1)
    fine = torch.nn.functional.interpolate(coarse, size=(L, Gh, Gw), mode="trilinear", align_corners=True)
    fine[0] = 0
    return (torch.from_numpy(D.identity_grids(V, Gh, Gw, L)).double() + fine).float().numpy()


def graded_targets(renders, grids):
    """the float64 reference's slice of the true renders, as float32 on the GPU"""
    return torch.from_numpy(D.explicit(renders.cpu().numpy(), grids)["out"]).float().cuda()


@pytest.fixture(scope="module")
def scene():
    from siu3r_amd.refine import covariances_from

    truth = _truth()
    cams, K = _cams([0, 1, 2, 3])
    renders = _render(cams, K, truth["means"], covariances_from(truth["rotations"], truth["scales"]), truth["harmonics"], truth["opacities"])[0]
    grids = true_grids(4)
    g = torch.Generator().manual_seed(77)
    n = lambda *s: torch.randn(*s, generator=g).cuda()
    G = truth["means"].shape[0]
    start = dict(truth)  # the "appearance" perturbation of test_refine_cameras_gpu.py's joint fixture
    start["harmonics"] = truth["harmonics"] + 0.15 * n(G, 3, 4)
    start["opacities"] = torch.sigmoid(torch.logit(truth["opacities"]) + 0.7 * n(G))
    start["scales"] = torch.exp(torch.log(truth["scales"]) + 0.2 * n(G, 3))
    return dict(truth=truth, start={k: v.clone() for k, v in start.items()}, cams=cams, K=K, renders=renders, grids=grids, targets=graded_targets(renders, grids))


def photometric(out, s, transform):
    """the photometric term alone of a returned scene: re-rendered, the returned transform applied"""
    from siu3r_amd.losses import apply_bilagrid, apply_exposure, photometric_loss

    img = _render(out.get("c2w", s["cams"]), s["K"], out["means"], out["covariances"], out["harmonics"], out["opacities"])[0]
    if transform == "affine":
        img = apply_exposure(img, out["exposure"])
    elif transform == "bilagrid":
        img = apply_bilagrid(img, out["bilagrid"])
    return float(photometric_loss(img, s["targets"]))


def _refine(s, fields, **kw):
    from siu3r_amd.refine import refine_gaussians

    return refine_gaussians(*(fields[k] for k in FIELDS), s["targets"], s["cams"], s["K"], NEAR, FAR, BG, **kw)


def test_grid_recovery_against_frozen_gaussians(scene):
    """frozen true Gaussians and poses, params=(): 300 iterations bring the photometric loss below a tenth of the initial one (the bar
    test_refine_cameras_gpu.py sets for pose), view 0 keeps the identity grid's bits, and nothing else moves"""
    from siu3r_amd.cameras import CameraControl, identity_grids

    control = CameraControl(pose=False, exposure="bilagrid", bilagrid_shape=SHAPE)
    first = photometric(dict(scene["truth"], covariances=_cov(scene["truth"])), scene, None)
    out, losses = _refine(scene, scene["truth"], iters=300, params=(), log_every=50, cameras=control)
    last = photometric(out, scene, "bilagrid")
    err = float((out["bilagrid"][1:].cpu() - torch.from_numpy(scene["grids"][1:])).abs().max())
    print(f"\ngrid recovery, lr_bilagrid {control.lr_bilagrid:g}, lambda_tv {control.lambda_tv:g}: photometric {first:.5f} -> {last:.6f}; "
          f"max |grid - true| {err:.4f}; objective {losses[0]:.5f} -> {losses[-1]:.6f}")
    assert set(out) == set(FIELDS) | {"covariances", "c2w", "exposure", "camera_steps", "bilagrid"}
    assert out["bilagrid"].shape == (4, 12, SHAPE[2], SHAPE[0], SHAPE[1]) and out["camera_steps"] == 300
    assert torch.equal(out["bilagrid"][0], identity_grids(1, SHAPE, "cuda")[0]), "the fixed view's grid is not exactly the identity"
    assert torch.equal(out["exposure"], torch.eye(3, 4).repeat(4, 1, 1).cuda()) and torch.equal(out["c2w"], scene["cams"])
    for k in FIELDS:
        assert torch.equal(out[k], scene["truth"][k]), f"{k} is frozen and moved"
    assert last < first / 10, (first, last)


def _cov(fields):
    from siu3r_amd.refine import covariances_from

    return covariances_from(fields["rotations"], fields["scales"])


def test_bilagrid_beats_affine_beats_no_cameras(scene):
    """joint refinement (scales, opacities, SH) from perturbed appearance, 60 iterations, scored by the photometric term alone on the returned
    scene with the returned transform: strictly bilagrid < affine < none, with the default lr_bilagrid.  No spread margin is applied: two
    runs of one configuration differ by the composite backward's float atomics only, in the last bits, and the three scores measured on an
    MI355X are 0.0032 / 0.0100 / 0.0202."""
    from siu3r_amd.cameras import CameraControl

    kw = dict(iters=60, params=("scales", "opacities", "harmonics"), log_every=0)
    none, _ = _refine(scene, scene["start"], **kw)
    affine, _ = _refine(scene, scene["start"], cameras=CameraControl(pose=False, exposure="affine"), **kw)
    control = CameraControl(pose=False, exposure="bilagrid", bilagrid_shape=SHAPE)
    grid, _ = _refine(scene, scene["start"], cameras=control, **kw)
    scores = dict(none=photometric(none, scene, None), affine=photometric(affine, scene, "affine"), bilagrid=photometric(grid, scene, "bilagrid"))
    print(f"\nphotometric after 60 iterations (lr_bilagrid {control.lr_bilagrid:g}, lambda_tv {control.lambda_tv:g}): {scores}")
    path = os.path.join(ROOT, "profiles", "bilagrid_refine.json")
    if os.access(os.path.dirname(path), os.W_OK):
        with open(path, "w") as fh:
            json.dump(dict(scores, iters=60, lr_bilagrid=control.lr_bilagrid, lambda_tv=control.lambda_tv, bilagrid_shape=list(SHAPE),
                           gpu=torch.cuda.get_device_name()), fh, indent=1, sort_keys=True)
            fh.write("\n")
    assert scores["bilagrid"] < scores["affine"] < scores["none"], scores


def test_affine_is_the_exposure_of_before_bit_for_bit(scene):
    """exposure="affine" against exposure=True with frozen Gaussians and poses, where every kernel of the loop is deterministic (with free
    Gaussians two runs of ONE control already differ in the last bits: the composite backward adds with float atomics)"""
    from siu3r_amd.cameras import CameraControl

    kw = dict(iters=12, params=(), log_every=1)
    a, la = _refine(scene, scene["truth"], cameras=CameraControl(pose=False, exposure=True), **kw)
    b, lb = _refine(scene, scene["truth"], cameras=CameraControl(pose=False, exposure="affine"), **kw)
    assert la == lb and len(la) == 12 and set(a) == set(b) and "bilagrid" not in a
    assert not torch.equal(a["exposure"][1], torch.eye(3, 4).cuda())
    for k in a:
        assert a[k] == b[k] if isinstance(a[k], int) else torch.equal(a[k], b[k]), k


def test_two_bilagrid_runs_give_the_same_bits(scene):
    """frozen Gaussians and poses: the slice, both its backwards, the total variation and the grid's Adam step are deterministic"""
    from siu3r_amd.cameras import CameraControl

    control = CameraControl(pose=False, exposure="bilagrid", bilagrid_shape=(5, 6, 9))
    (a, la), (b, lb) = [_refine(scene, scene["truth"], iters=12, params=(), log_every=1, cameras=control) for _ in range(2)]
    assert la == lb and len(la) == 12 and la[-1] < la[0]
    assert torch.equal(a["bilagrid"], b["bilagrid"]) and not torch.equal(a["bilagrid"][1], a["bilagrid"][0])


@pytest.mark.parametrize("variant", ["density", "mcmc", "depth_hip_pose"])
def test_bilagrid_with_the_other_keywords(scene, variant):
    """the control next to DensityControl, MCMCControl, a depth term, optimizer="hip" and pose optimisation"""
    from siu3r_amd.cameras import CameraControl, identity_grids
    from siu3r_amd.density import DensityControl
    from siu3r_amd.mcmc import MCMCControl

    control = CameraControl(pose=False, exposure="bilagrid", bilagrid_shape=SHAPE)
    if variant == "density":
        kw = dict(density=DensityControl(start=10, every=10))
    elif variant == "mcmc":
        kw = dict(density=MCMCControl(start=10, every=10, cap_max=scene["start"]["means"].shape[0] + 500))
    else:
        control = CameraControl(pose=True, exposure="bilagrid", bilagrid_shape=(4, 5, 9), start=5)
        kw = dict(depths=torch.full((4, H, W), 3.0).cuda(), lambda_depth=0.1, optimizer="hip", sparse=True)
    out, losses = _refine(scene, scene["start"], iters=24, params=("scales", "opacities", "harmonics"), cameras=control, **kw)
    Gh, Gw, L = control.bilagrid_shape
    rows = {out[k].shape[0] for k in FIELDS} | {out["covariances"].shape[0]}
    print(f"\nbilagrid + {variant}: objective {losses[0]:.5f} -> {losses[-1]:.5f}, {rows} rows, {out['camera_steps']} camera steps")
    assert len(rows) == 1 and len(losses) == 24 and all(np.isfinite(losses))
    assert out["bilagrid"].shape == (4, 12, L, Gh, Gw) and bool(torch.isfinite(out["bilagrid"]).all())
    assert torch.equal(out["bilagrid"][0], identity_grids(1, control.bilagrid_shape, "cuda")[0])
    assert not torch.equal(out["bilagrid"][1], identity_grids(1, control.bilagrid_shape, "cuda")[0])
    assert torch.equal(out["exposure"], torch.eye(3, 4).repeat(4, 1, 1).cuda())
    assert out["camera_steps"] == (19 if variant == "depth_hip_pose" else 24)
    if variant == "depth_hip_pose":
        assert out["optimizer_steps"] == 24 and torch.equal(out["c2w"][0], scene["cams"][0]) and not torch.equal(out["c2w"][1:], scene["cams"][1:])
    else:
        assert torch.equal(out["c2w"], scene["cams"]) and len(out["density_events"]) >= 1


def test_iters_zero_returns_the_identity_grids(scene):
    from siu3r_amd.cameras import CameraControl, identity_grids

    out, losses = _refine(scene, scene["start"], iters=0, cameras=CameraControl(exposure="bilagrid", bilagrid_shape=(3, 4, 5)))
    assert losses == [] and out["camera_steps"] == 0 and torch.equal(out["bilagrid"], identity_grids(4, (3, 4, 5), "cuda"))
