"""refine.refine_gaussians with optimizer="hip" (siu3r_amd/optim.py::GaussianAdam, csrc/gaussian_adam.hip): the assertions the torch path
passes in tests/test_refine_gpu.py, the first-step arithmetic of the learning-rate rules, the row skip, and density control through
moments / rebind.  Scenes as tests/test_refine_gpu.py builds them."""
import numpy as np
import pytest
import torch

from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _psnr, _render, _truth

pytestmark = pytest.mark.gpu


def _touched(c2w, K, s):
    """[G] bool: the Gaussians with radii > 0 in any of the views"""
    from siu3r_amd.refine import covariances_from

    _, _, aux = _render(c2w, K, s["means"], covariances_from(s["rotations"], s["scales"]), s["harmonics"], s["opacities"], aux=True)
    return (torch.cat([a["radii"] for a in aux]) > 0).any(-1).any(0)


@pytest.mark.parametrize("variant,sparse", [("appearance", False), ("everything", False), ("everything", True)])
def test_hip_optimizer_recovers_perturbed_gaussians(variant, sparse):
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
    out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=60, params=params, optimizer="hip", sparse=sparse)
    after = _psnr(_render(held, Kh, out["means"], out["covariances"], out["harmonics"], out["opacities"])[0][0], held_target)
    print(f"\nrefine, hip optimiser ({variant}{', sparse' if sparse else ''}): training loss {losses[0]:.5f} -> {losses[-1]:.5f}, "
          f"held-out PSNR {before:.3f} -> {after:.3f} dB")
    assert len(losses) == 60 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert after > before
    assert out["optimizer_steps"] == 60
    for k in FIELDS:
        assert torch.equal(start[k], keep[k]), f"input {k} was modified"
        assert start[k].grad is None and not start[k].requires_grad
        assert out[k].data_ptr() != start[k].data_ptr() and out[k].shape == start[k].shape
        if k in params:
            assert not torch.equal(out[k], start[k]), f"{k} is free and did not move"
        else:
            assert torch.equal(out[k], start[k]), f"{k} is frozen and moved"
    assert out["covariances"].shape == (G, 3, 3) and torch.equal(out["covariances"], covariances_from(out["rotations"], out["scales"]))
    if sparse:
        unseen = ~_touched(train, Kt, start)
        print(f"{int(unseen.sum())} Gaussians are in no training view at the start")


def _ulp(x):
    """one unit in the last place of every float32 element"""
    return (torch.nextafter(x.abs(), torch.full_like(x, float("inf"))) - x.abs())


def _check_first_step(move, old, rate, touched, what):
    """at t = 1 the Adam step is rate * g / (|g| + eps): at most `rate` long, and `rate` long wherever |g| >> eps"""
    bound = rate * (1 + 1e-3) + _ulp(old)
    assert bool((move.abs() <= bound).all()), f"{what}: a step longer than {rate:.3e} (1 + 1e-3) + 1 ulp: {float((move.abs() - bound).max()):.3e} over"
    rows = move.flatten(1).any(1)
    assert int(rows.sum()) > 0 and not bool((rows & ~touched).any()), f"{what}: a Gaussian outside the render's radii > 0 set moved"
    return rows


def test_first_step_of_the_sh_rates():
    from siu3r_amd.refine import refine_gaussians

    s = _truth(seed=3)
    train, Kt = _cams([0, 1, 2, 3])
    targets = torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    touched = _touched(train, Kt, s)
    L = 2.5e-3
    for sparse in (False, True):
        out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=1, lambda_dssim=0.0, params=("harmonics",),
                                       lrs={"harmonics": L}, optimizer="hip", sh_rest_lr_scale=0.05, sparse=sparse)
        move = out["harmonics"] - s["harmonics"]
        dc, rest = move[:, :, 0], move[:, :, 1:]
        rows = _check_first_step(dc, s["harmonics"][:, :, 0], L, touched, "DC")
        _check_first_step(rest, s["harmonics"][:, :, 1:], 0.05 * L, touched, "higher bands")
        median = float(dc[dc != 0].abs().median())
        print(f"\nfirst SH step{' (sparse)' if sparse else ''}: {int(rows.sum())} of {int(touched.sum())} touched Gaussians moved; median DC move {median:.6e} "
              f"(rate {L:.3e}), largest higher-band move {float(rest.abs().max()):.6e} (rate {0.05 * L:.3e})")
        assert median >= 0.99 * L
        assert len(losses) == 1 and out["optimizer_steps"] == 1
        for k in ("means", "scales", "rotations", "opacities"):
            assert torch.equal(out[k], s[k])


def test_first_step_of_the_extent_scaled_means_rate():
    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import refine_gaussians

    s = _truth(seed=3)
    train, Kt = _cams([0, 1, 2, 3])
    targets = torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    touched = _touched(train, Kt, s)
    L = 1.6e-4
    out, _ = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=1, lambda_dssim=0.0, params=("means",), lrs={"means": L},
                              optimizer="hip", means_lr_extent_scale=True, means_lr_final=1e-6, density=DensityControl(scene_extent=3.0))
    move = out["means"] - s["means"]
    _check_first_step(move, s["means"], 3 * L, touched, "means")
    median = float(move[move != 0].abs().median())
    print(f"\nfirst means step: median move {median:.6e}, extent 3 x rate {L:.3e} = {3 * L:.3e}")
    assert median >= 0.99 * 3 * L
    assert out["density_events"] == [] and out["optimizer_steps"] == 1
    # the decay: the last of two steps runs at 3 x means_lr_final, so two steps move at most 3 (L + final) (+ rounding)
    out2, _ = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=2, lambda_dssim=0.0, params=("means",), lrs={"means": L},
                               optimizer="hip", means_lr_extent_scale=True, means_lr_final=1e-6, density=DensityControl(scene_extent=3.0))
    move2 = (out2["means"] - s["means"]).abs()
    assert bool((move2 <= 3 * (L + 1e-6) * (1 + 1e-3) + 2 * _ulp(s["means"])).all()) and float(move2.max()) > 3 * L * 0.99


def test_sparse_steps_with_density_control():
    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import covariances_from, refine_gaussians

    truth = _truth()
    train, Kt = _cams([0, 1, 2, 3])
    targets = _render(train, Kt, truth["means"], covariances_from(truth["rotations"], truth["scales"]), truth["harmonics"], truth["opacities"])[0]
    G0 = truth["means"].shape[0]
    half = torch.randperm(G0, generator=torch.Generator().manual_seed(21))[: G0 // 2].sort().values.cuda()
    start = {k: v[half].clone() for k, v in truth.items()}
    control = DensityControl(grad_threshold=2e-5, start=10, every=10, scene_extent=5.0, reset_every=15)
    out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=30, density=control, optimizer="hip", sparse=True,
                                   sh_rest_lr_scale=0.05, means_lr_final=1.6e-6, means_lr_extent_scale=True)
    ev = out["density_events"]
    plain, plain_losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=30, density=control)
    print(f"\nsparse + density: {G0 // 2} -> {out['means'].shape[0]} Gaussians, events {ev}; loss {losses[0]:.5f} -> {losses[-1]:.5f} (the opacity reset "
          f"of iteration 15 is 15 steps old; torch optimiser, same control: {plain['means'].shape[0]} Gaussians, {plain_losses[0]:.5f} -> {plain_losses[-1]:.5f})")
    assert [e["iteration"] for e in ev] == [10, 20] and ev[0]["rows_out"] != ev[0]["rows_in"]
    assert all(out[k].shape[0] == ev[-1]["rows_out"] for k in FIELDS + ("covariances",))
    assert len(losses) == 30 and all(np.isfinite(losses))
    assert out["optimizer_steps"] == 30
    assert all(bool(torch.isfinite(out[k]).all()) for k in FIELDS)


def test_sparse_steps_with_a_depth_term():
    """sparse=True together with depths=: the one iteration whose radii (for the step) and opacity map (for the depth term) come out of the
    same aux.  A pin that this branch runs, returns the right keys, shapes and step count and leaves the unseen rows alone; a Gaussian
    no view saw has a zero gradient and zero moments, so a dense step would keep its bits too: that the radii gate the step is
    pinned by tests/test_gaussian_adam_gpu.py, not here.  Geometry is frozen, so the set of Gaussians the training views see is the
    same at every iteration."""
    from siu3r_amd.refine import covariances_from, refine_gaussians

    s = _truth(G=2000)
    train, Kt = _cams([0, 1])
    targets, depth, aux = _render(train, Kt, s["means"], covariances_from(s["rotations"], s["scales"]), s["harmonics"], s["opacities"], aux=True)
    opacity = torch.cat([a["opacity"] for a in aux])
    conf = (opacity > 0.5).float()
    depths = torch.where(opacity > 0.5, depth / opacity.clamp_min(1e-6), torch.zeros_like(depth))
    keep = {k: v.clone() for k, v in s.items()}
    out, losses = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=3, params=("opacities", "harmonics"), optimizer="hip",
                                   sparse=True, depths=depths, depth_weights=conf, lambda_depth=1.0)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert len(out["depth_losses"]) == 3 and all(np.isfinite(out["depth_losses"]))
    assert out["optimizer_steps"] == 3
    for k in ("means", "scales", "rotations"):
        assert torch.equal(out[k], keep[k]), f"{k} is frozen and moved"
    untouched = ~_touched(train, Kt, keep) & ~_touched(train, Kt, out)
    touched = ~untouched
    print(f"\nsparse + depth: {int(touched.sum())} of {untouched.numel()} Gaussians touched, losses {losses}, depth term {out['depth_losses']}")
    assert int(untouched.sum()) > 0 and int(touched.sum()) > 0
    assert torch.equal(out["harmonics"][untouched], keep["harmonics"][untouched])
    round_trip = torch.sigmoid(torch.logit(keep["opacities"].clamp(1e-6, 1 - 1e-6)))  # what a free opacity that never moved comes back as
    assert torch.equal(out["opacities"][untouched], round_trip[untouched])
    assert not torch.equal(out["harmonics"][touched], keep["harmonics"][touched]), "no touched harmonics row moved"
    assert not torch.equal(out["opacities"][touched], round_trip[touched]), "no touched opacity moved"


def test_torch_path_does_not_report_optimizer_steps():
    from siu3r_amd.refine import refine_gaussians

    s = _truth(G=2000, seed=2)
    train, Kt = _cams([0, 1])
    targets = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    out, _ = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=2)
    assert set(out) == set(FIELDS) | {"covariances"}
    out, _ = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=2, optimizer="hip")
    assert set(out) == set(FIELDS) | {"covariances", "optimizer_steps"} and out["optimizer_steps"] == 2
    out, _ = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=0, optimizer="hip")
    assert out["optimizer_steps"] == 0 and all(torch.equal(out[k], s[k]) for k in FIELDS)
