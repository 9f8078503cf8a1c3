"""refine.refine_gaussians with MCMC densification (siu3r_amd/mcmc.py, csrc/mcmc.hip): relocation of the dead rows, growth by 5 % per event
up to the cap, both optimisers, and the objective going down.  Scenes as tests/test_refine_gpu.py builds them."""
import numpy as np
import pytest
import torch

from refine_scenes import BG, FAR, FIELDS, NEAR, _cams, _psnr, _render, _truth

pytestmark = pytest.mark.gpu

G, K_DEAD, ITERS = 4000, 137, 30
_CACHE = {}


def _scene():
    """the truth (4000 Gaussians), its four training views and one held-out view, and the start: the truth with K_DEAD opacities at 1e-4
    (seeded rows) and perturbed SH coefficients.  Built once, never modified."""
    if not _CACHE:
        from siu3r_amd.refine import covariances_from

        truth = _truth(G=G)
        train, Kt = _cams([0, 1, 2, 3])
        held, Kh = _cams([4])
        cov = covariances_from(truth["rotations"], truth["scales"])
        targets = _render(train, Kt, truth["means"], cov, truth["harmonics"], truth["opacities"])[0]
        held_target = _render(held, Kh, truth["means"], cov, truth["harmonics"], truth["opacities"])[0][0]
        g = torch.Generator().manual_seed(17)
        dead = torch.randperm(G, generator=g)[:K_DEAD].cuda()
        start = {k: v.clone() for k, v in truth.items()}
        start["opacities"][dead] = 1e-4
        start["harmonics"] = start["harmonics"] + 0.1 * torch.randn(G, 3, 4, generator=g).cuda()
        _CACHE.update(start=start, keep={k: v.clone() for k, v in start.items()}, train=train, Kt=Kt, held=held, Kh=Kh, targets=targets,
                      held_target=held_target, dead=dead)
    return _CACHE


def _run(density, **kw):
    from siu3r_amd.refine import refine_gaussians

    s = _scene()
    out, losses = refine_gaussians(*(s["start"][k] for k in FIELDS), s["targets"], s["train"], s["Kt"], NEAR, FAR, BG, density=density, **{"iters": ITERS, **kw})
    for k in FIELDS:
        assert torch.equal(s["start"][k], s["keep"][k]), f"input {k} was modified"
    return out, losses


def _check_events(out, cap_max, min_opacity=0.005, frozen_opacities=True):
    """what every run must show.  With the opacities out of `params` only the events move them: an event moves every row at or under the
    floor onto a live one, and the update's clamp (which would put a row exactly AT the floor) is out of reach of this scene's opacities
    of at least 0.05 and counts of a few, so no such row may be returned.  Free opacities take ten more Adam steps of up to 0.05 in the
    logit after the last event, which may push a row under the floor again (the next event would relocate it): the caller prints that
    count instead."""
    ev = out["density_events"]
    assert [e["iteration"] for e in ev] == [10, 20]
    rows = G
    for e in ev:
        assert set(e) == {"iteration", "rows_in", "rows_out", "relocated", "added"}
        assert e["rows_in"] == rows and e["rows_out"] == min(cap_max, int(1.05 * e["rows_in"])) and e["added"] == e["rows_out"] - e["rows_in"]
        rows = e["rows_out"]
    for k in FIELDS + ("covariances",):
        assert out[k].shape[0] == rows, k
    assert out["covariances"].shape == (rows, 3, 3) and out["harmonics"].shape[1:] == (3, 4)
    if frozen_opacities:
        assert not bool((out["opacities"] <= min_opacity).any()), "a dead Gaussian was returned"
    assert all(bool(torch.isfinite(out[k]).all()) for k in FIELDS)
    return ev


@pytest.mark.parametrize("optimizer", ["torch", "hip-sparse"])
def test_frozen_opacities_relocate_exactly_the_dead_rows_and_the_set_grows(optimizer):
    """the opacities stay out of `params`: nothing but the events moves them, so the first event finds exactly the K_DEAD rows"""
    from siu3r_amd.mcmc import MCMCControl

    kw = dict(optimizer="hip", sparse=True) if optimizer == "hip-sparse" else {}
    out, losses = _run(MCMCControl(cap_max=10**6, start=10, every=10), params=("means", "scales", "rotations", "harmonics"), **kw)
    ev = _check_events(out, 10**6)
    print(f"\nMCMC ({optimizer}), frozen opacities: events {ev}; objective {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert ev[0]["relocated"] == K_DEAD and ev[1]["relocated"] == 0
    assert (ev[0]["rows_out"], ev[1]["rows_out"]) == (4200, 4410)
    assert len(losses) == ITERS and all(np.isfinite(losses))
    if optimizer == "hip-sparse":
        assert out["optimizer_steps"] == ITERS
    else:
        assert "optimizer_steps" not in out


@pytest.mark.parametrize("optimizer", ["torch", "hip-sparse"])
def test_at_the_cap_the_row_count_never_changes(optimizer):
    from siu3r_amd.mcmc import MCMCControl

    kw = dict(optimizer="hip", sparse=True) if optimizer == "hip-sparse" else {}
    out, losses = _run(MCMCControl(cap_max=G, start=10, every=10), params=("means", "scales", "rotations", "harmonics"), **kw)
    ev = _check_events(out, G)
    assert all(e["added"] == 0 and e["rows_out"] == G for e in ev) and ev[0]["relocated"] == K_DEAD
    assert out["means"].shape[0] == G and len(losses) == ITERS and all(np.isfinite(losses))
    if optimizer == "hip-sparse":
        assert out["optimizer_steps"] == ITERS
    # a cap between G and 1.05 G is reached exactly
    out, _ = _run(MCMCControl(cap_max=G + 77, start=10, every=10), params=("harmonics",), **kw)
    ev = _check_events(out, G + 77)
    assert [e["added"] for e in ev] == [77, 0]


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
@pytest.mark.parametrize("control", ["classic", "mcmc"])
def test_before_the_first_event_a_control_leaves_the_frozen_fields_bit_identical(control, optimizer):
    """a run that ends before the control's `start`: no event runs, so no frozen field may have gone through its unconstrained form
    (sigmoid(logit(x)) is not x, exp(log(x)) is not x): means, scales, rotations and opacities come back with the input's bits"""
    from siu3r_amd.density import DensityControl
    from siu3r_amd.mcmc import MCMCControl

    density = DensityControl(start=100) if control == "classic" else MCMCControl(cap_max=10**6, start=100)
    out, losses = _run(density, params=("harmonics",), iters=5, optimizer=optimizer)
    assert out["density_events"] == [] and len(losses) == 5
    for k in ("means", "scales", "rotations", "opacities"):
        assert torch.equal(out[k], _scene()["start"][k]), f"frozen {k} changed without an event"
    assert not torch.equal(out["harmonics"], _scene()["start"]["harmonics"])


def test_all_fields_free_the_objective_goes_down():
    """every field free: the logged objective (photometric + both regulariser values) ends below its start.  The held-out PSNR against clone / split / prune at equal iterations is printed, not asserted (nobody
    has measured it)."""
    from siu3r_amd.density import DensityControl
    from siu3r_amd.mcmc import MCMCControl

    s = _scene()
    psnr = lambda o: _psnr(_render(s["held"], s["Kh"], o["means"], o["covariances"], o["harmonics"], o["opacities"])[0][0], s["held_target"])
    out, losses = _run(MCMCControl(cap_max=10**6, start=10, every=10))
    ev = _check_events(out, 10**6, frozen_opacities=False)
    assert len(losses) == ITERS and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert ev[0]["relocated"] >= K_DEAD  # (free opacities: the regulariser may have pushed more rows under the floor)
    print(f"\nall fields free: {int((out['opacities'] <= 0.005).sum())} returned opacities at or under the floor, the smallest {float(out['opacities'].min()):.5f}")
    plain, plain_losses = _run(MCMCControl(cap_max=10**6, start=10, every=10, opacity_reg=0.0, scale_reg=0.0, noise_lr=0.0))
    _check_events(plain, 10**6, frozen_opacities=False)
    assert losses[0] > plain_losses[0], "the logged objective includes the regulariser values"
    classic, classic_losses = _run(DensityControl(start=10, every=10))
    none, none_losses = _run(None)
    print(f"\nall fields free, {ITERS} iterations: MCMC events {ev}; objective {losses[0]:.5f} -> {losses[-1]:.5f} (no regulariser, no noise: "
          f"{plain_losses[0]:.5f} -> {plain_losses[-1]:.5f}; clone / split / prune: {classic_losses[0]:.5f} -> {classic_losses[-1]:.5f}; fixed set: "
          f"{none_losses[0]:.5f} -> {none_losses[-1]:.5f}); held-out PSNR: MCMC {psnr(out):.3f} dB ({out['means'].shape[0]} Gaussians), clone / split / prune "
          f"{psnr(classic):.3f} dB ({classic['means'].shape[0]}), fixed set {psnr(none):.3f} dB")
    assert "density_events" not in none


def test_depth_and_learning_rate_keywords_work_with_the_control():
    from siu3r_amd.mcmc import MCMCControl
    from siu3r_amd.refine import covariances_from

    s = _scene()
    truth = _truth(G=G)
    depths = _render(s["train"], s["Kt"], truth["means"], covariances_from(truth["rotations"], truth["scales"]), truth["harmonics"], truth["opacities"])[1]
    out, losses = _run(MCMCControl(cap_max=4100, start=10, every=10), depths=depths, lambda_depth=0.1, optimizer="hip", sparse=True, means_lr_final=1.6e-6,
                       sh_rest_lr_scale=0.05)
    ev = _check_events(out, 4100, frozen_opacities=False)
    print(f"\ndepth term, hip optimiser, sparse, decayed means rate: events {ev}; objective {losses[0]:.5f} -> {losses[-1]:.5f}, depth term "
          f"{out['depth_losses'][0]:.5f} -> {out['depth_losses'][-1]:.5f}")
    assert out["optimizer_steps"] == ITERS and len(out["depth_losses"]) == ITERS and losses[-1] < losses[0]
