"""refine.refine_gaussians with adaptive density control (siu3r_amd/density.py, csrc/density.hip): prune, growth, optimiser state carry,
and the default path untouched.  Scenes as tests/test_refine_gpu.py builds them."""
import numpy as np
import pytest
import torch

from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _psnr, _render, _truth

pytestmark = pytest.mark.gpu


def _render_fields(c2w, K, s, aux=False):
    from siu3r_amd.refine import covariances_from

    return _render(c2w, K, s["means"], covariances_from(s["rotations"], s["scales"]), s["harmonics"], s["opacities"], aux=aux)


def _unconstrained(s):
    return dict(means=s["means"].clone(), scales=torch.log(s["scales"]), rotations=s["rotations"].clone(),
                opacities=torch.logit(s["opacities"].clamp(1e-6, 1 - 1e-6)), harmonics=s["harmonics"].clone())


def _constrained(u):
    return dict(means=u["means"], scales=torch.exp(u["scales"]), rotations=u["rotations"], opacities=torch.sigmoid(u["opacities"]), harmonics=u["harmonics"])


def _with_hidden(truth, n=2000, seed=9):
    """+ n Gaussians BEHIND every camera (the cameras sit within 0.3 of the origin and look down +z), opacity 0.001: never visible"""
    g = torch.Generator().manual_seed(seed)
    extra = dict(means=torch.stack((torch.rand(n, generator=g) * 2 - 1, torch.rand(n, generator=g) * 2 - 1, -3.0 - 2.0 * torch.rand(n, generator=g)), -1),
                 scales=0.01 + 0.1 * torch.rand(n, 3, generator=g), rotations=torch.randn(n, 4, generator=g), opacities=torch.full((n,), 0.001),
                 harmonics=torch.rand(n, 3, 4, generator=g) - 0.5)
    where = torch.randperm(truth["means"].shape[0] + n, generator=g)[:n].sort().values  # scattered through the memory order
    total = truth["means"].shape[0] + n
    hidden = torch.zeros(total, dtype=torch.bool)
    hidden[where] = True
    out = {}
    for k in FIELDS:
        t = torch.empty((total, *truth[k].shape[1:]), device="cuda")
        t[hidden.cuda()] = extra[k].cuda()
        t[~hidden.cuda()] = truth[k]
        out[k] = t
    return out, hidden.cuda()


def _contains_row(rows, wanted):
    """does any row of `wanted` occur in `rows` (bit-equal)?"""
    return bool((rows[:, None, :] == wanted[None, :, :]).all(-1).any())


def test_never_visible_transparent_gaussians_are_pruned():
    from siu3r_amd.density import DensityControl, DensityStats, densify_and_prune
    from siu3r_amd.refine import covariances_from, refine_gaussians

    scene, hidden = _with_hidden(_truth())
    G = scene["means"].shape[0]
    assert G == 22000
    train, Kt = _cams([0, 1, 2, 3])
    targets = _render_fields(train, Kt, scene)[0]
    _, _, aux = _render_fields(train, Kt, scene, aux=True)
    radii = torch.cat([a["radii"] for a in aux])
    assert not bool((radii[:, hidden] > 0).any()), "the hidden Gaussians must not be visible from any training view"
    keep = {k: v.clone() for k, v in scene.items()}
    g = torch.Generator().manual_seed(5)
    start = dict(scene)
    start["harmonics"] = scene["harmonics"] + 0.1 * torch.randn(G, 3, 4, generator=g).cuda()
    keep["harmonics"] = start["harmonics"].clone()
    out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=30, params=("scales", "opacities", "harmonics"),
                                   density=DensityControl(start=10, every=10))
    ev = out["density_events"]
    print(f"\nprune: {G} -> {out['means'].shape[0]} Gaussians, events {ev}; loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert [e["iteration"] for e in ev] == [10, 20]
    assert ev[0]["pruned"] >= 2000
    assert not _contains_row(out["means"], scene["means"][hidden]), "a hidden Gaussian survived"
    n = out["means"].shape[0]
    rows = G
    for e in ev:
        assert e["rows_in"] == rows and e["rows_out"] == rows + e["cloned"] + e["split"] - e["pruned"]
        rows = e["rows_out"]
    assert n == rows
    for k in FIELDS:
        assert out[k].shape[0] == n and out[k].shape[1:] == start[k].shape[1:]
        assert torch.equal(start[k], keep[k]), f"input {k} was modified"
    assert out["covariances"].shape == (n, 3, 3) and torch.equal(out["covariances"], covariances_from(out["rotations"], out["scales"]))
    assert len(losses) == 30 and all(np.isfinite(losses))

    # a prune-only event removes exactly the hidden ones by an order-preserving compaction: the render keeps its bits
    u = _unconstrained(scene)
    new_u, new_m, info = densify_and_prune(u, {}, DensityStats(G, "cuda"), DensityControl(scene_extent=1.0), 1.0, torch.zeros(G, 2, 3, device="cuda"))
    assert info == dict(rows_in=G, rows_out=G - 2000, pruned=2000, kept=G - 2000, cloned=0, split=0, capped=False) and new_m == {}
    for k in FIELDS:
        assert torch.equal(new_u[k], u[k][~hidden])
    before = _render_fields(train, Kt, _constrained(u))
    after = _render_fields(train, Kt, _constrained(new_u))
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert float(before[0].abs().max()) > 0.05


def test_growth_from_half_the_gaussians():
    """Half of the truth's Gaussians removed (seeded), a threshold low enough that the first event clones and splits.  scene_extent = 5
    puts the clone / split boundary (percent_dense x extent = 0.05) inside the scene's scale range (0.01 .. 0.12).  The held-out PSNR
    with and without density control at equal iterations is printed, not asserted (nobody has run this scenario before)."""
    from siu3r_amd.density import DensityControl, DensityStats, densify_and_prune
    from siu3r_amd.refine import refine_gaussians

    truth = _truth()
    train, Kt = _cams([0, 1, 2, 3])
    held, Kh = _cams([4])
    targets = _render_fields(train, Kt, truth)[0]
    held_target = _render_fields(held, Kh, truth)[0][0]
    G0 = truth["means"].shape[0]
    half = torch.randperm(G0, generator=torch.Generator().manual_seed(21))[: G0 // 2].sort().values.cuda()
    start = {k: v[half].clone() for k, v in truth.items()}
    control = DensityControl(grad_threshold=2e-5, start=20, every=20, scene_extent=5.0)
    out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=60, density=control)
    plain, plain_losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=60)
    ev = out["density_events"]
    psnr = lambda s: _psnr(_render(held, Kh, s["means"], s["covariances"], s["harmonics"], s["opacities"])[0][0], held_target)
    from siu3r_amd.refine import covariances_from
    before = _psnr(_render(held, Kh, start["means"], covariances_from(start["rotations"], start["scales"]), start["harmonics"], start["opacities"])[0][0], held_target)
    print(f"\ngrowth: {G0 // 2} -> {out['means'].shape[0]} Gaussians, events {ev}; training loss {losses[0]:.5f} -> {losses[-1]:.5f} "
          f"(fixed set: {plain_losses[0]:.5f} -> {plain_losses[-1]:.5f}); held-out PSNR {before:.3f} dB at the start, {psnr(out):.3f} dB with density control, "
          f"{psnr(plain):.3f} dB without, 60 iterations each")
    assert [e["iteration"] for e in ev] == [20, 40]
    assert ev[0]["cloned"] > 0 and ev[0]["split"] > 0
    rows = G0 // 2
    for e in ev:
        assert e["rows_in"] == rows and e["rows_out"] - e["rows_in"] == e["cloned"] + e["split"] - e["pruned"]
        rows = e["rows_out"]
    assert all(out[k].shape[0] == rows for k in FIELDS + ("covariances",)) and rows > G0 // 2
    assert len(losses) == 60 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert "density_events" not in plain and plain["means"].shape[0] == G0 // 2

    # optimiser state carry: statistics from one real backward, Adam-like moments, one event; kept rows carry their moments unchanged
    from siu3r_amd.cuda_splatting import render_cuda
    from siu3r_amd import raster

    u = {k: v.requires_grad_(True) for k, v in _unconstrained(start).items()}
    c = _constrained(u)
    V = train.shape[0]
    e = lambda x: x[None].expand(V, *x.shape)
    stats = DensityStats(G0 // 2, "cuda")
    cov6 = raster.quat_scale_to_cov6(torch.roll(c["rotations"], 1, dims=-1), c["scales"])
    img, _ = render_cuda(train, Kt, torch.full((V,), NEAR), torch.full((V,), FAR), (H, W), torch.zeros(V, 3), e(c["means"]), e(cov6), e(c["harmonics"]),
                         e(c["opacities"]), density_stats=stats)
    (img - targets).abs().mean().backward()
    assert int((stats.seen > 0).sum()) > 1000 and float(stats.grad_accum.max()) > 0
    moments = {k: (0.1 * u[k].grad, u[k].grad ** 2 + 1e-12) for k in FIELDS}
    params = {k: v.detach() for k, v in u.items()}
    noise = torch.randn(G0 // 2, 2, 3, generator=torch.Generator().manual_seed(1)).cuda()
    new_p, new_m, info = densify_and_prune(params, moments, stats, control, 5.0, noise)
    assert info["cloned"] > 0 and info["split"] > 0 and info["kept"] > 0
    from siu3r_amd import density

    action, offset, _ = density.plan(stats, params["scales"], params["opacities"], **control.thresholds(5.0))
    kept = action == density.KEEP
    first_of_clone = action == density.CLONE
    for k in FIELDS:
        for sel in (kept, first_of_clone):
            at = offset[sel].long()
            assert torch.equal(new_p[k][at], params[k][sel])
            assert torch.equal(new_m[k][0][at], moments[k][0][sel]) and torch.equal(new_m[k][1][at], moments[k][1][sel])
        copies = offset[first_of_clone].long() + 1
        assert not bool(new_m[k][0][copies].any()) and not bool(new_m[k][1][copies].any())


def test_density_none_is_the_plain_path_and_seeded_runs_repeat():
    """density=None against a call without the keyword: the same code path.  The K2 backward sums with float atomics, so two runs of
    refine_gaussians WITHOUT the keyword need not agree to the bit on a given board; when they do, None must too (torch.equal), and
    when they do not, None may differ from a plain run by at most 4 x what two plain runs differ by (the factor the issue gives a
    different summation order).  Seeded runs with a control: equal bits if the atomics allowed it for the plain runs, else equal G and
    equal events.  The control of this part decides by frozen fields only (threshold 0: everything seen or unseen is hot, the split /
    clone choice is the frozen scale, the prune the frozen opacity), so G does not hang on the last bits of a gradient."""
    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import refine_gaussians

    s = _truth(G=6000, seed=2)
    train, Kt = _cams([0, 1, 2])
    targets = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    call = lambda **kw: refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=4, **kw)
    a, la = call()
    b, lb = call()
    n, ln = call(density=None)
    assert set(n) == set(a) and "density_events" not in n
    same = all(torch.equal(a[k], b[k]) for k in a)
    print(f"\ntwo plain runs are {'the same bits' if same else 'NOT the same bits (float atomics in the backward)'}")
    for k in a:
        if same:
            assert torch.equal(n[k], a[k]), k
        else:
            spread = float((a[k] - b[k]).abs().max())
            assert float((n[k] - a[k]).abs().max()) <= 4 * spread, (k, spread)
    control = DensityControl(grad_threshold=0.0, start=2, every=1, stop=2, scene_extent=5.0, seed=123)
    runs = [refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=4, params=("means", "harmonics"), density=control)[0]
            for _ in range(2)]
    other = refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=4, params=("means", "harmonics"),
                             density=DensityControl(grad_threshold=0.0, start=2, every=1, stop=2, scene_extent=5.0, seed=124))[0]
    assert runs[0]["density_events"] == runs[1]["density_events"] == other["density_events"] and len(runs[0]["density_events"]) == 1
    assert runs[0]["density_events"][0]["split"] > 0 and runs[0]["means"].shape[0] == runs[1]["means"].shape[0] > 6000
    if same:
        assert all(torch.equal(runs[0][k], runs[1][k]) for k in FIELDS + ("covariances",))
    # the seed places the children of a split: another seed, other means, the same frozen scales
    assert torch.equal(runs[0]["scales"], other["scales"]) and not torch.equal(runs[0]["means"], other["means"])


def test_opacity_reset_clamps_the_free_opacities():
    """reset_every = 2 of 4 iterations, stop = 3 (resets happen up to `stop`), no densify event: at iteration 2 every logit opacity becomes min(logit, logit(0.01)) and its
    moments are zeroed; two Adam steps follow, each at most the learning rate long (|m_hat| / sqrt(v_hat) <= 1 for moments that start from
    zero), so every returned opacity is at most sigmoid(logit(0.01) + 2 lr).  Without the reset the same run keeps its opaque Gaussians."""
    import math

    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import DEFAULT_LRS, refine_gaussians

    s = _truth(G=6000, seed=6)
    train, Kt = _cams([0, 1, 2])
    targets = _render_fields(train, Kt, s)[0]
    run = lambda c: refine_gaussians(*(s[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=4, params=("opacities",), density=c)[0]
    out = run(DensityControl(start=100, stop=3, reset_every=2, reset_opacity=0.01))
    plain = run(DensityControl(start=100, stop=3))
    bound = 1.0 / (1.0 + math.exp(-(math.log(0.01 / 0.99) + 2 * DEFAULT_LRS["opacities"])))
    print(f"\nopacity reset: largest opacity {float(out['opacities'].max()):.5f} (bound {bound:.5f}), without a reset {float(plain['opacities'].max()):.5f}")
    assert out["density_events"] == [] and plain["density_events"] == [] and out["opacities"].shape == s["opacities"].shape
    assert float(out["opacities"].max()) <= bound * (1 + 1e-6)
    assert float(plain["opacities"].max()) > 0.5
    for k in ("means", "scales", "rotations", "harmonics"):
        assert torch.equal(out[k], s[k])
