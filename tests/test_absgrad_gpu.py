"""The absolute-gradient (AbsGS, Ye et al. 2024) densification statistics on the GPU: siu3r_raster_composite_rgb_bwd_abs
(composite_rgb_bwd_kernel<false, ABS = true> of siu3r_amd/csrc/raster_bwd.hip) called through the C ABI on the crafted composite cases of
tests/dense_raster_bwd64.py and held element by element to the float64 reference of tests/dense_absgrad64.py, then the layers above it:
raster.rasterize_views_k2(density_stats=DensityStats(absgrad=True)), density.plan on the case the statistics exist for, and
refine.refine_gaussians(density=DensityControl(absgrad=True)).

The tolerance is the signed element's, |got - ref| <= comp_bound(n_add) S[:, k] + chain[:, k] (k = MX, MY; |x| is 1-Lipschitz), with S,
chain and n_add of composite_bwd64 on the same case; margin pixels carry an upstream gradient of exactly 0, at most 1 % of a view's pixels,
as in tests/test_raster_bwd_stages_gpu.py, whose device-state helpers are reused.  Every output lies in a sentinel-filled parent.
With SIU3R_ABSGRAD_PARITY_LOG=file every comparison of abs_mean2d appends one JSON line (tools/absgrad_parity.py groups them into
profiles/absgrad_parity.json).

Figures of the run recorded in DESIGN.md section 25 (one MI355X): see profiles/absgrad_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import dense_absgrad64 as A
import dense_raster_bwd64 as B
from test_raster_bwd_stages_gpu import _cam_blocks, _check_composite, _composite_state, _dev, _f, _forward_totals, _ok, _p, _refused

pytestmark = pytest.mark.gpu
U24 = B.U24
MXY = [B.MX, B.MY]


def _close_abs(got, ref, r, name):
    """abs_mean2d of one view against the reference with the signed element's tolerance; one JSON line per comparison when asked"""
    got = got.detach().cpu() if torch.is_tensor(got) else got
    S, chain = r["S"][:, MXY], r["chain"][:, MXY]
    w = B.assert_elems_close(got, ref, S, r["bound"], name=name, extra=chain)
    if os.environ.get("SIU3R_ABSGRAD_PARITY_LOG"):
        med, mx = B.effective_bound(ref, S, r["bound"], chain)
        with open(os.environ["SIU3R_ABSGRAD_PARITY_LOG"], "a") as f:
            f.write(json.dumps({"case": name, "max_err_over_S": B.observed(got, ref, S), "worst_ratio_to_bound": w, "bound_over_S_median": med,
                                "bound_over_S_max": mx}) + "\n")
    return w


def _args(c, st, totals, ups, grad, abs_m):
    out, depth, alpha = totals
    g_out, g_alpha, g_depth = _dev(ups["g_out"]), _dev(ups["g_alpha"]), _dev(ups["g_depth"])
    keep = (g_out, g_alpha, g_depth)
    return keep, [st["arr"], c["V"], _p(st["cams_dev"]), c["G"], _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(out), _p(depth), _p(alpha),
                  _p(g_out), _p(g_depth), _p(g_alpha), _p(grad), _p(abs_m)]


def _run_abs(c, ups):
    """forward totals + the abs entry point on a crafted case -> st, totals, grad [V,G,10], abs_mean2d [V,G,2] (both _Guarded)"""
    st = _composite_state(c)
    with torch.no_grad():
        totals = _forward_totals(c, st)
    grad, abs_m = _f((c["V"], c["G"], 10)), _f((c["V"], c["G"], 2))
    keep, args = _args(c, st, totals, ups, grad, abs_m)
    _ok("siu3r_raster_composite_rgb_bwd_abs", *args)
    assert grad.guards_intact() and abs_m.guards_intact()
    return st, totals, grad, abs_m


def _check_abs(name, refs, abss, grad, abs_m):
    got_g, got_a = grad.t.cpu(), abs_m.t.cpu()
    for v, (r, a) in enumerate(zip(refs, abss)):
        _close_abs(got_a[v], a["abs"], r, f"{name} view {v} abs_mean2d")
        nowhere = torch.from_numpy(r["n_add"] == 0)
        assert not bool((got_a[v][nowhere] != 0).any()) and not bool((got_g[v][nowhere] != 0).any()), "a Gaussian that blends nowhere gets exactly 0"
        assert bool((got_a[v] >= 0).all())


RUNS = [("k2_full", "all"), ("k2_small", "all")] + [("k2_ragged", m) for m in B.COMP_MODES]


@pytest.mark.parametrize("name,mode", RUNS)
def test_abs_entry_point_on_the_crafted_cases(name, mode):
    c = B.comp_case(name)
    refs, ups, abss = A.crafted_ref(name, mode)
    low = c["margins"] < B.MARGIN
    assert low.reshape(c["V"], -1).mean(1).max() <= B.ZERO_SHARE_CAP, "more than 1 % of a view's pixels are zeroed"
    if name == "k2_full":
        assert max(int(np.diff(l[0]).max()) for l in c["lists"]) > 256, "no tile with a second staging slice"
    st, totals, grad, abs_m = _run_abs(c, ups)
    _check_abs(f"{name} {mode}", refs, abss, grad, abs_m)
    # the signed record of the same launch: the existing comparison, forward maps included
    _check_composite(f"{name} {mode} (abs launch)", "k2", 3, refs, low, totals, grad, None, c)


def test_single_pixel_upstream_gives_the_exact_identity():
    """an upstream gradient that is non-zero at ONE pixel: every element is a sum of one term, so abs_mean2d == |grad[..., :2]| to the bit"""
    c = B.comp_case("k2_small")
    refs, _, _ = A.crafted_ref("k2_small")
    # the pixel (of those above the margin) that blends the most entries
    depth_of = np.zeros((c["H"], c["W"]), np.int64)
    for tile, (w, _, _) in c["walk_cache"][0].items():
        px, py, inside, _ = B._tile_pixels(c["cams"][0], tile, False)
        depth_of[py[inside], px[inside]] = (w["bl"] & ~w["clamped"]).sum(0)[inside]
    depth_of[c["margins"][0] < B.MARGIN] = 0
    y, x = np.unravel_index(int(depth_of.argmax()), depth_of.shape)
    assert depth_of[y, x] >= 3
    ups = {k: np.zeros_like(v) for k, v in c["ups"].items()}
    for k in ups:
        ups[k][..., y, x] = c["ups"][k][..., y, x]
    _, _, grad, abs_m = _run_abs(c, ups)
    assert int((abs_m.t != 0).any(-1).sum()) >= 3, "the pixel's entries got nothing"
    assert torch.equal(abs_m.t, grad.t[..., :2].abs())


def test_the_cancellation_the_statistics_exist_for():
    from siu3r_amd import density

    c = A.cancel_case()
    refs, ups, abss = A.crafted_ref("cancel")
    r, a = refs[0], abss[0]
    assert (c["margins"] < B.MARGIN).mean() <= B.ZERO_SHARE_CAP
    assert int((np.diff(c["lists"][0][0]) > 0).sum()) == 4, "the footprint must span four tiles (cross-tile atomics)"
    _, _, grad, abs_m = _run_abs(c, ups)
    _check_abs("cancel", refs, abss, grad, abs_m)
    B.assert_elems_close(grad.t[0].cpu(), r["grad"], r["S"], r["bound"], name="cancel grad", extra=r["chain"])
    tol = A.abs_tolerance(r)
    signed, absv = grad.t[0, :, :2].cpu().double().numpy(), abs_m.t[0].cpu().double().numpy()
    print(f"\n[cancel] signed {signed[0]}, abs {absv[0]}, S {r['S'][0, MXY]}, tolerance {tol[0]}")
    assert (np.abs(signed) <= tol).all(), "the signed mean gradient does not cancel"
    assert (absv >= 0.5 * r["S"][:, MXY]).all()
    # through the statistics and the plan: the signed norm keeps the Gaussian, the absolute one grows it
    radii = torch.full((1, 1, 2), 12, dtype=torch.int32, device="cuda")
    sx, sy = 0.5 * 1 * c["W"], 0.5 * 1 * c["H"]
    s_signed, s_abs = density.DensityStats(1, "cuda"), density.DensityStats(1, "cuda", absgrad=True)
    s_signed.accumulate(grad.t[:, :, :2].contiguous(), radii, sx, sy)
    s_abs.accumulate(abs_m.t.contiguous(), radii, sx, sy)
    lo, hi = float(s_signed.grad_accum[0]), float(s_abs.grad_accum[0])
    assert 0.0 <= lo < 1e-3 * hi, (lo, hi)
    ctl = density.DensityControl(grad_threshold=0.5 * (lo + hi), scene_extent=1.0)
    log_scales, logit_op = torch.full((1, 3), -5.0, device="cuda"), torch.zeros(1, device="cuda")
    act = lambda s: int(density.plan(s, log_scales, logit_op, **ctl.thresholds(1.0))[0][0])
    assert act(s_signed) == density.KEEP and act(s_abs) in (density.CLONE, density.SPLIT), (act(s_signed), act(s_abs))


def test_front_end_on_the_state_of_a_real_forward():
    import raster_stages_ref as RS
    from siu3r_amd import raster
    from siu3r_amd.density import DensityStats

    sc = B.forward_scene("k2")
    cams, V, G, H, W = sc["cams"], len(sc["cams"]), sc["means"].shape[0], sc["H"], sc["W"]
    m, cov, op, col = (_dev(sc[k]) for k in ("means", "cov6", "opac", "colors"))
    with torch.no_grad():
        plain = raster.rasterize_views_k2(cams, m, cov, col, op)

    def render(stats):
        leaves = [t.clone().requires_grad_(True) for t in (m, cov, col, op)]
        o = raster.rasterize_views_k2(cams, leaves[0], leaves[1], leaves[2], leaves[3], density_stats=stats)
        return o, leaves

    s_abs, s_signed = DensityStats(G, "cuda", absgrad=True), DensityStats(G, "cuda")
    o, leaves = render(s_abs)
    for k in ("image", "depth", "opacity", "radii"):
        assert torch.equal(o[k], plain[k]), f"{k} changed with density_stats"
    fs = o["state"]
    geo = RS.geometry_ref(W, H)
    E = fs.totals(2)
    lists = [RS.tile_lists_ref(geo, fs["bin_start"][v].cpu().numpy(), fs["entries"][v, :E[v]].cpu().numpy()) for v in range(V)]
    g = np.random.default_rng(11)
    case = dict(kind="k2", V=V, H=H, W=W, cams=cams, rec=fs["rec"].cpu().numpy(), lists=lists, feats=None, walk_cache=[{} for _ in range(V)],
                ups=dict(g_out=g.normal(size=(V, 3, H, W)).astype(np.float32), g_alpha=g.normal(size=(V, H, W)).astype(np.float32),
                         g_depth=g.normal(size=(V, H, W)).astype(np.float32)))
    refs, ups = B.comp_ref(case)
    assert (case["margins"] < B.MARGIN).reshape(V, -1).mean(1).max() <= B.ZERO_SHARE_CAP
    abss = A.case_abs_ref(case, refs, ups)
    up = [_dev(ups[k]) for k in ("g_out", "g_depth", "g_alpha")]
    torch.autograd.backward([o["image"], o["depth"], o["opacity"]], up)
    o2, leaves2 = render(s_signed)
    torch.autograd.backward([o2["image"], o2["depth"], o2["opacity"]], up)
    torch.cuda.synchronize()
    assert torch.equal(s_abs.seen, s_signed.seen) and torch.equal(s_abs.max_radius, s_signed.max_radius) and int(s_abs.seen.sum()) > G // 2
    for a, b in zip(leaves, leaves2):  # the gradients handed back are the signed ones either way (float atomics: not to the bit)
        assert float((a.grad - b.grad).norm()) <= 1e-4 * float(b.grad.norm()) and float(b.grad.norm()) > 0
    radii = o["radii"].cpu().numpy()
    sx, sy = 0.5 * V * W, 0.5 * V * H
    ref, tol = np.zeros(G), np.zeros(G)
    for v in range(V):
        vis = (radii[v] > 0).any(-1)
        h = np.hypot(sx * abss[v]["abs"][:, 0], sy * abss[v]["abs"][:, 1])
        t = A.abs_tolerance(refs[v])
        ref += np.where(vis, h, 0.0)
        tol += np.where(vis, sx * t[:, 0] + sy * t[:, 1] + 4 * U24 * h, 0.0)
        assert not (abss[v]["abs"][~vis] != 0).any(), "a culled Gaussian blends"
    got, got_signed = s_abs.grad_accum.cpu().double().numpy(), s_signed.grad_accum.cpu().double().numpy()
    err = np.abs(got - ref)
    print(f"\n[front-end] grad_accum: worst element {float((err / np.maximum(tol, 1e-300))[tol > 0].max()):.3f} of its tolerance; absgrad / signed norm, median "
          f"{float(np.median(got[got_signed > 0] / got_signed[got_signed > 0])):.2f}")
    assert (err <= tol).all() and float(ref.max()) > 0
    assert (got >= got_signed - tol).all()
    assert (got > 1.5 * got_signed).sum() > G // 10, "the absolute statistics are nowhere larger than the signed ones"


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_refinement_with_absgrad_statistics(optimizer):
    """The scene and the schedule of tests/test_refine_density_gpu.py::test_growth_from_half_the_gaussians (half of the truth's Gaussians,
    60 iterations, events at 20 and 40), with the absolute statistics at gsplat's threshold for them.  A split replaces a Gaussian by two
    sampled children with fresh Adam moments, so the objective steps UP at an event and needs the iterations that follow to come back:
    the schedule leaves twenty after the last event, as that test does."""
    from refine_scenes import BG, FAR, FIELDS, NEAR, _cams, _render, _truth
    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import covariances_from, refine_gaussians

    truth = _truth()
    train, Kt = _cams([0, 1, 2, 3])
    targets = _render(train, Kt, truth["means"], covariances_from(truth["rotations"], truth["scales"]), truth["harmonics"], truth["opacities"])[0]
    G0 = truth["means"].shape[0]
    half = torch.randperm(G0, generator=torch.Generator().manual_seed(21))[: G0 // 2].sort().values.cuda()
    start = {k: v[half].clone() for k, v in truth.items()}
    control = DensityControl(absgrad=True, grad_threshold=8e-4, start=20, every=20, scene_extent=5.0)
    out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=60, density=control, optimizer=optimizer)
    ev = out["density_events"]
    print(f"\nabsgrad refinement ({optimizer}): {G0 // 2} -> {out['means'].shape[0]} Gaussians, events {ev}; objective "
          f"{' '.join(f'[{i}] {losses[i]:.5f}' for i in (0, 19, 20, 39, 40, 59))}")
    assert len(losses) == 60 and [e["iteration"] for e in ev] == [20, 40]
    assert set(ev[0]) == {"rows_in", "rows_out", "pruned", "kept", "cloned", "split", "capped", "iteration"}, "no key is added to density_events"
    assert ev[0]["rows_in"] == G0 // 2 and ev[1]["rows_in"] == ev[0]["rows_out"]
    assert all(out[k].shape[0] == ev[-1]["rows_out"] for k in FIELDS + ("covariances",))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_error_paths_of_the_abs_entry_point():
    c, k3 = B.comp_case("k2_small"), B.comp_case("k3_small")
    st = _composite_state(c)
    V, G, H, W = 1, c["G"], c["H"], c["W"]
    z = lambda *s: torch.zeros(s, device="cuda")
    totals = (z(V, 3, H, W), z(V, H, W), z(V, H, W))
    ups = dict(g_out=np.zeros((V, 3, H, W), np.float32), g_alpha=np.zeros((V, H, W), np.float32), g_depth=np.zeros((V, H, W), np.float32))
    grad, abs_m = _f((V, G, 10)), _f((V, G, 2))
    keep, args = _args(c, st, totals, ups, grad, abs_m)
    arr3, _ = _cam_blocks(k3["cams"])
    _refused("siu3r_raster_composite_rgb_bwd_abs", "mode 0", arr3, *args[1:], outs=[grad, abs_m])
    _refused("siu3r_raster_composite_rgb_bwd_abs", "null pointer", *args[:-1], None, outs=[grad, abs_m])
    _refused("siu3r_raster_composite_rgb_bwd_abs", "null pointer", *args[:-2], None, args[-1], outs=[grad, abs_m])
    _refused("siu3r_raster_composite_rgb_bwd_abs", "bad sizes", *args[:3], -1, *args[4:], outs=[grad, abs_m])
    _ok("siu3r_raster_composite_rgb_bwd_abs", *args[:3], 0, *args[4:-2], None, None)  # an empty scene writes nothing and needs no outputs
    assert grad.untouched() and abs_m.untouched()
