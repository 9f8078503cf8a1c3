"""The float64 reference of the absolute-gradient densification statistics (tests/dense_absgrad64.py) checked on the CPU, before
tests/test_absgrad_gpu.py holds siu3r_raster_composite_rgb_bwd_abs to it: its signed sums are composite_bwd64's, it lies between |signed|
and S, it IS "absolute value per pixel, then sum" (shown through the linearity of the backward in its upstream gradient, not through the
hand-written terms), the comparison metric rejects |signed sum|, and the Python surface carries the flag."""
import numpy as np
import pytest

import dense_absgrad64 as A
import dense_raster_bwd64 as B

MXY = [B.MX, B.MY]


@pytest.mark.parametrize("name", ["k2_small", "k2_ragged", "one_tile", "cancel"])
def test_signed_sums_are_those_of_composite_bwd64_and_abs_lies_between_signed_and_S(name):
    refs, _, abss = A.crafted_ref(name)
    for r, a in zip(refs, abss):
        S = r["S"][:, MXY]
        assert (np.abs(a["signed"] - r["grad"][:, MXY]) <= 1e-12 * S).all(), "not the same walk"
        assert (np.abs(a["signed"]) <= a["abs"] + 1e-12 * S).all() and (a["abs"] <= S * (1 + 1e-12)).all()
        assert (a["abs"][r["n_add"] == 0] == 0).all()
        assert int(a["n_term"].sum()) > 0 and float(a["abs"].max()) > 0


def test_abs_is_the_sum_over_pixels_of_the_absolute_single_pixel_backward():
    """the backward is linear in its upstream gradient: with the gradient restricted to one pixel, composite_bwd64's grad IS that pixel's
    term, so sum_p |grad(upstream restricted to p)| is the statistic by definition, whatever the terms are"""
    c = A.one_tile_case()
    refs, ups, abss = A.crafted_ref("one_tile", "all")
    assert c["geo"]["T"] == 1 and refs[0]["counts"]["clamped"] > 0 and refs[0]["counts"]["blend"] > 1000, refs[0]["counts"]
    H, W = c["H"], c["W"]
    total = np.zeros((c["G"], 2))
    for y in range(H):
        for x in range(W):
            one = {k: np.zeros_like(v[0]) for k, v in ups.items()}
            for k in one:
                one[k][..., y, x] = ups[k][0][..., y, x]
            r = B.composite_bwd64("k2", c["cams"][0], c["rec"][0], c["lists"][0], one["g_out"], one["g_alpha"], one["g_depth"], cache=c["walk_cache"][0])
            total += np.abs(r["grad"][:, MXY])
    S = refs[0]["S"][:, MXY]
    assert (np.abs(total - abss[0]["abs"]) <= 1e-12 * S).all()
    # and it is not the absolute value of the sum: most Gaussians of the case see terms of both signs
    assert (abss[0]["abs"] > np.abs(abss[0]["signed"]) * 1.5).any()


@pytest.mark.parametrize("name", ["k2_small", "cancel"])
def test_the_metric_rejects_the_absolute_value_of_the_signed_sum(name):
    refs, _, abss = A.crafted_ref(name)
    r, a = refs[0], abss[0]
    S, chain = r["S"][:, MXY], r["chain"][:, MXY]
    assert not B.rejects(a["abs"], a["abs"], S, r["bound"], chain)
    assert B.rejects(np.abs(a["signed"]), a["abs"], S, r["bound"], chain), "|signed sum| passes for the per-pixel absolute sum"
    assert (A.abs_tolerance(r) == r["bound"] * S + chain).all()


def test_the_cancellation_case_cancels():
    refs, _, abss = A.crafted_ref("cancel")
    r, a = refs[0], abss[0]
    assert r["n_add"][0] > 300 and int((np.diff(A.cancel_case()["lists"][0][0]) > 0).sum()) == 4, "the footprint must span four tiles"
    tol = A.abs_tolerance(r)
    assert (np.abs(a["signed"]) <= 1e-12 * r["S"][:, MXY]).all() and (np.abs(r["grad"][:, MXY]) <= tol).all()
    assert (a["abs"] >= 0.5 * r["S"][:, MXY]).all() and (a["abs"] > 1000 * tol).all()


def test_the_python_surface_carries_the_flag():
    from siu3r_amd.density import DensityControl, DensityStats

    assert DensityControl().absgrad is False and DensityControl(absgrad=True).absgrad is True
    assert DensityControl(absgrad=True).grad_threshold == DensityControl().grad_threshold, "the threshold is not changed automatically"
    assert DensityStats(4, "cpu").absgrad is False and DensityStats(4, "cpu", absgrad=True).absgrad is True
    s = DensityStats(4, "cpu", absgrad=True)
    assert s.G == 4 and s.grad_accum.shape == (4,) and s.seen.shape == (4,) and s.max_radius.shape == (4,)


def test_code_object_resources_of_the_abs_instantiation():
    """composite_rgb_bwd_kernel<false, ABS = true> spills nothing and costs exactly the two extra slots per staged entry (256 x 2 floats) of
    LDS over the plain K2 instantiation; the gsplat-family instantiation keeps the plain one's LDS"""
    from siu3r_amd import build as Bd

    res = Bd.kernel_resources("raster_bwd.hip")
    pick = lambda tag: [r for k, r in res.items() if "composite_rgb_bwd_kernel" + tag in k]
    (plain,), (absr,), (k3,) = pick("ILb0ELb0EE"), pick("ILb0ELb1EE"), pick("ILb1ELb0EE")
    assert not pick("ILb1ELb1EE"), "K3 has no ABS instantiation"
    for r in (plain, absr, k3):
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert absr["LDS Size [bytes/block]"] == plain["LDS Size [bytes/block]"] + 2048
    assert k3["LDS Size [bytes/block]"] == plain["LDS Size [bytes/block]"]
    assert absr["Occupancy [waves/SIMD]"] == plain["Occupancy [waves/SIMD]"]


def test_the_binding_declares_the_new_entry_point():
    from siu3r_amd import _lib

    sig = _lib.SIGNATURES["siu3r_raster_composite_rgb_bwd_abs"]
    plain = _lib.SIGNATURES["siu3r_raster_composite_rgb_bwd"]
    assert sig[:-1] == plain and sig[-2] == sig[-1] == plain[-1], "the plain call's arguments, then abs_mean2d in front of the stream"
    assert _lib.ABI_VERSION == 13
