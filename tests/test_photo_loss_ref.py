"""Pins tests/dense_photo64.py, the reference of the GPU photometric-loss tests, on the CPU: its SSIM is metrics.ssim, its autograd gradient
agrees with central differences, and the closed-form derivative the HIP kernel implements agrees with autograd."""
import numpy as np
import pytest
import torch

from siu3r_amd import metrics

import dense_photo64 as D


@pytest.mark.parametrize("H,W", [(24, 37), (33, 33)])
@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("C", [1, 3])
def test_restated_ssim_is_metrics_ssim(H, W, data_range, C):
    g = torch.Generator().manual_seed(H * 100 + C)
    p = torch.rand(2, C, H, W, generator=g, dtype=torch.float64) * data_range
    t = (p + 0.2 * data_range * torch.randn(2, C, H, W, generator=g, dtype=torch.float64)).clamp(0, data_range)
    m = D.ssim_map(p, t, data_range)
    assert m.shape == (2, C, H - 10, W - 10)
    for v in range(2):
        ref = metrics.ssim(p[v].permute(1, 2, 0).numpy(), t[v].permute(1, 2, 0).numpy(), data_range=data_range)
        assert abs(float(m[v].mean()) - ref) <= 1e-12, (float(m[v].mean()), ref)


def test_autograd_gradient_agrees_with_central_differences():
    g = torch.Generator().manual_seed(5)
    p = torch.rand(1, 2, 14, 15, generator=g, dtype=torch.float64)
    t = torch.rand(1, 2, 14, 15, generator=g, dtype=torch.float64)
    for lam in (0.2, 1.0):
        _, grad = D.loss_and_grad(p, t, lam)
        h = 1e-6
        worst = 0.0
        for idx in [(0, 0, 0, 0), (0, 1, 7, 7), (0, 0, 13, 14), (0, 1, 3, 11), (0, 0, 6, 2)]:
            e = torch.zeros_like(p)
            e[idx] = h
            fd = (float(D.photo_loss(p + e, t, lam)[0]) - float(D.photo_loss(p - e, t, lam)[0])) / (2 * h)
            worst = max(worst, abs(fd - float(grad[idx])))
        assert worst <= 1e-8, worst


@pytest.mark.parametrize("flat", [False, True])
def test_closed_form_derivative_agrees_with_autograd(flat):
    g = torch.Generator().manual_seed(6)
    p = torch.rand(2, 3, 30, 41, generator=g, dtype=torch.float64)
    t = torch.rand(2, 3, 30, 41, generator=g, dtype=torch.float64)
    if flat:  # exactly flat regions: both clamps active
        p[:, :, :16, :20] = 0.5
        t[:, :, 8:, 15:] = 1.0
    _, grad = D.loss_and_grad(p, t, 1.0)  # loss = 1 - SSIM
    cf = D.closed_form_grad(p, t)
    assert float((cf + grad).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))


# ---- the per-element parity metric of tests/test_loss_stages_gpu.py, proved on the CPU ----------------------------------------------------
import os
import re

import dense_raster_bwd64 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(D.PHOTO_CASES)


def _ratio(got, ref, S, bound, name, extra):
    """the worst element as a fraction of its tolerance; a NaN of the reference (a term switched off) must meet a NaN"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    if (np.isnan(got) != nan).any():
        return float("inf")
    return B.worst_ratio(np.where(nan, 0.0, got), np.where(nan, 0.0, ref), S, bound, extra)[0]


def test_window_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "siu3r_amd", "csrc", "photo_loss.hip")).read()
    body = re.search(r"GW\[TAPS\]\s*=\s*\{(.*?)\}", text, re.S).group(1)
    lit = np.array([np.float32(x.rstrip("f")) for x in re.findall(r"[0-9.]+f", body)], np.float32)
    assert lit.shape == (11,) and np.array_equal(lit, D.GW32)
    assert D.TILE == int(re.search(r"constexpr int TILE = (\d+)", text).group(1))


@pytest.mark.parametrize("name", CASES)
def test_closed_form_of_the_crafted_case_agrees_with_autograd(name):
    """float64 autograd of the dense restatement (unshifted E[p^2] - mu^2, so its own rounding is 2^-53 in units of max |p|^2: the unshifted
    scale at 2^-53 instead of u, four-fold) plus the allowance of the undecided windows, where autograd takes the exact branch"""
    c, ref, un = D.photo_case(name), D.photo_ref(name), D.photo_ref(name, shifted=False)
    (loss, l1, ss), grad = D.loss_and_grad(torch.from_numpy(c["P"]), torch.from_numpy(c["T"]), c["lam"], c["dr"])
    f64 = 4 * 2.0 ** -29
    for k, v in enumerate((loss, l1, ss)):
        if v is None:
            assert np.isnan(ref["out"][k])
        else:
            assert abs(v - ref["out"][k]) <= f64 * D.PHOTO_BOUND * un["S_out"][k] + 1e-15 * abs(v), (k, v, ref["out"][k])
    if c["grad"]:
        tol = f64 * D.PHOTO_BOUND * un["S_grad"] + ref["extra_grad"] + un["extra_grad"] + 1e-14 * np.abs(ref["grad"])
        d = np.abs(grad.numpy() - ref["grad"])
        assert (d <= tol).all(), float((d / np.maximum(tol, 1e-300)).max())
    n_l1, n_ss = c["V"] * c["C"] * c["H"] * c["W"], c["V"] * c["C"] * (c["H"] - 10) * (c["W"] - 10)
    assert ref["partials"].shape == (c["V"] * c["C"] * -(-c["H"] // 32) * -(-c["W"] // 32), 2)
    if l1 is not None:
        assert abs(ref["partials"][:, 0].sum() / n_l1 - l1) <= 1e-12 * l1
    if ss is not None:
        assert abs(ref["partials"][:, 1].sum() / n_ss - ref["out"][2]) <= 1e-15


@pytest.mark.parametrize("name", CASES)
def test_float32_emulation_of_the_kernel_lies_within_the_bound(name):
    w = D.photo_compare(D.photo_emulate(name), D.photo_ref(name), _ratio)
    print(name, w)
    assert max(w.values()) <= 1.0, w
    if D.photo_case(name)["grad"] is False:
        assert D.photo_emulate(name)["grad"] is None


# fault -> the cases that must reject it (every listed one is asserted)
FAULT_SHOWS = {
    "no_shift": ("offset_1e4", "offset_1e4_right_tile", "offset_pair", "outlier_centre"),
    "swap_shift": ("offset_pair",),
    "unclamped_centre": ("offset_1e4_right_tile",),
    "valid_plus_one": ("one_window_11x12", "one_window_12x11_nograd", "one_column_43x74", "ssim_only_nograd"),
    "ownership": ("tile_edge_32x33", "sliver_33x43", "third_tile_74x42"),
    "clamp_inverted": ("pred_flat", "flat_off_centre", "one_window_11x12"),
    "dmu_term": ("one_window_11x12", "offset_pair", "range_255"),
    "tap_shift": ("one_window_11x12", "third_tile_74x42"),
    "l1_sign": ("one_window_11x12", "l1_only", "one_column_43x74"),
    "norm_hw": ("one_window_11x12", "ssim_only_nograd", "flat_equal"),
}


@pytest.mark.parametrize("fault", D.PHOTO_FAULTS)
def test_one_line_wrong_falls_outside_the_bound(fault):
    assert FAULT_SHOWS[fault]
    for name in FAULT_SHOWS[fault]:
        w = D.photo_compare(D.photo_emulate(name, fault), D.photo_ref(name), _ratio)
        assert max(w.values()) > 1.0, (fault, name, w)


def test_the_bound_is_in_shifted_units():
    """the kernel without its shift is rejected on the cases built for it, and the scale of a kernel without the shift is what would let it
    pass: orders of magnitude wider"""
    assert set(FAULT_SHOWS["no_shift"]) <= set(D.SHIFT_CASES)
    for name in ("offset_1e4", "offset_pair"):
        ref, un = D.photo_ref(name), D.photo_ref(name, shifted=False)
        assert float(np.median(un["S_grad"] / ref["S_grad"])) > 100.0
        assert max(D.photo_compare(D.photo_emulate(name, "no_shift"), un, _ratio).values()) <= 1.0


GT = lambda n: (">=", n)
POPULATION = {
    "one_window_11x12": dict(windows=2, tiles=1, halo_windows=0),
    "one_window_12x11_nograd": dict(windows=12, tiles=1),
    "tile_edge_32x33": dict(tiles=2, tiles_without_window=1, halo_windows=GT(1)),
    "sliver_33x43": dict(tiles=4, tiles_without_window=2),
    "no_window_tile_42x75": dict(tiles=6, tiles_without_window=3),
    "one_column_43x74": dict(tiles=6, tiles_without_window=2),
    "third_tile_74x42": dict(tiles=6, tiles_without_window=4),
    "third_tile_75x32_nograd": dict(tiles=3, tiles_without_window=0, halo_windows=0),
    "flat_equal": dict(equal_pixels=33 * 42, clamp_pp=736, undecided=0),
    "flat_off_centre": dict(undecided=GT(1000), clamp_tt=GT(1000), equal_pixels=0),
    "pred_flat": dict(clamp_pp=GT(500), clamp_tt=0),
    "target_flat": dict(clamp_tt=726, clamp_pp=0),
    "flat_across_seam": dict(undecided=GT(100), clamp_tt=GT(100), tiles=6),
    "outlier_centre": dict(tiles=6),
    "many_planes_300": dict(windows=300, tiles=1),
    "l1_only": dict(windows=0, tiles=4),
    "l1_only_equal": dict(windows=0, tiles=2, equal_pixels=2 * 12 * 33),
}


@pytest.mark.parametrize("name", CASES)
def test_branch_population_of_the_crafted_case(name):
    c, pop = D.photo_case(name), D.photo_ref(name)["pop"]
    assert c["H"] <= 80 and c["W"] <= 80 and (c["V"] * c["C"] <= 6 or name == "many_planes_300")
    if D.PHOTO_CASES[name][4] != "flat_equal":
        assert pop["equal_pixels"] == 0
    for k, want in POPULATION.get(name, {}).items():
        assert (pop[k] >= want[1]) if isinstance(want, tuple) else (pop[k] == want), (name, k, pop[k], want)


def test_the_case_list_covers_what_it_claims():
    cs = [D.photo_case(n) for n in CASES]
    assert {11, 12, 32, 33, 42, 43, 74, 75} <= {c["H"] for c in cs} | {c["W"] for c in cs} and all(c["H"] != c["W"] or n == "many_planes_300" for n, c in zip(CASES, cs))
    assert {0.0, 1.0, float(np.float32(0.2)), D.LAM_NEAR_ONE} == {c["lam"] for c in cs}
    assert {(c["grad"], c["lam"] == 0.0) for c in cs} == {(True, True), (True, False), (False, True), (False, False)}
    assert {1, 6, 300} <= {c["V"] * c["C"] for c in cs}
    lays = {D.PHOTO_CASES[n][8] for n in CASES} | {D.PHOTO_CASES[n][9] for n in CASES}
    assert lays == {"nchw", "nhwc", "window", "nhwc_spare", "view0", "chan0", "same_views"}
    assert any(D.PHOTO_CASES[n][8] != D.PHOTO_CASES[n][9] for n in CASES)
    # the sentinel of the slack is not image data, and the layouts address what they claim
    for n in ("no_window_tile_42x75", "third_tile_74x42"):
        lay = D.photo_case(n)["play"]
        own = D.owned_mask(lay)
        assert 0 < own.sum() < own.size and (lay["parent"][~own].view(np.int32) == D.SENT_BITS).all() and not (lay["parent"][own].view(np.int32) == D.SENT_BITS).any()
