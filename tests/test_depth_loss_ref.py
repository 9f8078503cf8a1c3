"""Pins tests/dense_depth64.py, the reference of the GPU depth-loss tests, on the CPU: the closed-form derivative the HIP kernel implements
agrees with torch autograd in float64, autograd agrees with central differences, and the counting rules hold on crafted views.  Also the
host-side parts of the feature: the two C entry points are declared and exported, depth_weight_schedule, and the argument validation of
refine_gaussians (which runs before any device work, so CPU tensors reach it)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import dense_depth64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES, SPACES = ("l1", "pearson"), ("depth", "inverse")


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,V,H,W", [("noise", 1, 7, 5), ("smooth", 3, 33, 47), ("smooth", 2, 128, 128)])
def test_closed_form_derivative_agrees_with_autograd(kind, V, H, W, mode, space, weights):
    Dm, O, T, Wt = D.make_inputs(kind, V, H, W, seed=V * 100 + H, weights=weights)
    a = D.loss_and_grad(Dm, O, T, Wt, mode, space, route="autograd")
    c = D.loss_and_grad(Dm, O, T, Wt, mode, space, route="closed")
    assert a["loss"] == c["loss"] and a["loss"] > 0 and a["count"] > 0
    for k in ("g_depth", "g_opacity"):
        gmax = float(a[k].abs().max())
        assert gmax > 0
        assert float((a[k] - c[k]).abs().max()) <= 1e-12 * gmax, (k, float((a[k] - c[k]).abs().max()) / gmax)
        assert not bool(a[k][~D.valid_mask(Dm, O, T, Wt, 0.5)].any())


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("mode", MODES)
def test_autograd_gradient_agrees_with_central_differences(mode, space):
    Dm, O, T, Wt = (None if t is None else t.double() for t in D.make_inputs("noise", 2, 9, 11, seed=3, weights=True))
    ref = D.loss_and_grad(Dm, O, T, Wt, mode, space, route="autograd")
    valid = D.valid_mask(Dm, O, T, Wt, 0.5)
    idx = valid.nonzero()[::17][:6]
    assert len(idx) >= 4
    h, worst = 1e-6, 0.0
    f = lambda d, o: float(D.terms(d, o, T, Wt, mode, space)[0])
    for i in idx:
        e = torch.zeros_like(Dm)
        e[tuple(i)] = h
        worst = max(worst, abs((f(Dm + e, O) - f(Dm - e, O)) / (2 * h) - float(ref["g_depth"][tuple(i)])))
        worst = max(worst, abs((f(Dm, O + e) - f(Dm, O - e)) / (2 * h) - float(ref["g_opacity"][tuple(i)])))
    assert worst <= 1e-8, worst


def test_counting_rules_on_crafted_views():
    g = torch.Generator().manual_seed(1)
    V, H, W = 5, 6, 7
    O = torch.ones(V, H, W)
    Dm = 1.0 + 3.0 * torch.rand(V, H, W, generator=g)
    T = 1.0 + 3.0 * torch.rand(V, H, W, generator=g)
    T[1] = 0.0
    T[1, 2, 3] = 2.0   # view 1: one valid pixel
    Dm[2] = 2.5        # view 2: constant x (O = 1: the quotient is exact in every precision)
    T[3] = 1.75        # view 3: constant y
    O[4] = 0.25        # view 4: nothing valid
    for space in SPACES:
        r = D.loss_and_grad(Dm, O, T, None, "pearson", space)
        assert r["count"] == 1.0 and r["valid"].tolist() == [42, 1, 42, 42, 0]
        assert not math.isnan(float(r["per_view"][0])) and bool(torch.isnan(r["per_view"][1:]).all())
        assert abs(r["loss"] - float(r["per_view"][0])) <= 1e-15
        for k in ("g_depth", "g_opacity"):
            assert float(r[k][0].abs().max()) > 0 and not bool(r[k][1:].any())
        l = D.loss_and_grad(Dm, O, T, None, "l1", space)
        assert l["count"] == 127.0 and bool(torch.isnan(l["per_view"][4])) and not bool(torch.isnan(l["per_view"][:4]).any())


@pytest.mark.parametrize("mode", MODES)
def test_all_invalid_input_gives_zero(mode):
    Dm, O, T, _ = D.make_inputs("noise", 2, 5, 5, seed=2)
    for route in ("closed", "autograd"):
        r = D.loss_and_grad(Dm, O * 0.4, T, None, mode, "depth", route=route)
        assert r["loss"] == 0.0 and r["count"] == 0.0 and r["valid"].tolist() == [0, 0]
        assert not bool(r["g_depth"].any()) and not bool(r["g_opacity"].any()) and bool(torch.isnan(r["per_view"]).all())
    Dm[0, 0, 0], O[0, 1, 1], T[1, 2, 2] = float("nan"), float("inf"), float("nan")
    r = D.loss_and_grad(Dm, O, T, None, mode, "inverse")
    assert math.isfinite(r["loss"]) and bool(torch.isfinite(r["g_depth"]).all()) and bool(torch.isfinite(r["g_opacity"]).all())
    assert r["g_depth"][0, 0, 0] == 0 and r["g_opacity"][0, 1, 1] == 0 and r["g_depth"][1, 2, 2] == 0


def test_entry_points_are_declared_and_exported():
    from siu3r_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siu3r_hip.h")).read(), flags=re.S)
    l = _lib.lib()
    for name in ("siu3r_depth_loss_ws", "siu3r_depth_loss"):
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/siu3r_hip.h"
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert len(_lib.SIGNATURES["siu3r_depth_loss"]) == 17 and l.siu3r_depth_loss_ws.restype is C.c_int64
    assert l.siu3r_abi_version() == _lib.ABI_VERSION == 13
    # host function: one record of 11 doubles per 1,024 pixels of a view plus 4 doubles per view
    assert l.siu3r_depth_loss_ws(1, 16, 64) == (11 + 4) * 8
    assert l.siu3r_depth_loss_ws(1, 5, 205) == (2 * 11 + 4) * 8
    assert l.siu3r_depth_loss_ws(3, 1080, 1920) == 3 * (2025 * 11 + 4) * 8
    assert l.siu3r_depth_loss_ws(0, 4, 4) == 0 and l.siu3r_depth_loss_ws(1, 65536, 32768) == 0


def test_depth_weight_schedule():
    from siu3r_amd.refine import depth_weight_schedule

    assert depth_weight_schedule(0.25, 4) == [0.25] * 4 and depth_weight_schedule(0.0, 3) == [0.0] * 3
    s = depth_weight_schedule((1.0, 0.01), 11)
    assert len(s) == 11 and s[0] == 1.0 and s[-1] == 0.01
    for a, b in zip(s[:-1], s[1:]):
        assert abs(b / a - 0.01 ** 0.1) <= 1e-12
    up = depth_weight_schedule((0.3, 0.7), 3)
    assert up[0] == 0.3 and up[2] == 0.7 and abs(up[1] - math.sqrt(0.21)) <= 1e-15
    assert depth_weight_schedule((0.3, 0.7), 1) == [0.3] and depth_weight_schedule((0.3, 0.7), 2) == [0.3, 0.7]
    assert depth_weight_schedule((0.3, 0.7), 0) == [] and depth_weight_schedule(1.0, 0) == []
    for bad in ((0.0, 1.0), (1.0, -0.5), (1.0,), (1.0, 2.0, 3.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError):
            depth_weight_schedule(bad, 5)
    with pytest.raises(ValueError):
        depth_weight_schedule(float("nan"), 5)


def test_refine_validates_the_depth_keywords_before_any_device_work():
    """CPU tensors throughout: every case must raise ValueError from the validation, not RuntimeError from a kernel wrapper"""
    from siu3r_amd.refine import refine_gaussians

    G, V, H, W = 8, 2, 16, 16
    g = torch.Generator().manual_seed(0)
    fields = (torch.rand(G, 3, generator=g), torch.rand(G, 3, generator=g) + 0.1, torch.randn(G, 4, generator=g), torch.rand(G, generator=g),
              torch.rand(G, 3, 4, generator=g))
    images = torch.rand(V, 3, H, W, generator=g)
    cams = (torch.eye(4)[None].repeat(V, 1, 1), torch.eye(3), 0.5, 100.0, (0.0, 0.0, 0.0))
    depths = 1.0 + torch.rand(V, H, W, generator=g)
    call = lambda **kw: refine_gaussians(*fields, images, *cams, iters=2, **kw)
    with pytest.raises(ValueError, match="depths"):
        call(lambda_depth=1.0)
    with pytest.raises(ValueError, match="depths"):
        call(lambda_depth=(1.0, 0.1))
    with pytest.raises(ValueError, match="depths"):
        call(depths=depths[:, :15], lambda_depth=1.0)
    with pytest.raises(ValueError, match="depths"):
        call(depths=depths[:1], lambda_depth=1.0)
    with pytest.raises(ValueError, match="depth_weights"):
        call(depths=depths, depth_weights=torch.ones(V, H, W + 1), lambda_depth=1.0)
    neg = torch.ones(V, H, W)
    neg[1, 3, 3] = -0.5
    with pytest.raises(ValueError, match="depth_weights"):
        call(depths=depths, depth_weights=neg, lambda_depth=1.0)
    for pair in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0)):
        with pytest.raises(ValueError, match="lambda_depth"):
            call(depths=depths, lambda_depth=pair)
    with pytest.raises(ValueError, match="depth_mode"):
        call(depths=depths, lambda_depth=1.0, depth_mode="l2")
    with pytest.raises(ValueError, match="depth_space"):
        call(depths=depths, lambda_depth=1.0, depth_space="log")
    # a valid set of keywords passes the validation and only then meets the GPU-only render
    with pytest.raises(RuntimeError):
        call(depths=depths, depth_weights=torch.ones(V, H, W), lambda_depth=(1.0, 0.1))


def test_depth_loss_argument_errors_need_no_gpu():
    from siu3r_amd import losses

    x = torch.rand(2, 8, 8)
    with pytest.raises(ValueError, match="mode"):
        losses.depth_loss(x, x, x, mode="l2")
    with pytest.raises(ValueError, match="space"):
        losses.depth_loss(x, x, x, space="log")
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_loss(x, x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_loss(x, x, x, weight=x, mode="pearson", space="inverse")


# ---- the per-element parity metric of tests/test_loss_stages_gpu.py, proved on the CPU ----------------------------------------------------
import numpy as np

DCASES = list(D.DEPTH_CASES)


def _tensors(c):
    f = lambda a: None if a is None else torch.from_numpy(a)
    return f(c["D"]), f(c["O"]), f(c["T"]), f(c["Wt"])


@pytest.mark.parametrize("name", DCASES)
def test_closed_form_of_the_crafted_case_agrees_with_autograd(name):
    c, ref = D.depth_case(name), D.depth_ref(name)
    a = D.loss_and_grad(*_tensors(c), c["mode"], c["space"], D.MIN_OPACITY, route="autograd")
    assert a["valid"].tolist() == ref["valid"].tolist()
    assert abs(a["loss"] - ref["out"][0]) <= 1e-12 * abs(a["loss"]) + 1e-300 and abs(a["count"] - ref["out"][1]) <= 1e-12 * a["count"]
    pv = a["per_view"].numpy()
    assert np.array_equal(np.isnan(pv), np.isnan(ref["per_view"])) and np.allclose(np.nan_to_num(pv), np.nan_to_num(ref["per_view"]), rtol=1e-10, atol=0)
    owed = ref["out"][2]  # l1: the maps come without 1 / N
    for k in ("g_depth", "g_opacity"):
        want, got = ref[k] * owed, a[k].numpy()
        assert np.isfinite(got).all() and np.isfinite(want).all()
        fp64 = (ref["tol_" + k] - D.DEPTH_BOUND * np.abs(ref[k])) * owed  # the statistics' own conditioning (pearson), at 2^-53
        d, tol = np.abs(got - want), 1e-9 * np.abs(want) + 1e-12 * np.abs(want).max() + 64 * fp64
        assert (d <= tol).all(), (k, float((d / np.maximum(tol, 1e-300)).max()))
        assert not want[~ref["ok"]].any()


@pytest.mark.parametrize("name", DCASES)
def test_emulation_of_the_kernels_lies_within_the_bound(name):
    c, ref = D.depth_case(name), D.depth_ref(name)
    em = D.depth_emulate(name)
    w = D.depth_worst(em, ref, c["grad"])
    print(name, w)
    assert max(w.values()) <= 1.0, w
    if c["grad"]:
        assert not em["g_depth"][~ref["ok"]].any() and not em["g_opacity"][~ref["ok"]].any()


DEPTH_FAULT_SHOWS = {
    "valid_ge": ("p1023_views3", "p1024", "p1025_views3", "p2049_l1_inverse"),
    "inverse_sign": ("p4", "p1023_views3", "equal_pixels_inverse", "views_constant"),
    "uncounted_in_mean": ("views_none_one", "views_constant"),
    "tail_fill": ("p1", "p3_views3", "p5_views3", "p1025_views3", "p2049_views3"),
}


@pytest.mark.parametrize("fault", D.DEPTH_FAULTS)
def test_one_depth_line_wrong_falls_outside_the_bound(fault):
    for name in DEPTH_FAULT_SHOWS[fault]:
        c = D.depth_case(name)
        w = D.depth_worst(D.depth_emulate(name, fault), D.depth_ref(name), c["grad"])
        assert max(w.values()) > 1.0, (fault, name, w)


def test_branch_population_of_the_depth_cases():
    pop = {n: D.depth_ref(n)["pop"] for n in DCASES}
    cs = {n: D.depth_case(n) for n in DCASES}
    assert {c["H"] * c["W"] for c in cs.values()} >= {1, 3, 4, 5, 1023, 1024, 1025, 2049, 513 * 512}
    assert {c["V"] for c in cs.values()} == {1, 3}
    combos = {(c["mode"], c["space"], c["Wt"] is not None, c["grad"]) for c in cs.values()}
    assert {(m, s) for m, s, _, _ in combos} == {(m, s) for m in MODES for s in SPACES}
    assert {(m, w) for m, _, w, _ in combos} == {(m, w) for m in MODES for w in (False, True)} and {(m, g) for m, _, _, g in combos} == {(m, g) for m in MODES for g in (False, True)}
    for n in ("p3_views3", "p5_views3", "p1023_views3", "p1025_views3", "p2049_views3"):  # odd planes: the bases of views 1 and 2 are not 16-byte aligned
        assert pop[n]["scalar_views"] == 2 and pop[n]["tail"] > 0
    for n in DCASES:
        if D.DEPTH_CASES[n][7] == "thresholds":
            rows = 4 if cs[n]["Wt"] is not None else 3
            assert pop[n]["threshold_valid"] == 3 * rows and pop[n]["threshold_invalid"] == 6 * rows, (n, pop[n])
    assert pop["nonfinite"]["nonfinite_invalid"] == 12 and pop["nonfinite_l1"]["nonfinite_invalid"] == 12
    assert pop["views_none_one"]["uncounted_views"] == 2 and D.depth_ref("views_none_one")["valid"].tolist()[:2] == [0, 1]
    assert D.depth_ref("views_none_one_l1")["valid"].tolist()[:2] == [0, 1] and np.isnan(D.depth_ref("views_none_one_l1")["per_view"]).tolist() == [True, False, False]
    assert pop["views_constant"]["uncounted_views"] == 2 and pop["views_constant"]["counted_views"] == 1
    assert pop["equal_pixels"]["zero_subgradient"] > 10 and pop["equal_pixels_inverse"]["zero_subgradient"] > 10
    assert all(p["zero_subgradient"] == 0 for n, p in pop.items() if not n.startswith("equal_pixels"))
    assert pop["two_chunks_of_records"]["records"] > 256 and pop["p1025_views3"]["records"] == 2
    assert 3e-4 < D.depth_ref("small_loss")["out"][0] < 6e-4
    # on the small loss the fp64 allowance of the statistics is far below the float32 store: the bound stays a few ulps of the element
    r = D.depth_ref("small_loss")
    store = D.DEPTH_BOUND * np.abs(r["g_depth"])
    assert float(np.median((r["tol_g_depth"] - store)[r["ok"]] / store[r["ok"]])) < 1e-2
