"""CPU tests of the bilateral grid (csrc/bilagrid.hip, losses.apply_bilagrid, cameras.CameraControl): the two float64 forms agree, the float32
emulation of every kernel stays inside the derived bounds of dense_bilagrid64.py, each listed wrong answer exceeds them, the gradient cases
keep their distance from the kinks, the control's validation, the C ABI's refusals and the compiler's resource remarks."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import dense_bilagrid64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("siu3r_bilagrid_apply", "siu3r_bilagrid_apply_bwd", "siu3r_bilagrid_tv_ws", "siu3r_bilagrid_tv")
SMALL = [n for n in D.CASES if n not in ("c_default", "g_staged_side", "g_global_side")]  # the cases every mutation is tried on


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, float64 reference, bounds) of a case, computed once"""
    img, grids, g_out = D.make_case(name)
    return (img, grids, g_out), D.explicit(img, grids, g_out), D.bounds(img, grids, g_out)


def _worst(got, ref, bound):
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


def test_the_two_float64_forms_agree():
    """explicit formulas against grid_sample and its autograd: the convention, forward and all gradients; 1e-13 relative to the largest value"""
    for name in D.CASES:
        (img, grids, g_out), ref, _ = _case(name)
        out, g_in, g_grids = D.by_grid_sample(img, grids, g_out)
        for key, other in (("out", out), ("g_in", g_in), ("g_grids", g_grids)):
            err, scale = float(np.abs(ref[key] - other).max()), float(np.abs(other).max())
            assert err <= 1e-13 * max(scale, 1e-30), (name, key, err, scale)
    img, grids = D.kink_case()
    assert float(np.abs(D.explicit(img, grids)["out"] - D.by_grid_sample(img, grids)).max()) <= 1e-14
    value, grad, _ = D.tv(D.smooth_grids(2, 3, 4, 5, 3))
    A = torch.tensor(D.smooth_grids(2, 3, 4, 5, 3), dtype=torch.float64)
    want = sum(((A.narrow(ax, 1, A.shape[ax] - 1) - A.narrow(ax, 0, A.shape[ax] - 1)) ** 2).mean(dim=(1, 2, 3, 4)).mean() for ax in (2, 3, 4))
    assert abs(value - float(want)) <= 1e-15 and np.isfinite(grad).all()


def test_gradient_cases_keep_their_distance_from_the_kinks():
    """no pixel of a gradient case has lum within 1e-4 of 0 or 1 or fz within 1e-4 (L - 1) of an integer, so no gradient test excludes a pixel;
    and fp32 puts every pixel of every case in the float64 x and y cell (the forward bound's premise)"""
    for name, (V, H, W, (Gh, Gw, L), _) in D.CASES.items():
        img = D.make_case(name)[0]
        d_lum, d_fz = D.kink_distances(img, L)
        assert d_lum >= D.KINK and d_fz >= D.KINK, (name, d_lum, d_fz)
        for n, g in ((H, Gh), (W, Gw)):
            assert np.array_equal(D.coords(n, g, np.float32)[1], D.coords(n, g, np.float64)[1]), (name, n, g)
    lo, hi = D.kink_distances(D.kink_case()[0], 5)
    assert lo == 0.0 and hi == 0.0, "the kink case must sit on the kinks"


def test_emulation_stays_inside_every_bound():
    worst = {}
    for name in D.CASES:
        (img, grids, g_out), ref, bound = _case(name)
        emu = D.explicit(img, grids, g_out, dtype=np.float32)
        for key in ("out", "g_in", "g_grids"):
            worst[f"{name}/{key}"] = _worst(emu[key], ref[key], bound[key])
    img, grids = D.kink_case()
    worst["kinks/out"] = _worst(D.explicit(img, grids, dtype=np.float32)["out"], D.explicit(img, grids)["out"], D.bounds(img, grids)["out"])
    for shape in ((2, 2, 2, 2), (2, 3, 4, 5), (1, 16, 16, 8)):
        A = D.smooth_grids(*shape, seed=11)
        value, grad, _ = D.tv(A)
        ev, eg = D.tv_emulated(A)
        bv, bg = D.tv_bounds(A)
        worst[f"tv{shape}/value"] = abs(float(ev) - value) / bv
        worst[f"tv{shape}/grad"] = _worst(eg, grad, bg)
    print("\nworst |emulation - float64| / bound:", json.dumps({k: round(v, 4) for k, v in worst.items()}))
    path = os.path.join(ROOT, "profiles", "bilagrid_parity.json")
    if os.access(os.path.dirname(path), os.W_OK):
        record = json.load(open(path)) if os.path.exists(path) else {}
        record["emulation"] = {k: round(v, 4) for k, v in worst.items()}
        with open(path, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


@pytest.mark.parametrize("mut", D.MUTATIONS)
def test_each_wrong_answer_exceeds_the_bound(mut):
    """a float64 evaluation of each wrong variant leaves the bound of at least one case, in the output the variant touches"""
    keys = ("g_in",) if "guidance_grad" in mut else ("out", "g_in", "g_grids")
    ratios = {}
    for name in SMALL:
        (img, grids, g_out), ref, bound = _case(name)
        bad = D.explicit(img, grids, g_out, mut=mut)
        ratios[name] = max(_worst(bad[k], ref[k], bound[k]) for k in keys)
    print(f"\n{mut}: worst ratio per case", {k: f"{v:.3g}" for k, v in ratios.items()})
    assert max(ratios.values()) > 1.0
    if mut == "guidance_grad_unclamped":
        assert ratios["h_clamped"] > 1.0, "only a case with clamped pixels can tell"


@pytest.mark.parametrize("mut", D.TV_MUTATIONS)
def test_each_wrong_total_variation_exceeds_the_bound(mut):
    A = D.smooth_grids(2, 3, 4, 5, seed=11)
    value, grad, _ = D.tv(A)
    bv, bg = D.tv_bounds(A)
    bad_v, bad_g, _ = D.tv(A, mut=mut)
    assert abs(bad_v - value) > bv and float((np.abs(bad_g - grad) / bg).max()) > 1.0


def test_identity_grid_returns_the_input_bits_in_the_emulation():
    img = D.image(2, 9, 11, 8, seed=4, lo=-0.5, hi=1.5)
    img[0, :, 0, 0] = (-0.0, 0.0, 1e-30)
    out = D.explicit(img, D.identity_grids(2, 5, 4, 8), dtype=np.float32)["out"]
    assert out.dtype == np.float32 and np.array_equal(out, img)
    assert not np.signbit(out[0, 0, 0, 0]), "a -0 comes back as +0"


def test_new_symbols_are_declared_exported_and_signed():
    from siu3r_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siu3r_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(siu3r_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for s in SYMBOLS:
        assert s in declared and hasattr(l, s) and s in _lib.SIGNATURES, s
    assert l.siu3r_abi_version() == _lib.ABI_VERSION == 13
    assert l.siu3r_bilagrid_tv_ws(6, 8, 16, 16) == 8 * 576  # 6 x 12 x 8 x 16 x 16 elements, 256 per workgroup
    assert l.siu3r_bilagrid_tv_ws(1, 2, 2, 2) == 8 and l.siu3r_bilagrid_tv_ws(64, 16, 64, 64) == 8 * 1024
    for bad in ((0, 8, 16, 16), (1, 1, 16, 16), (1, 17, 16, 16), (1, 8, 1, 16), (1, 8, 16, 1025)):
        assert l.siu3r_bilagrid_tv_ws(*bad) == 0, bad


def test_abi_refusals_before_any_device_work():
    """every argument check answers through siu3r_last_error() without touching a device: the pointers are never dereferenced"""
    from siu3r_amd import _lib

    l = _lib.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    st = (C.c_int64 * 4)(48, 16, 4, 1)
    neg = (C.c_int64 * 4)(48, 16, -4, 1)

    def refused(rc, word):
        assert rc == 1 and word in l.siu3r_last_error().decode(), (rc, l.siu3r_last_error())

    refused(l.siu3r_bilagrid_apply(None, st, p, 1, 4, 4, 2, 2, 2, p, None), "null")
    refused(l.siu3r_bilagrid_apply(p, None, p, 1, 4, 4, 2, 2, 2, p, None), "null")
    refused(l.siu3r_bilagrid_apply(p, st, None, 1, 4, 4, 2, 2, 2, p, None), "null")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 4, 4, 2, 2, 2, None, None), "null")
    refused(l.siu3r_bilagrid_apply(p, st, p, 0, 4, 4, 2, 2, 2, p, None), "views")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 0, 4, 2, 2, 2, p, None), "empty")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 4, 4, 1, 2, 2, p, None), "levels")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 4, 4, 17, 2, 2, p, None), "levels")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 4, 4, 2, 1, 2, p, None), "grid")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 4, 4, 2, 2, 1025, p, None), "grid")
    refused(l.siu3r_bilagrid_apply(p, neg, p, 1, 4, 4, 2, 2, 2, p, None), "negative")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 1 << 16, 1 << 15, 2, 2, 2, p, None), "32-bit")
    refused(l.siu3r_bilagrid_apply(p, st, p, 1, 1, (1 << 22) + 1, 2, 2, 2, p, None), "pixel centres")
    refused(l.siu3r_bilagrid_apply_bwd(p, st, p, None, 1, 4, 4, 2, 2, 2, p, p, None), "null")
    refused(l.siu3r_bilagrid_apply_bwd(p, neg, p, p, 1, 4, 4, 2, 2, 2, p, p, None), "negative")
    refused(l.siu3r_bilagrid_apply_bwd(p, st, p, p, 1, 4, 4, 17, 2, 2, p, p, None), "levels")
    assert l.siu3r_bilagrid_apply_bwd(p, st, p, p, 1, 4, 4, 2, 2, 2, None, None, None) == 0, "neither gradient asked for: nothing is launched"
    refused(l.siu3r_bilagrid_tv(None, 1, 2, 2, 2, 1.0, None, p, p, None), "null")
    refused(l.siu3r_bilagrid_tv(p, 1, 2, 2, 2, 1.0, None, p, None, None), "null")
    refused(l.siu3r_bilagrid_tv(p, 1, 2, 2, 2, 1.0, None, None, p, None), "workspace")
    refused(l.siu3r_bilagrid_tv(p, 1, 2, 2, 2, 1.0, None, p + 4, p, None), "workspace")
    refused(l.siu3r_bilagrid_tv(p, 1, 1, 2, 2, 1.0, None, p, p, None), "levels")
    refused(l.siu3r_bilagrid_tv(p, 1, 2, 2, 2, float("nan"), None, p, p, None), "finite")


def test_camera_control_validation_of_the_new_fields():
    from siu3r_amd.cameras import CameraControl

    for ok in (True, "affine", "bilagrid"):
        CameraControl(exposure=ok).validate(3)
    CameraControl(pose=True, exposure=False).validate(3)
    CameraControl(pose=False, exposure="bilagrid", bilagrid_shape=(2, 2, 2), lambda_tv=0.0).validate(2)
    for bad in ("bilateral", "Affine", "", "true"):
        with pytest.raises(ValueError, match="exposure"):
            CameraControl(exposure=bad).validate(3)
    with pytest.raises(ValueError, match="both off"):
        CameraControl(pose=False, exposure=False).validate(3)
    for bad in ((16, 16), (16, 16, 1), (1, 16, 8), (16, 1, 8), (16, 16, 17), (16, 2000, 8), (16.0, 16, 8), (True, 16, 8), "16x16x8", None):
        with pytest.raises(ValueError, match="bilagrid_shape"):
            CameraControl(exposure="bilagrid", bilagrid_shape=bad).validate(3)
    for bad in (0.0, -1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lr_bilagrid"):
            CameraControl(lr_bilagrid=bad).validate(3)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lambda_tv"):
            CameraControl(lambda_tv=bad).validate(3)
    c = CameraControl(lr_bilagrid=2e-3, lr_final_scale=0.1)
    r = c.bilagrid_rates(200)
    assert len(r) == 200 and r[0] == 2e-3 and abs(r[-1] - 2e-4) <= 1e-18 and abs(r[100] / 2e-3 - 0.1 ** (100 / 199)) <= 1e-12
    assert len(c.rates(200)[0]) == 3 and CameraControl(start=5).bilagrid_rates(5) == []


def test_refine_rejects_an_unknown_exposure_before_any_device_work():
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.refine import refine_gaussians

    G, V = 4, 3
    args = (torch.zeros(G, 3), torch.ones(G, 3), torch.ones(G, 4), torch.full((G,), 0.5), torch.zeros(G, 3, 4), torch.zeros(V, 3, 16, 16),
            torch.eye(4).repeat(V, 1, 1), torch.eye(3), 0.5, 100.0, (0, 0, 0))
    with pytest.raises(ValueError, match="exposure"):
        refine_gaussians(*args, cameras=CameraControl(exposure="bilateral"))
    with pytest.raises(ValueError, match="bilagrid_shape"):
        refine_gaussians(*args, cameras=CameraControl(exposure="bilagrid", bilagrid_shape=(16, 16, 32)))


def test_code_object_resources():
    """no kernel of the unit uses scratch memory or spills (the grid gradient's 96 sums per thread live in registers)"""
    from siu3r_amd import build as B

    res = B.kernel_resources("bilagrid.hip")
    for n in ("bilagrid_stream_kernelILb0E", "bilagrid_stream_kernelILb1E", "bilagrid_ggrid_kernel", "bilagrid_tv_kernel", "bilagrid_tv_sum_kernel"):
        assert any(n in k for k in res), (n, sorted(res))
    for k, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
