"""csrc/bilagrid.hip on the GPU through losses.apply_bilagrid / bilagrid_tv and through the C ABI, element by element against the float64
reference and the derived bounds of dense_bilagrid64.py.  The cases (and their letters) are that module's list; every launch is repeated
once and must return the same bits."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import dense_bilagrid64 as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 777.0
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _record_the_worst_ratios():
    """after the module's tests: the worst |gpu - float64| / bound of this run goes to profiles/bilagrid_parity.json"""
    yield
    path = os.path.join(ROOT, "profiles", "bilagrid_parity.json")
    if _worst and os.access(os.path.dirname(path), os.W_OK):
        record = json.load(open(path)) if os.path.exists(path) else {}
        record["gpu"] = dict(_worst, gpu=torch.cuda.get_device_name())
        with open(path, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")


@functools.lru_cache(maxsize=None)
def _case(name):
    img, grids, g_out = D.make_case(name)
    return (img, grids, g_out), D.explicit(img, grids, g_out), D.bounds(img, grids, g_out)


def _cuda(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def _ratio(got, ref, bound):
    return float((np.abs(got.double().cpu().numpy() - ref) / bound).max())


def _run(img, grids, g_out, want_img=True, want_grids=True, channels_last=False):
    """(out, g_img, g_grids) through autograd; img is used as given (any layout)"""
    from siu3r_amd.losses import apply_bilagrid

    x = img.detach().requires_grad_(want_img)
    A = grids.detach().requires_grad_(want_grids)
    out = apply_bilagrid(x, A, channels_last=channels_last)
    out.backward(g_out)
    return out.detach(), x.grad, A.grad


@pytest.mark.parametrize("name", list(D.CASES))
def test_cases_against_float64(name):
    (img, grids, g_out), ref, bound = _case(name)
    x, A, g = _cuda(img, grids, g_out)
    first = _run(x, A, g)
    again = _run(x, A, g)
    for key, a, b in zip(("out", "g_in", "g_grids"), first, again):
        assert torch.equal(a, b), f"{name}/{key}: two runs differ"
        r = _ratio(a, ref[key], bound[key])
        _worst[f"{name}/{key}"] = round(r, 4)
        print(f"\n{name}/{key}: worst |gpu - float64| / bound = {r:.4f}")
        assert r <= 1.0, (name, key, r)
    if name == "d_finer_than_pixels":  # vertices no pixel reaches: exact zeros
        empty = torch.from_numpy(ref["g_grids"] == 0).cuda()
        assert empty.any() and bool((first[2][empty] == 0).all())


def test_kinks_forward_only():
    from siu3r_amd.losses import apply_bilagrid

    img, grids = D.kink_case()
    x, A = _cuda(img, grids)
    out = apply_bilagrid(x, A)
    r = _ratio(out, D.explicit(img, grids)["out"], D.bounds(img, grids)["out"])
    _worst["kinks/out"] = round(r, 4)
    assert r <= 1.0 and torch.equal(out, apply_bilagrid(x, A))


def test_only_the_gradients_asked_for():
    """(j) g_in only, g_grids only and both give the bits of the run that computes both; a single image takes grids [12,L,Gh,Gw]"""
    from siu3r_amd.losses import apply_bilagrid

    (img, grids, g_out), _, _ = _case("b_uneven_345")
    x, A, g = _cuda(img, grids, g_out)
    out, g_img, g_grids = _run(x, A, g)
    o1, gi1, gg1 = _run(x, A, g, want_grids=False)
    o2, gi2, gg2 = _run(x, A, g, want_img=False)
    assert gg1 is None and gi2 is None
    assert torch.equal(o1, out) and torch.equal(o2, out) and torch.equal(gi1, g_img) and torch.equal(gg2, g_grids)
    assert torch.equal(apply_bilagrid(x, A), out)  # the path without autograd
    o3, gi3, gg3 = _run(x[0], A[0], g)
    assert o3.shape == out.shape and gi3.shape == x[0].shape and gg3.shape == A[0].shape
    assert torch.equal(o3, out) and torch.equal(gi3, g_img[0]) and torch.equal(gg3, g_grids[0])


def test_layouts_with_canaries():
    """(i) channels_last, a channel / row / column slice of a wider buffer whose base is not 16-byte aligned, through the C ABI with canary-filled
    parents: the same bits as the contiguous run, and no canary is touched"""
    from siu3r_amd import _lib
    from siu3r_amd.ops import _p, _stream

    (img, grids, g_out), ref, bound = _case("h_clamped")
    x, A, g = _cuda(img, grids, g_out)
    V, _, H, W = x.shape
    _, _, L, Gh, Gw = A.shape
    want = _run(x, A, g)
    got = _run(x.permute(0, 2, 3, 1).contiguous(), A, g, channels_last=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].permute(0, 3, 1, 2), want[1]) and torch.equal(got[2], want[2])
    lib = _lib.lib()
    for kind in ("planes_slice", "pixels_slice", "pixels_unaligned"):
        if kind == "planes_slice":  # [V,5,H+2,W+3], channels 1..3, rows 1.., columns 2..: strided, base 8 bytes off
            parent = torch.full((V, 5, H + 2, W + 3), float("nan"), device="cuda")
            sl = lambda t: t[:, 1:4, 1:H + 1, 2:W + 2]
        elif kind == "pixels_slice":  # [V,H,W,5] channels 1..3 seen as [V,3,H,W]
            parent = torch.full((V, H, W, 5), float("nan"), device="cuda")
            sl = lambda t: t[..., 1:4].permute(0, 3, 1, 2)
        else:  # dense pixels one float into a flat buffer: the 16-byte path must not be taken
            parent = torch.full((V * H * W * 3 + 8,), float("nan"), device="cuda")
            sl = lambda t: t[1:1 + V * H * W * 3].view(V, H, W, 3).permute(0, 3, 1, 2)
        sl(parent).copy_(x)
        view = sl(parent)
        st = (C.c_int64 * 4)(*view.stride())
        out = torch.full((V * 3 * H * W + 8,), CANARY, device="cuda")
        g_parent = torch.full_like(parent, CANARY)
        g_grids = torch.full((A.numel() + 8,), CANARY, device="cuda")
        for _ in range(2):
            _lib.check(lib.siu3r_bilagrid_apply(_p(view), st, _p(A), V, H, W, L, Gh, Gw, _p(out[4:]), _stream()))
            _lib.check(lib.siu3r_bilagrid_apply_bwd(_p(view), st, _p(A), _p(g), V, H, W, L, Gh, Gw, _p(sl(g_parent)), _p(g_grids[4:]), _stream()))
            assert torch.equal(out[4:-4].view(V, 3, H, W), want[0]), kind
            assert torch.equal(sl(g_parent), want[1]), kind
            assert torch.equal(g_grids[4:-4].view_as(A), want[2]), kind
        assert bool((out[:4] == CANARY).all() and (out[-4:] == CANARY).all() and (g_grids[:4] == CANARY).all() and (g_grids[-4:] == CANARY).all()), kind
        sl(g_parent).fill_(CANARY)
        assert bool((g_parent == CANARY).all()), f"{kind}: g_in wrote outside the view"
    _worst["h_clamped/layouts"] = round(_ratio(want[1], ref["g_in"], bound["g_in"]), 4)


def test_identity_grid_returns_the_input_bits():
    from siu3r_amd.cameras import identity_grids
    from siu3r_amd.losses import apply_bilagrid

    img = D.image(2, 37, 53, 8, seed=4, lo=-0.5, hi=1.5)
    img[0, :, 0, 0] = (-0.0, 0.0, 1e-30)
    (x,) = _cuda(img)
    for shape in ((16, 16, 8), (2, 2, 2), (3, 5, 16)):
        out = apply_bilagrid(x, identity_grids(2, shape, "cuda"))
        assert torch.equal(out.view(torch.int32), (x + 0.0).view(torch.int32)), shape  # (x + 0: a -0 comes back as +0)


def test_a_grid_constant_in_z_has_exactly_no_guidance_gradient():
    """a grid that is one matrix per view gives the bits of the affine transform's image gradient; a grid constant in z only gives the bits of
    the same planes at another L"""
    from siu3r_amd.losses import apply_bilagrid, apply_exposure

    (img, _, g_out), _, _ = _case("b_uneven_345")
    x, g = _cuda(img, g_out)
    M = (torch.eye(3, 4) + 0.2 * torch.randn(1, 3, 4, generator=torch.Generator().manual_seed(3))).cuda()
    A = M.reshape(1, 12, 1, 1, 1).expand(1, 12, 5, 3, 4).contiguous()
    xe = x.clone().requires_grad_(True)
    apply_exposure(xe, M).backward(g)
    _, g_img, _ = _run(x, A, g, want_grids=False)
    assert torch.equal(g_img, xe.grad)
    planes = torch.from_numpy(D.smooth_grids(1, 3, 4, 2, seed=8)[:, :, :1]).cuda()
    _, g5, _ = _run(x, planes.expand(1, 12, 5, 3, 4).contiguous(), g, want_grids=False)
    _, g2, _ = _run(x, planes.expand(1, 12, 2, 3, 4).contiguous(), g, want_grids=False)
    assert torch.equal(g5, g2)


def test_a_nan_pixel_poisons_only_itself():
    from siu3r_amd.losses import apply_bilagrid

    (img, grids, _), _, _ = _case("c_default")
    x, A = _cuda(img, grids)
    clean = apply_bilagrid(x, A)
    x[1, 1, 17, 33] = float("nan")
    out = apply_bilagrid(x, A)
    hit = torch.zeros_like(out, dtype=torch.bool)
    hit[1, :, 17, 33] = True
    assert bool(torch.isnan(out[hit]).all()) and torch.equal(out[~hit], clean[~hit])


def test_total_variation():
    from siu3r_amd import _lib
    from siu3r_amd.losses import bilagrid_tv
    from siu3r_amd.ops import _p, _stream

    for shape in ((2, 2, 2, 2), (2, 3, 4, 5), (3, 16, 16, 8)):
        grids = D.smooth_grids(*shape, seed=11)
        value, grad, _ = D.tv(grids)
        bv, bg = D.tv_bounds(grids)
        (A,) = _cuda(grids)
        A.requires_grad_(True)
        tv = bilagrid_tv(A)
        (3.0 * tv).backward()
        assert tv.dim() == 0 and abs(float(tv.detach()) - value) <= bv, (shape, float(tv.detach()), value)
        r = float((np.abs(A.grad.double().cpu().numpy() - 3.0 * grad) / (3.0 * bg + 3.0 * np.abs(grad) * D.U)).max())  # (the multiply by 3 rounds once more)
        _worst[f"tv{shape}/grad"] = round(r, 4)
        assert r <= 1.0, (shape, r)
        assert torch.equal(bilagrid_tv(A.detach()), tv.detach()) and torch.equal(bilagrid_tv(A[0].detach()).isfinite(), torch.tensor(True).cuda())
        # the C ABI accumulates scale x gradient into g_grids
        lib = _lib.lib()
        V, L, Gh, Gw = A.shape[0], A.shape[2], A.shape[3], A.shape[4]
        ws = torch.empty(int(lib.siu3r_bilagrid_tv_ws(V, L, Gh, Gw)) // 8, dtype=torch.float64, device="cuda")
        val = torch.empty(1, device="cuda")
        base = torch.from_numpy(D.smooth_grids(*shape, seed=12)).cuda()
        acc = [base.clone(), base.clone()]
        for a in acc:
            _lib.check(lib.siu3r_bilagrid_tv(_p(A.detach()), V, L, Gh, Gw, 0.5, _p(a), _p(ws), _p(val), _stream()))
        assert torch.equal(acc[0], acc[1]) and float(val) == float(tv.detach())
        want = base.double().cpu().numpy() + 0.5 * grad
        assert float((np.abs(acc[0].double().cpu().numpy() - want) / (0.5 * bg + np.abs(want) * D.U)).max()) <= 1.0


def test_refusals():
    from siu3r_amd.losses import apply_bilagrid, bilagrid_tv

    x = torch.rand(2, 3, 8, 9).cuda()
    A = torch.from_numpy(D.identity_grids(2, 3, 4, 5)).cuda()
    with pytest.raises(TypeError):
        apply_bilagrid(x.cpu().numpy(), A)
    with pytest.raises(RuntimeError):
        apply_bilagrid(x.cpu(), A.cpu())
    for bad_x, bad_A in ((x.double(), A), (x, A.double()), (x[:, :2], A), (x, A[:1]), (x, A[:, :11]), (x, A[:, :, :1]), (x, A[0]),
                         (x, torch.zeros(2, 12, 17, 4, 4).cuda()), (x[0], A)):
        with pytest.raises(ValueError):
            apply_bilagrid(bad_x, bad_A)
    with pytest.raises(ValueError):
        bilagrid_tv(A[:, :, :, :1])
    with pytest.raises(RuntimeError):
        bilagrid_tv(A.cpu())
