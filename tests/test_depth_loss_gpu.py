"""The fused depth loss (siu3r_amd/losses.py::depth_loss, csrc/depth_loss.hip) on the GPU against tests/dense_depth64.py in float64.

Tolerance of the accuracy tests: the float64 reference is evaluated on the SAME float32 inputs upcast; the composed float32 torch loss
(the same restatement in float32 with autograd, on the CPU) is evaluated on those inputs too, and the HIP result's error against float64
(relative for the loss and the per-view values, max-normalised for each gradient map) may be at most 2 x the composed float32 error, with a
floor of 1e-6 (cases where float32 torch happens to be exact).  The counts of valid pixels must be exact.  Where the reference is exactly
zero (no counted view, no valid pixel) the HIP result must be exactly zero."""
import math

import pytest
import torch

import dense_depth64 as D
from scenes import default_K, look_at_camera, random_scene

pytestmark = pytest.mark.gpu

MODES, SPACES = ("l1", "pearson"), ("depth", "inverse")


def _hip(Dm, O, T, Wt, mode, space, min_opacity=0.5):
    from siu3r_amd import losses

    d, o = Dm.cuda().requires_grad_(True), O.cuda().requires_grad_(True)
    loss, per_view, valid = losses.depth_loss(d, o, T.cuda(), None if Wt is None else Wt.cuda(), mode, space, min_opacity, return_terms=True)
    loss.backward()
    assert loss.dim() == 0 and loss.is_cuda and not per_view.requires_grad and valid.dtype == torch.int32
    return dict(loss=float(loss.detach()), per_view=per_view.cpu().double(), valid=valid.cpu().long(), g_depth=d.grad.cpu().double(),
                g_opacity=o.grad.cpu().double())


def _rel(got, ref):
    if ref == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return abs(got - ref) / abs(ref)


def _errors(res, ref, strict=True):
    """(loss, per-view, g_depth, g_opacity) errors of `res` against the float64 `ref`; strict: the NaN per-view entries must coincide"""
    nan_r, nan_g = torch.isnan(ref["per_view"]), torch.isnan(res["per_view"].double())
    if strict:
        assert torch.equal(nan_r, nan_g), (ref["per_view"], res["per_view"])
    both = ~nan_r & ~nan_g
    pv = max([_rel(float(g), float(r)) for g, r in zip(res["per_view"].double()[both], ref["per_view"][both])], default=0.0)
    out = [_rel(res["loss"], ref["loss"]), pv]
    for k in ("g_depth", "g_opacity"):
        gmax = float(ref[k].abs().max())
        diff = float((res[k].double() - ref[k]).abs().max())
        out.append(diff / gmax if gmax > 0 else (0.0 if diff == 0.0 else math.inf))
    return out


def _compare(tag, Dm, O, T, Wt, mode, space):
    ref = D.loss_and_grad(Dm, O, T, Wt, mode, space, dtype=torch.float64)
    cmp_ = D.loss_and_grad(Dm, O, T, Wt, mode, space, dtype=torch.float32, route="autograd")
    hip = _hip(Dm, O, T, Wt, mode, space)
    share = float(ref["valid"].sum()) / Dm.numel()
    e_cmp, e_hip = _errors(cmp_, ref, strict=False), _errors(hip, ref)
    names = ("loss", "per-view", "g_depth", "g_opacity")
    print(f"\n{tag} {mode} {space}: valid {share * 100:.0f} %, loss {ref['loss']:.6e}; " + "; ".join(f"{n} composed-f32 {c:.2e} hip {h:.2e}" for n, c, h in zip(names, e_cmp, e_hip)))
    assert torch.equal(hip["valid"], ref["valid"]), (hip["valid"], ref["valid"])
    assert bool(torch.isfinite(hip["g_depth"]).all()) and bool(torch.isfinite(hip["g_opacity"]).all()) and math.isfinite(hip["loss"])
    invalid = ~D.valid_mask(Dm, O, T, Wt, 0.5)
    assert not bool(hip["g_depth"][invalid].any()) and not bool(hip["g_opacity"][invalid].any())
    for n, c, h in zip(names, e_cmp, e_hip):
        assert h <= max(2.0 * c, 1e-6), f"{tag} {mode} {space} {n}: hip error {h:.3e} > max(2 x composed float32 error {c:.3e}, 1e-6)"
    return ref


# V, H, W, weights.  A workgroup owns 1,024 pixels of a view: 1 x 16 x 64 is exactly one, 1 x 5 x 205 one pixel more; 1 x 1080 x 1920 has
# 2,025 records for the 256 threads of the finalize kernel; 3 x 33 x 47 has planes whose base is not 16-byte aligned (the scalar path).
SHAPES = [(1, 1, 2, False), (1, 7, 5, False), (3, 33, 47, False), (6, 64, 80, False), (2, 128, 128, False), (1, 16, 64, False), (1, 5, 205, False),
          (1, 1080, 1920, False), (3, 33, 47, True), (6, 64, 80, True), (2, 128, 128, True)]


def _seed(V, H, W):
    return 5 if (V, H, W) == (1, 1, 2) else V * 1000 + H  # (1 x 1 x 2: a seed that leaves a valid pixel, asserted below)


@pytest.mark.parametrize("V,H,W,weights", SHAPES)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_value_and_gradient_against_float64(kind, V, H, W, weights):
    Dm, O, T, Wt = D.make_inputs(kind, V, H, W, seed=_seed(V, H, W), weights=weights)
    assert int(D.valid_mask(Dm, O, T, Wt, 0.5).sum()) >= 1
    for mode in MODES:
        for space in SPACES:
            _compare(f"{kind} {V}x{H}x{W}{' weighted' if weights else ''}", Dm, O, T, Wt, mode, space)


@pytest.mark.parametrize("mode", MODES)
def test_two_calls_give_identical_bits(mode):
    Dm, O, T, Wt = D.make_inputs("smooth", 6, 200, 150, seed=3, weights=True)
    a, b = _hip(Dm, O, T, Wt, mode, "depth"), _hip(Dm, O, T, Wt, mode, "depth")
    assert a["loss"] == b["loss"] and a["loss"] > 0
    assert torch.equal(a["per_view"], b["per_view"]) and torch.equal(a["valid"], b["valid"])
    assert torch.equal(a["g_depth"], b["g_depth"]) and torch.equal(a["g_opacity"], b["g_opacity"])


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_pixels_are_invalid_pixels(mode, space):
    Dm, O, T, Wt = D.make_inputs("noise", 3, 40, 50, seed=11, weights=True)
    g = torch.Generator().manual_seed(12)
    was_valid = D.valid_mask(Dm, O, T, Wt, 0.5)
    where = torch.randperm(Dm.numel(), generator=g)[:48]
    poison = [float("nan"), float("inf"), -float("inf")]
    bad = [t.clone() for t in (Dm, O, T, Wt)]
    for i, idx in enumerate(where.tolist()):
        bad[i % 4].view(-1)[idx] = poison[(i // 4) % 3]
    masked = Wt.clone()
    masked.view(-1)[where] = 0.0
    assert int(was_valid.view(-1)[where].sum()) >= 10, "the poison must hit pixels that were valid"
    a, b = _hip(*bad, mode, space), _hip(Dm, O, T, masked, mode, space)
    assert a["loss"] == b["loss"] and math.isfinite(a["loss"]) and a["loss"] > 0
    assert torch.equal(a["per_view"], b["per_view"]) and torch.equal(a["valid"], b["valid"]) and bool(torch.isfinite(a["per_view"]).all())
    for k in ("g_depth", "g_opacity"):
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all())
        assert not bool(a[k].view(-1)[where].any())
        assert float(a[k].abs().max()) > 0


def test_skipped_views():
    Dm, O, T, _ = D.make_inputs("noise", 6, 24, 30, seed=21)
    O[0] = 0.25                              # view 0: nothing valid
    T[2] = 0.0
    Dm[2, 5, 7], O[2, 5, 7], T[2, 5, 7] = 2.0, 1.0, 3.0  # view 2: a single valid pixel
    Dm[4], O[4] = 2.5, 1.0                   # view 4: constant x (exact in every precision)
    for space in SPACES:
        ref = _compare("skipped views", Dm, O, T, None, "pearson", space)
        assert ref["count"] == 3.0 and torch.isnan(ref["per_view"]).tolist() == [True, False, True, False, True, False]
        assert ref["valid"][0] == 0 and ref["valid"][2] == 1
        hip = _hip(Dm, O, T, None, "pearson", space)
        assert not bool(hip["g_depth"][[0, 2, 4]].any()) and not bool(hip["g_opacity"][[0, 2, 4]].any())
        ref = _compare("skipped views", Dm, O, T, None, "l1", space)
        assert torch.isnan(ref["per_view"]).tolist() == [True] + [False] * 5
        assert ref["count"] == float(ref["valid"].sum())
    from siu3r_amd import losses

    loss, per_view, valid = losses.depth_loss(Dm.cuda(), (O * 0.3).cuda(), T.cuda(), mode="pearson", return_terms=True)
    assert float(loss) == 0.0 and bool(torch.isnan(per_view).all()) and not bool(valid.any())
    d = Dm.cuda().requires_grad_(True)
    loss = losses.depth_loss(d, (O * 0.3).cuda(), T.cuda(), mode="l1")
    loss.backward()
    assert float(loss) == 0.0 and not bool(d.grad.any())


def test_gradients_through_a_real_render():
    from siu3r_amd import losses
    from siu3r_amd.cuda_splatting import render_cuda

    V, H, W, G = 3, 128, 128, 20000
    means, cov, opac, sh = (x.cuda() for x in random_scene(G, seed=0, n_sh=4))
    leaves = [x.requires_grad_(True) for x in (means, cov, sh, opac)]
    c2w = torch.stack([look_at_camera(seed=i) for i in range(V)]).cuda()
    K = default_K()[None].repeat(V, 1, 1).cuda()
    e = lambda x: x[None].expand(V, *x.shape)
    _, depth, aux = render_cuda(c2w, K, torch.full((V,), 0.1), torch.full((V,), 100.0), (H, W), torch.zeros(V, 3), e(means), e(cov), e(sh), e(opac),
                                return_aux=True)
    opacity = torch.cat([a["opacity"] for a in aux])
    radii = torch.cat([a["radii"] for a in aux])
    assert depth.requires_grad and opacity.requires_grad and depth.shape == opacity.shape == (V, H, W)
    target = (1.1 * depth / opacity.clamp_min(1e-6)).detach()
    loss, per_view, valid = losses.depth_loss(depth, opacity, target, mode="l1", return_terms=True)
    loss.backward()
    print(f"\nrender: depth l1 {float(loss):.6f}, per view {per_view.tolist()}, valid pixels {valid.tolist()}")
    assert int(valid.sum()) > 1000 and float(loss) > 0
    for x in (means, opac):
        assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    unseen = ~(radii > 0).any(-1).any(0)
    assert int(unseen.sum()) > 0
    assert not bool(means.grad[unseen].any()) and not bool(opac.grad[unseen].any())


def test_autograd_plumbing_and_layouts():
    from siu3r_amd import losses

    Dm, O, T, Wt = (t.cuda() for t in D.make_inputs("noise", 2, 20, 30, seed=5, weights=True))
    for mode in MODES:
        a_d, a_o = Dm.clone().requires_grad_(True), O.clone().requires_grad_(True)
        losses.depth_loss(a_d, a_o, T, Wt, mode).backward()
        b_d, b_o = Dm.clone().requires_grad_(True), O.clone().requires_grad_(True)
        (losses.depth_loss(b_d, b_o, T, Wt, mode) * 4.0).backward()  # (a power of two: the two multiplies commute exactly)
        assert torch.equal(b_d.grad, a_d.grad * 4.0) and torch.equal(b_o.grad, a_o.grad * 4.0)
        # without requires_grad: the plain forward, the same bits; target and weight receive nothing
        plain = losses.depth_loss(Dm, O, T, Wt, mode)
        assert plain.grad_fn is None and plain.dim() == 0 and plain.is_cuda
        assert torch.equal(plain, losses.depth_loss(Dm.clone().requires_grad_(True), O, T, Wt, mode).detach())
        with torch.no_grad():
            assert losses.depth_loss(Dm.clone().requires_grad_(True), O, T, Wt, mode).grad_fn is None
        tt, ww = T.clone().requires_grad_(True), Wt.clone().requires_grad_(True)
        assert losses.depth_loss(Dm, O, tt, ww, mode).grad_fn is None
        c_d = Dm.clone().requires_grad_(True)
        losses.depth_loss(c_d, O, tt, ww, mode).backward()  # only depth wants a gradient
        assert tt.grad is None and ww.grad is None and torch.equal(c_d.grad, a_d.grad)
        # non-contiguous target and weight, and a single [H,W] image
        big_t, big_w = torch.zeros(2, 20, 37).cuda(), torch.zeros(2, 20, 37).cuda()
        big_t[:, :, 3:33], big_w[:, :, 3:33] = T, Wt
        assert torch.equal(losses.depth_loss(Dm, O, big_t[:, :, 3:33], big_w[:, :, 3:33], mode), plain)
        one_d = Dm[1].clone().requires_grad_(True)
        l, per_view, valid = losses.depth_loss(one_d, O[1], T[1], Wt[1], mode, return_terms=True)
        l.backward()
        assert one_d.grad.shape == (20, 30) and per_view.shape == (1,) and valid.shape == (1,)
        if mode == "l1":
            assert abs(float(l) - float(per_view[0])) <= 1e-6 * float(l)


def test_error_paths():
    from siu3r_amd import losses

    x = torch.rand(2, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_loss(x, x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_loss(x.cuda(), x.cuda(), x)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_loss(x.cuda(), x.cuda(), x.cuda(), weight=x)
    g = x.cuda()
    with pytest.raises(ValueError, match="float32"):
        losses.depth_loss(g.double(), g.double(), g.double())
    with pytest.raises(ValueError, match="float32"):
        losses.depth_loss(g, g, g.bfloat16())
    with pytest.raises(ValueError, match="shape"):
        losses.depth_loss(g, g[:, :15], g)
    with pytest.raises(ValueError, match="shape"):
        losses.depth_loss(g, g, g, weight=g[:1])
    with pytest.raises(ValueError, match="mode"):
        losses.depth_loss(g, g, g, mode="l2")
    with pytest.raises(ValueError, match="space"):
        losses.depth_loss(g, g, g, space="disparity")
    with pytest.raises(ValueError, match="min_opacity"):
        losses.depth_loss(g, g, g, min_opacity=-0.1)
    with pytest.raises(ValueError):
        losses.depth_loss(torch.rand(2, 1, 16, 16).cuda(), torch.rand(2, 1, 16, 16).cuda(), torch.rand(2, 1, 16, 16).cuda())


def test_loss_and_backward_do_not_synchronise():
    from siu3r_amd import losses

    Dm, O, T, Wt = (t.cuda() for t in D.make_inputs("smooth", 3, 64, 64, seed=4, weights=True))
    for mode in MODES:
        warm = Dm.clone().requires_grad_(True)
        losses.depth_loss(warm, O, T, Wt, mode).backward()
        x = Dm.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = losses.depth_loss(x, O, T, Wt, mode)
            loss.backward()
            plain = losses.depth_loss(Dm, O, T, Wt, mode, return_terms=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(x.grad, warm.grad) and torch.equal(plain[0], loss.detach()) and plain[1].shape == (3,)
