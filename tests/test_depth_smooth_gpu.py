"""The fused depth smoothness (siu3r_amd/losses.py::depth_smoothness, csrc/depth_smooth.hip) on the GPU against tests/dense_smooth64.py in
float64.

Tolerance of the accuracy tests: the float64 reference is evaluated on the SAME float32 inputs upcast; the composed float32 torch loss (the
same restatement in float32 with autograd, on the CPU) is evaluated on those inputs too, and the HIP result's error against float64
(relative for the loss, its two parts and the per-view values, max-normalised for each gradient map) may be at most 2 x the composed
float32 error, with a floor of 1e-6.  The counts of active terms must be exact.  Where the reference is exactly zero the HIP result must be
exactly zero.  A gradient element one of whose terms has |t| < 1e-9 max|x| without being exactly 0 would be left out of the comparison (at
most 0.1 % of a map); the inputs are chosen so that there is none, which the tests assert."""
import math

import pytest
import torch

import dense_smooth64 as S

pytestmark = pytest.mark.gpu

ORDERS, SPACES = (1, 2), ("render", "expected")


def _hip(D, O, seg, order, space, min_opacity=0.5):
    from siu3r_amd import losses

    d = D.cuda().requires_grad_(True)
    o = None if O is None else O.cuda().requires_grad_(True)
    loss, per_view, active = losses.depth_smoothness(d, o, None if seg is None else seg.cuda(), order, space, min_opacity, return_terms=True)
    loss.backward()
    assert loss.dim() == 0 and loss.is_cuda and not per_view.requires_grad and active.dtype == torch.int32 and active.shape == (D.shape[0], 2)
    g_o = torch.zeros_like(D) if o is None or o.grad is None else o.grad.cpu()
    return dict(loss=float(loss.detach()), per_view=per_view.cpu().double(), active=active.cpu().long(), g_depth=d.grad.cpu().double(), g_opacity=g_o.double())


def _values(D, O, seg, order, space):
    """the value-only call (no gradient maps): (out [4], per_view, active) on the CPU"""
    from siu3r_amd import losses

    out, per_view, active, gd, go = losses._launch_smooth(D.cuda(), None if O is None else O.cuda(), None if seg is None else seg.cuda(), order, space, 0.5, False)
    assert gd is None and go is None
    return out.cpu().double(), per_view.cpu().double(), active.cpu().long()


def _rel(got, ref):
    if ref == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return abs(got - ref) / abs(ref)


def _errors(res, ref, keep):
    """(loss, per-view, g_depth, g_opacity) errors of `res` against the float64 `ref`; keep: the gradient elements that are compared"""
    pv = max((_rel(float(g), float(r)) for g, r in zip(res["per_view"].double(), ref["per_view"])), default=0.0)
    out = [_rel(res["loss"], ref["loss"]), pv]
    for k in ("g_depth", "g_opacity"):
        gmax = float(ref[k].abs().max())
        diff = float((res[k].double() - ref[k])[keep].abs().max()) if bool(keep.any()) else 0.0
        out.append(diff / gmax if gmax > 0 else (0.0 if diff == 0.0 else math.inf))
    return out


def _compare(tag, D, O, seg, order, space):
    ref = S.loss_and_grad(D, O, seg, order, space, dtype=torch.float64)
    cmp_ = S.loss_and_grad(D, O, seg, order, space, dtype=torch.float32, route="autograd")
    hip = _hip(D, O, seg, order, space)
    out, per_view, active = _values(D, O, seg, order, space)
    ex = S.excluded(D, O, seg, order, space)
    assert int(ex.sum()) == 0 and float(ex.float().mean()) <= 1e-3, f"{tag}: {int(ex.sum())} gradient elements hang on a term within 1e-9 max|x| of zero"
    keep = ~ex
    e_cmp, e_hip = _errors(cmp_, ref, keep), _errors(hip, ref, keep)
    e_parts = [_rel(float(out[1]), ref["parts"][0]), _rel(float(out[2]), ref["parts"][1])]
    c_parts = [_rel(cmp_["parts"][0], ref["parts"][0]), _rel(cmp_["parts"][1], ref["parts"][1])]
    names = ("loss", "per-view", "g_depth", "g_opacity", "x part", "y part")
    share = float(ref["active"].sum()) / max(2 * D.numel(), 1)
    print(f"\n[parity] {tag} order {order} {space}{'' if seg is None else ' segments'}: active {share * 100:.0f} %, loss {ref['loss']:.6e}; "
          + "; ".join(f"{n} composed-f32 {c:.2e} hip {h:.2e}" for n, c, h in zip(names, e_cmp + c_parts, e_hip + e_parts)))
    assert torch.equal(hip["active"], ref["active"]) and torch.equal(active, ref["active"]), (hip["active"], ref["active"])
    assert float(out[0]) == hip["loss"] and float(out[3]) == 0.0 and torch.equal(per_view, hip["per_view"])  # the value-only kernels: the same bits
    assert bool(torch.isfinite(hip["g_depth"]).all()) and bool(torch.isfinite(hip["g_opacity"]).all()) and math.isfinite(hip["loss"])
    Od = torch.ones_like(D) if O is None else O
    dead = ~S.usable_mask(D, Od, space, 0.5) | ((seg < 0) if seg is not None else torch.zeros_like(D, dtype=torch.bool))
    assert not bool(hip["g_depth"][dead].any()) and not bool(hip["g_opacity"][dead].any())
    for n, c, h in zip(names, e_cmp + c_parts, e_hip + e_parts):
        assert h <= max(2.0 * c, 1e-6), f"{tag} order {order} {space} {n}: hip error {h:.3e} > max(2 x composed float32 error {c:.3e}, 1e-6)"
    return ref


# 1x1x1, 1x1x2, 1x2x1: no term / one term.  1x2x2: no position of order 2 on either axis.  1x3x3: one order-2 term per row / column.  A
# workgroup owns a 64 x 16 tile: 1x16x64 is exactly one, 1x17x65 one pixel more on both axes (one-pixel tiles whose halo is a whole neighbour),
# 3x37x67 has planes whose base is not 16-byte aligned for v > 0 and a W that is no multiple of 4 (the scalar path), 2x48x200 is four tiles
# across and three down on the 16-byte path.
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (1, 3, 3), (1, 16, 64), (1, 17, 65), (3, 37, 67), (2, 48, 200)]


@pytest.mark.parametrize("V,H,W", SHAPES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_value_and_gradient_against_float64(kind, V, H, W):
    for segments in (True, False):
        D, O, seg = S.make_inputs(kind, V, H, W, seed=V * 1000 + H, segments=segments)
        for order in ORDERS:
            for space in SPACES:
                ref = _compare(f"{kind} {V}x{H}x{W}", D, O, seg, order, space)
                if not segments and H * W < 64:  # every pixel usable, one segment: every position is an active term
                    assert ref["active"].tolist() == [[H * max(W - order, 0), max(H - order, 0) * W]]
                if H * W >= 64:
                    assert int(ref["active"].sum()) > 0 and ref["loss"] > 0
    if (V, H, W) == (2, 48, 200):  # the render space without an opacity map at all
        D, _, seg = S.make_inputs(kind, V, H, W, seed=1, segments=True)
        _compare(f"{kind} {V}x{H}x{W} no opacity", D, None, seg, 2, "render")


def test_exact_zero_terms_take_no_gradient():
    """constant regions: their terms are active and exactly zero, so sign(t) = 0 in every precision"""
    D, O, seg = S.make_inputs("smooth", 2, 48, 200, seed=2, segments=False)
    for order in ORDERS:
        for space in SPACES:
            (tx, ty), _, _ = S.term_values(D.double(), O.double(), seg, order, space)
            assert int((tx[1] & (tx[0] == 0)).sum()) > 300 and int((ty[1] & (ty[0] == 0)).sum()) > 300
            hip = _hip(D, O, seg, order, space)
            inner = hip["g_depth"][:, 2:4, 2:7]  # every term of these pixels lies inside the constant 6 x 9 block
            assert not bool(inner.any()) and not bool(hip["g_opacity"][:, 2:4, 2:7].any()) and bool(hip["g_depth"][:, 8:, :].any())


def test_two_calls_give_identical_bits():
    D, O, seg = S.make_inputs("smooth", 4, 100, 150, seed=3, segments=True)
    for order in ORDERS:
        for space in SPACES:
            a, b = _hip(D, O, seg, order, space), _hip(D, O, seg, order, space)
            assert a["loss"] == b["loss"] and a["loss"] > 0
            for k in ("per_view", "active", "g_depth", "g_opacity"):
                assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("order", ORDERS)
def test_poisoned_pixels_are_void_pixels(order, space):
    D, O, seg = S.make_inputs("noise", 3, 40, 70, seed=11, segments=True)
    g = torch.Generator().manual_seed(12)
    live = S.usable_mask(D, O, space, 0.5) & (seg >= 0)
    where = torch.randperm(D.numel(), generator=g)[:48]
    assert int(live.view(-1)[where].sum()) >= 10, "the poison must hit pixels that were live"
    poison = [float("nan"), float("inf"), -float("inf")]
    bad_d, bad_o = D.clone(), O.clone()
    for i, idx in enumerate(where.tolist()):
        (bad_d if space == "render" or i % 2 == 0 else bad_o).view(-1)[idx] = poison[(i // 2) % 3]  # (the render space does not read O)
    void = seg.clone()
    void.view(-1)[where] = -1
    a, b = _hip(bad_d, bad_o, seg, order, space), _hip(D, O, void, order, space)
    assert a["loss"] == b["loss"] and math.isfinite(a["loss"]) and a["loss"] > 0
    assert torch.equal(a["per_view"], b["per_view"]) and torch.equal(a["active"], b["active"]) and bool(torch.isfinite(a["per_view"]).all())
    for k in ("g_depth", "g_opacity"):
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all())
        assert not bool(a[k].view(-1)[where].any())
    assert float(a["g_depth"].abs().max()) > 0


def test_an_all_void_view_reports_nothing():
    D, O, seg = S.make_inputs("noise", 3, 24, 70, seed=21, segments=True)
    seg[1] = -1
    for order in ORDERS:
        for space in SPACES:
            ref = _compare("all-void view", D, O, seg, order, space)
            hip = _hip(D, O, seg, order, space)
            assert hip["active"][1].tolist() == [0, 0] and float(hip["per_view"][1]) == 0.0 and int(ref["active"][[0, 2]].min()) > 0
            assert not bool(hip["g_depth"][1].any()) and not bool(hip["g_opacity"][1].any())
    from siu3r_amd import losses

    d = D.cuda().requires_grad_(True)
    loss, per_view, active = losses.depth_smoothness(d, O.cuda(), torch.full(D.shape, -1.0).cuda(), return_terms=True)  # the float map of an empty panoptic result
    loss.backward()
    assert float(loss.detach()) == 0.0 and not bool(per_view.any()) and not bool(active.any()) and not bool(d.grad.any())


def test_gradients_through_a_real_render():
    from refine_scenes import FAR, H, NEAR, W, _cams, _truth
    from siu3r_amd import losses
    from siu3r_amd.cuda_splatting import render_cuda
    from siu3r_amd.refine import covariances_from

    V = 2
    t = _truth()
    means, opac = t["means"].clone().requires_grad_(True), t["opacities"].clone().requires_grad_(True)
    cov = covariances_from(t["rotations"], t["scales"])
    c2w, K = _cams([0, 1])
    e = lambda x: x[None].expand(V, *x.shape)
    _, depth, aux = render_cuda(c2w, K, torch.full((V,), NEAR), torch.full((V,), FAR), (H, W), torch.zeros(V, 3), e(means), e(cov), e(t["harmonics"]), e(opac),
                                return_aux=True)
    opacity = torch.cat([a["opacity"] for a in aux])
    radii = torch.cat([a["radii"] for a in aux])
    assert depth.requires_grad and opacity.requires_grad and depth.shape == opacity.shape == (V, H, W)
    seg = S.block_segments(V, H, W).cuda()
    loss, per_view, active = losses.depth_smoothness(depth, opacity, seg, order=2, space="expected", return_terms=True)
    loss.backward()
    print(f"\nrender: second-order smoothness {float(loss):.6f}, per view {per_view.tolist()}, active terms {active.tolist()}")
    assert int(active.sum()) > 1000 and float(loss) > 0
    for x in (means, opac):
        assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    unseen = ~(radii > 0).any(-1).any(0)
    assert int(unseen.sum()) > 0
    assert not bool(means.grad[unseen].any()) and not bool(opac.grad[unseen].any())


def test_autograd_plumbing_and_layouts():
    from siu3r_amd import losses

    D, O, seg = S.make_inputs("noise", 2, 20, 30, seed=5, segments=True)
    D, O, seg = D.cuda(), O.cuda(), seg.cuda()
    for order in ORDERS:
        for space in SPACES:
            kw = dict(order=order, space=space)
            a_d, a_o = D.clone().requires_grad_(True), O.clone().requires_grad_(True)
            losses.depth_smoothness(a_d, a_o, seg, **kw).backward()
            b_d, b_o = D.clone().requires_grad_(True), O.clone().requires_grad_(True)
            (losses.depth_smoothness(b_d, b_o, seg, **kw) * 4.0).backward()  # (a power of two: the multiply is exact)
            assert torch.equal(b_d.grad, a_d.grad * 4.0) and torch.equal(b_o.grad, a_o.grad * 4.0)
            assert bool(a_o.grad.any()) == (space == "expected")
            # only the needed gradient: an opacity that does not require grad gets none, and its map is not kept for the backward
            c_d = D.clone().requires_grad_(True)
            loss = losses.depth_smoothness(c_d, O, seg, **kw)
            assert loss.grad_fn.saved_tensors[1] is None
            loss.backward()
            assert torch.equal(c_d.grad, a_d.grad) and O.grad is None
            if space == "expected":
                c_o = O.clone().requires_grad_(True)
                losses.depth_smoothness(D, c_o, seg, **kw).backward()
                assert torch.equal(c_o.grad, a_o.grad) and D.grad is None
            # without requires_grad: the plain forward, the same bits
            plain = losses.depth_smoothness(D, O, seg, **kw)
            assert plain.grad_fn is None and plain.dim() == 0 and plain.is_cuda and torch.equal(plain, loss.detach())
            with torch.no_grad():
                assert losses.depth_smoothness(D.clone().requires_grad_(True), O, seg, **kw).grad_fn is None
            # ids of another integer dtype, a non-contiguous map, and a single [H,W] image
            assert torch.equal(losses.depth_smoothness(D, O, seg.long(), **kw), plain)
            assert torch.equal(losses.depth_smoothness(D, O, seg.to(torch.int16), **kw), plain)
            big = torch.zeros(2, 20, 37, dtype=torch.int32).cuda()
            big[:, :, 3:33] = seg
            assert torch.equal(losses.depth_smoothness(D, O, big[:, :, 3:33], **kw), plain)
            one_d = D[1].clone().requires_grad_(True)
            l, per_view, active = losses.depth_smoothness(one_d, O[1], seg[1], return_terms=True, **kw)
            l.backward()
            assert one_d.grad.shape == (20, 30) and per_view.shape == (1,) and active.shape == (1, 2)
            assert abs(float(l) - float(per_view[0])) <= 1e-6 * float(l)


def test_validation_raises_before_any_launch(monkeypatch):
    from siu3r_amd import losses

    def boom(*a, **k):
        raise AssertionError("a launch was reached")

    monkeypatch.setattr(losses, "_launch_smooth", boom)
    x = torch.rand(2, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_smoothness(x)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_smoothness(x.cuda(), x)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.depth_smoothness(x.cuda(), x.cuda(), torch.zeros(2, 16, 16, dtype=torch.int32))
    g = x.cuda()
    ids = torch.zeros(2, 16, 16, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="float32"):
        losses.depth_smoothness(g.double())
    with pytest.raises(ValueError, match="float32"):
        losses.depth_smoothness(g, g.bfloat16(), space="expected")
    with pytest.raises(ValueError, match="integer"):
        losses.depth_smoothness(g, segments=ids.bool())
    with pytest.raises(ValueError, match="shape"):
        losses.depth_smoothness(g, g[:, :15])
    with pytest.raises(ValueError, match="shape"):
        losses.depth_smoothness(g, segments=ids[:1])
    with pytest.raises(ValueError, match="order"):
        losses.depth_smoothness(g, order=3)
    with pytest.raises(ValueError, match="order"):
        losses.depth_smoothness(g, order=True)
    with pytest.raises(ValueError, match="space"):
        losses.depth_smoothness(g, g, space="inverse")
    with pytest.raises(ValueError, match="min_opacity"):
        losses.depth_smoothness(g, g, min_opacity=-0.1)
    with pytest.raises(ValueError, match="min_opacity"):
        losses.depth_smoothness(g, g, min_opacity=float("inf"))
    with pytest.raises(ValueError, match="opacity"):
        losses.depth_smoothness(g, space="expected")
    with pytest.raises(TypeError, match="tensor"):
        losses.depth_smoothness(g, segments=[[0]])
    with pytest.raises(ValueError):
        losses.depth_smoothness(torch.rand(2, 1, 16, 16).cuda())
    with pytest.raises(AssertionError, match="launch"):
        losses.depth_smoothness(g)


def test_loss_and_backward_do_not_synchronise():
    from siu3r_amd import losses

    D, O, seg = S.make_inputs("smooth", 3, 64, 64, seed=4, segments=True)
    D, O, seg = D.cuda(), O.cuda(), seg.cuda().long()
    for order in ORDERS:
        warm = D.clone().requires_grad_(True)
        losses.depth_smoothness(warm, O, seg, order, "expected").backward()
        x = D.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = losses.depth_smoothness(x, O, seg, order, "expected")
            loss.backward()
            plain = losses.depth_smoothness(D, O, seg, order, "expected", return_terms=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(x.grad, warm.grad) and torch.equal(plain[0], loss.detach()) and plain[1].shape == (3,) and plain[2].shape == (3, 2)
