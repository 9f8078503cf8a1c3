"""losses.apply_exposure (csrc/camera.hip) on the GPU against tests/dense_camera64.py in float64.

Tolerance, the rule of tests/test_photo_loss_gpu.py: the float64 reference is evaluated on the SAME float32 inputs upcast; the composed
float32 torch expression is evaluated on the CPU for the same inputs, and the HIP result's max-normalised error against float64 (value and
each gradient) may be at most 2 x the composed float32 error, with a floor of 1e-6."""
import pytest
import torch

import dense_camera64 as D

pytestmark = pytest.mark.gpu

WG = 2048  # pixels of one view that a workgroup owns


def _store(x, layout):
    """the [V,3,H,W] values stored on the GPU in `layout` -> (tensor to hand to apply_exposure, channels_last)"""
    V, C, H, W = x.shape
    if layout == "nchw":
        return x.cuda().contiguous(), False
    if layout == "nhwc":
        return x.permute(0, 2, 3, 1).contiguous().cuda(), True
    if layout == "sliced":  # a window of a larger [V,C,H+7,W+9] buffer
        big = torch.full((V, C, H + 7, W + 9), 7.0).cuda()
        big[:, :, 3:3 + H, 4:4 + W] = x.cuda()
        return big[:, :, 3:3 + H, 4:4 + W], False
    if layout == "nhwc_sliced":  # the first C channels of a [V,H,W,C+1] buffer
        big = torch.full((V, H, W, C + 1), 7.0).cuda()
        big[..., :C] = x.permute(0, 2, 3, 1).cuda()
        return big[..., :C], True
    raise ValueError(layout)


def _inputs(V, H, W, seed, m_kind="near_identity"):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(V, 3, H, W, generator=g)
    g_out = torch.randn(V, 3, H, W, generator=g)
    M = torch.eye(3, 4).repeat(V, 1, 1) + 0.1 * torch.randn(V, 3, 4, generator=g)
    if m_kind == "zero_row":
        M[:, 1] = 0.0
    return img, M, g_out


SHAPES = [(1, 1, 1), (3, 7, 5), (6, 33, 47), (2, 32, 64), (2, 3, 683), (6, 64, 80), (6, 512, 512)]
assert 32 * 64 == WG and 3 * 683 == WG + 1
LAYOUTS = ("nchw", "nhwc", "sliced", "nhwc_sliced")
CASES = [(s, l, "near_identity") for s in SHAPES[:-1] for l in LAYOUTS] + [(SHAPES[-1], "nchw", "near_identity"), (SHAPES[-1], "nhwc", "near_identity")]
CASES += [((6, 33, 47), l, "zero_row") for l in LAYOUTS]
_REF = {}


def _reference(shape, m_kind):
    """inputs, the float64 reference and the composed float32 result of one (shape, M kind), computed once"""
    key = (shape, m_kind)
    if key not in _REF:
        img, M, g_out = _inputs(*shape, seed=shape[0] * 1000 + shape[1] + shape[2], m_kind=m_kind)
        _REF[key] = (img, M, g_out, D.exposure_and_grads(img, M, g_out, torch.float64), D.exposure_and_grads(img, M, g_out, torch.float32))
    return _REF[key]


@pytest.mark.parametrize("shape,layout,m_kind", CASES)
def test_value_and_gradients_against_float64(shape, layout, m_kind):
    from siu3r_amd import losses

    img, M, g_out, ref, cmp32 = _reference(shape, m_kind)
    x, cl = _store(img, layout)
    x.requires_grad_(True)
    m = M.cuda().requires_grad_(True)
    out = losses.apply_exposure(x, m, channels_last=cl)
    assert out.shape == img.shape and out.is_contiguous()
    out.backward(g_out.cuda())
    assert x.grad.shape == x.shape and m.grad.shape == m.shape
    got = (out.detach().cpu().double(), (x.grad.permute(0, 3, 1, 2) if cl else x.grad).cpu().double(), m.grad.cpu().double())
    rows = []
    for name, r, c, h in zip(("value", "g_in", "g_M"), ref, cmp32, got):
        scale = float(r.abs().max())
        rows.append((name, float((c.double() - r).abs().max()) / scale, float((h - r).abs().max()) / scale))
    print(f"\n{shape} {layout} {m_kind}: " + "; ".join(f"{n} composed-f32 {c:.2e} hip {h:.2e}" for n, c, h in rows))
    for h in got:
        assert torch.isfinite(h).all()
    for n, c, h in rows:
        assert h <= max(2.0 * c, 1e-6), f"{n}: hip error {h:.3e} > max(2 x composed float32 error {c:.3e}, 1e-6)"
    if m_kind == "zero_row":
        assert torch.equal(out[:, 1], torch.zeros_like(out[:, 1]))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_returns_the_bits_of_the_input(layout):
    from siu3r_amd import losses

    img, _, _ = _inputs(3, 45, 70, seed=5)
    x, cl = _store(img, layout)
    out = losses.apply_exposure(x, torch.eye(3, 4).repeat(3, 1, 1).cuda(), channels_last=cl)
    assert torch.equal(out, img.cuda())


@pytest.mark.parametrize("layout", ["nchw", "nhwc_sliced"])
def test_two_calls_give_identical_bits(layout):
    from siu3r_amd import losses

    img, M, g_out = _inputs(6, 200, 150, seed=3)
    x, cl = _store(img, layout)
    res = []
    for _ in range(2):
        a, m = x.detach().requires_grad_(True), M.cuda().requires_grad_(True)
        out = losses.apply_exposure(a, m, channels_last=cl)
        out.backward(g_out.cuda())
        res.append((out.detach().clone(), a.grad.clone(), m.grad.clone()))
    for p, q in zip(*res):
        assert torch.equal(p, q)


def test_only_the_needed_gradients_are_computed(monkeypatch):
    from siu3r_amd import _lib, losses

    img, M, g_out = _inputs(2, 40, 50, seed=9)
    x, m, g = img.cuda(), M.cuda(), g_out.cuda()
    both_x, both_m = x.clone().requires_grad_(True), m.clone().requires_grad_(True)
    losses.apply_exposure(both_x, both_m).backward(g)
    seen = []
    real = _lib.lib().siu3r_exposure_apply_bwd

    class Spy:
        def __getattr__(self, name):
            if name == "siu3r_exposure_apply_bwd":
                return lambda *a: (seen.append((a[7] is not None, a[8] is not None, a[9] is not None)), real(*a))[1]
            return getattr(_lib._lib, name)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    only_m = m.clone().requires_grad_(True)
    losses.apply_exposure(x, only_m).backward(g)
    only_x = x.clone().requires_grad_(True)
    losses.apply_exposure(only_x, m).backward(g)
    assert seen == [(False, True, True), (True, False, False)]  # (g_in, g_M, workspace) handed to the kernel
    assert torch.equal(only_m.grad, both_m.grad) and torch.equal(only_x.grad, both_x.grad)
    # neither: the plain forward, no graph, the same bits with and without grad mode
    plain = losses.apply_exposure(x, m)
    assert plain.grad_fn is None
    with torch.no_grad():
        quiet = losses.apply_exposure(x.clone().requires_grad_(True), m)
    assert quiet.grad_fn is None and torch.equal(quiet, plain)
    assert torch.equal(losses.apply_exposure(x.clone().requires_grad_(True), m).detach(), plain)
    # a scaled upstream gradient, and a single image without V
    c = m.clone().requires_grad_(True)
    (losses.apply_exposure(x, c) * 3.0).backward(g)
    assert torch.allclose(c.grad, both_m.grad * 3.0, rtol=1e-5, atol=1e-4)  # (3 g is rounded per pixel before the sums)
    one, m1 = x[0].clone().requires_grad_(True), m[0].clone().requires_grad_(True)
    o = losses.apply_exposure(one, m1)
    o.backward(g[:1])
    assert o.shape == (1, 3, 40, 50) and one.grad.shape == one.shape and m1.grad.shape == (3, 4)
    assert torch.equal(o[0], plain[0]) and torch.equal(one.grad, both_x.grad[0]) and torch.equal(m1.grad, both_m.grad[0])


def test_the_render_layouts_are_consumed_without_a_copy(monkeypatch):
    """[V,3,H,W] and [V,H,W,3]: the kernel receives the tensor's own storage and strides"""
    from siu3r_amd import losses

    seen = []
    real = losses._launch_exposure
    monkeypatch.setattr(losses, "_launch_exposure", lambda i4, M3: (seen.append((i4.data_ptr(), tuple(i4.shape), tuple(i4.stride()))), real(i4, M3))[1])
    img, M, _ = _inputs(2, 16, 24, seed=1)
    a = img.cuda()
    losses.apply_exposure(a, M.cuda())
    b = img.permute(0, 2, 3, 1).contiguous().cuda()
    losses.apply_exposure(b, M.cuda(), channels_last=True)
    assert seen == [(a.data_ptr(), (2, 3, 16, 24), (1152, 384, 24, 1)), (b.data_ptr(), (2, 3, 16, 24), (1152, 1, 72, 3))]


def test_forward_and_backward_do_not_synchronise():
    from siu3r_amd import losses

    img, M, g_out = _inputs(3, 64, 64, seed=4)
    x, m, g = img.cuda(), M.cuda(), g_out.cuda()
    wx, wm = x.clone().requires_grad_(True), m.clone().requires_grad_(True)
    losses.apply_exposure(wx, wm).backward(g)
    a, b = x.clone().requires_grad_(True), m.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = losses.apply_exposure(a, b)
        out.backward(g)
        plain = losses.apply_exposure(x, m)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a.grad, wx.grad) and torch.equal(b.grad, wm.grad) and torch.equal(plain, out.detach())


def test_error_paths():
    from siu3r_amd import losses

    img, M = torch.rand(2, 3, 8, 8), torch.eye(3, 4).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.apply_exposure(img, M)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.apply_exposure(img.cuda(), M)
    with pytest.raises(ValueError, match="float32"):
        losses.apply_exposure(img.cuda().double(), M.cuda().double())
    with pytest.raises(ValueError, match="float32"):
        losses.apply_exposure(img.cuda(), M.cuda().bfloat16())
    with pytest.raises(ValueError, match="img must be"):
        losses.apply_exposure(torch.rand(2, 4, 8, 8).cuda(), M.cuda())
    with pytest.raises(ValueError, match="img must be"):
        losses.apply_exposure(img.cuda(), M.cuda(), channels_last=True)
    with pytest.raises(ValueError, match="img must be"):
        losses.apply_exposure(torch.rand(8, 8).cuda(), M.cuda())
    with pytest.raises(ValueError, match="M must be"):
        losses.apply_exposure(img.cuda(), M.cuda()[:1])
    with pytest.raises(ValueError, match="M must be"):
        losses.apply_exposure(img.cuda(), torch.eye(3).repeat(2, 1, 1).cuda())
    with pytest.raises(TypeError):
        losses.apply_exposure(img.cuda(), None)
