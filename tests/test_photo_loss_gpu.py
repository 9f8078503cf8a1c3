"""The fused photometric loss (siu3r_amd/losses.py, csrc/photo_loss.hip) on the GPU against tests/dense_photo64.py in float64.

Tolerance of the accuracy test: the float64 reference is evaluated on the SAME float32 inputs upcast; the composed float32 torch loss is
evaluated on the CPU for the same inputs, and the HIP result's error against float64 (relative for loss / L1 / SSIM, max-normalised for the
gradient) may be at most 2 x the composed float32 error (a different summation order), with a floor of 1e-6 (cases where float32 torch
happens to be exact)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_photo64 as D
from scenes import default_K, look_at_camera, random_scene

pytestmark = pytest.mark.gpu


def _images(kind, V, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        p, t = torch.rand(V, C, H, W, generator=g), torch.rand(V, C, H, W, generator=g)
    elif kind == "smooth":  # bilinear-upsampled 16 x 16 noise scaled into [0.2, 0.8] plus sigma-0.02 noise
        up = lambda: 0.2 + 0.6 * F.interpolate(torch.rand(V, C, 16, 16, generator=g), size=(H, W), mode="bilinear", align_corners=False)
        p = up() + 0.02 * torch.randn(V, C, H, W, generator=g)
        t = up() + 0.02 * torch.randn(V, C, H, W, generator=g)
    elif kind == "flat":  # exactly flat regions of constants that are exact in float32: both clamps active, apart and together
        p, t = torch.rand(V, C, H, W, generator=g), torch.rand(V, C, H, W, generator=g)
        p[..., : H // 2, : W // 2] = 0.5
        p[..., H // 2 + 5:, W // 2 + 9:] = 1.0
        t[..., H // 4:, W // 3:] = 0.0
        t[..., : H // 4, :] = 1.0
    else:
        raise ValueError(kind)
    p, t = p.float(), t.float()
    same = p == t
    p[same] = p[same] + 0.25  # pred != target everywhere: the L1 subgradient is defined
    assert not bool((p == t).any())
    return p, t


def _store(x, layout):
    """the [V,C,H,W] values stored on the GPU in `layout` -> (tensor to hand to the loss, channels_last)"""
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


CASES = [
    # kind, V, C, H, W, lambda, layout
    ("noise", 1, 1, 11, 11, 1.0, "nchw"),
    ("noise", 1, 3, 11, 11, 0.2, "nchw"),
    ("noise", 6, 3, 64, 80, 0.2, "nchw"),
    ("noise", 1, 3, 45, 70, 0.0, "nchw"),
    ("noise", 6, 1, 45, 70, 1.0, "nhwc"),
    ("noise", 6, 3, 64, 80, 0.2, "nhwc"),
    ("noise", 1, 3, 45, 70, 0.2, "sliced"),
    ("noise", 6, 3, 33, 47, 0.2, "nhwc_sliced"),
    ("noise", 6, 3, 512, 512, 0.2, "nchw"),
    ("smooth", 1, 3, 512, 512, 0.2, "nchw"),
    ("smooth", 6, 1, 100, 75, 1.0, "nchw"),
    ("smooth", 6, 3, 100, 75, 0.2, "nhwc"),
    ("smooth", 1, 3, 256, 256, 0.0, "nchw"),
    ("flat", 1, 3, 96, 130, 0.2, "nchw"),
    ("flat", 6, 1, 96, 130, 1.0, "nchw"),
    ("flat", 6, 3, 70, 70, 0.2, "nhwc"),
    ("flat", 1, 1, 96, 130, 0.0, "sliced"),
]


@pytest.mark.parametrize("kind,V,C,H,W,lam,layout", CASES)
def test_value_and_gradient_against_float64(kind, V, C, H, W, lam, layout):
    from siu3r_amd import losses

    p, t = _images(kind, V, C, H, W, seed=V * 1000 + H + C)
    (ref_v, ref_g) = D.loss_and_grad(p, t, lam, dtype=torch.float64)
    (cmp_v, cmp_g) = D.loss_and_grad(p, t, lam, dtype=torch.float32)
    pd, cl = _store(p, layout)
    td, _ = _store(t, layout)
    pd.requires_grad_(True)
    out = losses.photometric_loss(pd, td, lam, channels_last=cl, return_terms=True)
    out[0].backward()
    assert pd.grad.shape == pd.shape
    hip_g = (pd.grad.permute(0, 3, 1, 2) if cl else pd.grad).cpu().double()
    hip_v = [float(x.detach()) for x in out]
    gmax = float(ref_g.abs().max())
    rows = []
    for name, r, c, h in zip(("loss", "L1", "SSIM"), ref_v, cmp_v, hip_v):
        if r is None:
            assert np.isnan(h), f"{name} is switched off by lambda = {lam} and must come back as NaN"
            continue
        rows.append((name, abs(c - r) / abs(r), abs(h - r) / abs(r)))
    rows.append(("grad", float((cmp_g.double() - ref_g).abs().max()) / gmax, float((hip_g - ref_g).abs().max()) / gmax))
    print(f"\n{kind} V={V} C={C} {H}x{W} lambda={lam} {layout}: " + "; ".join(f"{n} composed-f32 {c:.2e} hip {h:.2e}" for n, c, h in rows))
    assert torch.isfinite(hip_g).all()
    for n, c, h in rows:
        assert h <= max(2.0 * c, 1e-6), f"{n}: hip error {h:.3e} > max(2 x composed float32 error {c:.3e}, 1e-6)"


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_two_calls_give_identical_bits(layout):
    from siu3r_amd import losses

    p, t = _images("smooth", 6, 3, 200, 150, seed=3)
    pd, cl = _store(p, layout)
    td, _ = _store(t, layout)
    res = []
    for _ in range(2):
        x = pd.detach().clone().requires_grad_(True)
        out = losses.photometric_loss(x, td, 0.2, channels_last=cl, return_terms=True)
        out[0].backward()
        res.append((torch.stack(out).detach().clone(), x.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(losses.ssim(pd, td, channels_last=cl, reduction="none"), losses.ssim(pd, td, channels_last=cl, reduction="none"))


def _render(V=3, H=128, W=128, G=20000, seed=0, grad=False):
    from siu3r_amd.cuda_splatting import render_cuda

    means, cov, opac, sh = (x.cuda() for x in random_scene(G, seed=seed, n_sh=4))
    leaves = [x.requires_grad_(grad) for x in (means, cov, sh, opac)]
    c2w = torch.stack([look_at_camera(seed=i) for i in range(V)]).cuda()
    K = default_K()[None].repeat(V, 1, 1).cuda()
    e = lambda x: x[None].expand(V, *x.shape)
    img, _ = render_cuda(c2w, K, torch.full((V,), 0.1), torch.full((V,), 100.0), (H, W), torch.zeros(V, 3), e(means), e(cov), e(sh), e(opac))
    return img, leaves


def test_ssim_of_a_render_is_metrics_ssim():
    """per view against the evaluator's CPU float64 SSIM.  Bound 1e-4 absolute: a float32 window second moment carries up to ~4 ulp of 0.25
    (6e-8); at a flat window (the render's background) that stands against c2 = 9e-4, i.e. 7e-5 relative on an SSIM value <= 1."""
    from siu3r_amd import losses, metrics

    with torch.no_grad():
        img, _ = _render()
    tgt = img.roll(1, 0).contiguous()
    got = losses.ssim(img, tgt, data_range=1.0, reduction="none").cpu()
    mean = float(losses.ssim(img, tgt))
    assert got.shape == (3,)
    for v in range(3):
        ref = metrics.ssim(img[v].permute(1, 2, 0).cpu().numpy(), tgt[v].permute(1, 2, 0).cpu().numpy(), data_range=1.0)
        print(f"view {v}: metrics.ssim {ref:.9f} losses.ssim {float(got[v]):.9f}")
        assert abs(float(got[v]) - ref) <= 1e-4
    assert abs(mean - float(got.double().mean())) <= 1e-6


def test_autograd_plumbing():
    from siu3r_amd import losses

    p, t = _images("noise", 2, 3, 40, 50, seed=9)
    pd, td = p.cuda(), t.cuda()
    a = pd.clone().requires_grad_(True)
    losses.photometric_loss(a, td).backward()
    b = pd.clone().requires_grad_(True)
    (losses.photometric_loss(b, td) * 3.0).backward()
    assert torch.equal(b.grad, a.grad * 3.0)
    # without requires_grad: the plain forward, the same bits
    plain = losses.photometric_loss(pd, td)
    assert plain.grad_fn is None and plain.dim() == 0 and plain.is_cuda
    assert torch.equal(plain, losses.photometric_loss(pd.clone().requires_grad_(True), td).detach())
    with torch.no_grad():
        assert losses.photometric_loss(pd.clone().requires_grad_(True), td).grad_fn is None
    # the target receives no gradient
    tt = td.clone().requires_grad_(True)
    assert losses.photometric_loss(pd, tt).grad_fn is None
    c = pd.clone().requires_grad_(True)
    losses.photometric_loss(c, tt).backward()
    assert tt.grad is None and torch.equal(c.grad, a.grad)
    # a single image without V, and the terms
    one = pd[0].clone().requires_grad_(True)
    l, l1_, ss = losses.photometric_loss(one, td[0], return_terms=True)
    l.backward()
    assert one.grad.shape == one.shape and not l1_.requires_grad and not ss.requires_grad
    assert abs(float(l) - (0.8 * float(l1_) + 0.2 * (1 - float(ss)))) <= 1e-6
    assert abs(float(losses.l1(pd, td)) - float((pd - td).abs().mean())) <= 1e-6
    d = pd.clone().requires_grad_(True)
    losses.ssim(d, td).backward()
    e = pd.clone().requires_grad_(True)
    losses.photometric_loss(e, td, 1.0).backward()
    assert torch.equal(d.grad, -e.grad)


def test_render_losses_backpropagate_in_the_stored_layout(monkeypatch):
    """K2 render [V,3,H,W] and gsplat-seam render [V,H,W,3]: the kernel receives the render's own storage (no permuted copy)"""
    from siu3r_amd import losses
    from siu3r_amd.compat import gsplat

    seen = []
    real = losses._launch
    monkeypatch.setattr(losses, "_launch", lambda p4, t4, *a: (seen.append((p4.data_ptr(), tuple(p4.shape), tuple(p4.stride()))), real(p4, t4, *a))[1])
    img, leaves = _render(grad=True)
    V, _, H, W = img.shape
    target = torch.rand(V, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    losses.photometric_loss(img, target).backward()
    assert seen[-1] == (img.data_ptr(), (V, 3, H, W), (3 * H * W, H * W, W, 1))
    for x in leaves:
        assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0

    means, cov, opac, sh = (x.cuda() for x in random_scene(20000, seed=0, n_sh=4))
    rgb = torch.rand(20000, 3, generator=torch.Generator().manual_seed(2)).cuda()
    leaves = [x.requires_grad_(True) for x in (means, cov, opac, rgb)]
    vm = torch.linalg.inv(torch.stack([look_at_camera(seed=i) for i in range(V)])).cuda()
    Ks = (default_K() * torch.tensor([[W], [H], [1.0]]))[None].repeat(V, 1, 1).cuda()
    colors, _, _ = gsplat.rasterization(means, None, None, opac, rgb, vm, Ks, W, H, covars=cov)
    assert colors.shape == (V, H, W, 3)
    losses.photometric_loss(colors, target.permute(0, 2, 3, 1), channels_last=True).backward()
    assert seen[-1] == (colors.data_ptr(), (V, 3, H, W), (3 * H * W, 1, 3 * W, 3))
    for x in leaves:
        assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


def test_error_paths():
    from siu3r_amd import losses

    p, t = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.photometric_loss(p, t)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.ssim(p.cuda(), t)
    with pytest.raises(ValueError, match="float32"):
        losses.photometric_loss(p.cuda().double(), t.cuda().double())
    with pytest.raises(ValueError, match="float32"):
        losses.l1(p.cuda().bfloat16(), t.cuda())
    with pytest.raises(ValueError, match="shape"):
        losses.photometric_loss(p.cuda(), t.cuda()[:, :, :15])
    small_p, small_t = torch.rand(1, 3, 10, 32).cuda(), torch.rand(1, 3, 10, 32).cuda()
    with pytest.raises(ValueError, match="11 x 11"):
        losses.photometric_loss(small_p, small_t)
    with pytest.raises(ValueError, match="11 x 11"):
        losses.ssim(small_p, small_t)
    with pytest.raises(ValueError, match="11 x 11"):
        losses.ssim(torch.rand(1, 32, 10, 3).cuda(), torch.rand(1, 32, 10, 3).cuda(), channels_last=True)
    assert float(losses.l1(small_p, small_t)) > 0  # L1 alone needs no window
    assert float(losses.photometric_loss(small_p, small_t, 0.0)) > 0
    with pytest.raises(ValueError, match="lambda"):
        losses.photometric_loss(p.cuda(), t.cuda(), 1.5)
    with pytest.raises(ValueError, match="reduction"):
        losses.ssim(p.cuda(), t.cuda(), reduction="sum")
    with pytest.raises(ValueError):
        losses.photometric_loss(torch.rand(16, 16).cuda(), torch.rand(16, 16).cuda())


def test_loss_and_backward_do_not_synchronise():
    from siu3r_amd import losses

    p, t = _images("noise", 3, 3, 64, 64, seed=4)
    pd, td = p.cuda(), t.cuda()
    warm = pd.clone().requires_grad_(True)
    losses.photometric_loss(warm, td).backward()
    x = pd.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = losses.photometric_loss(x, td)
        loss.backward()
        plain = losses.photometric_loss(pd, td, return_terms=True)
        per_view = losses.ssim(pd, td, reduction="none")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(x.grad, warm.grad) and torch.equal(plain[0], loss.detach()) and per_view.shape == (3,)


def test_code_object_resources():
    """no GPU needed: no kernel of the unit uses scratch memory, and the LDS of each leaves room for two workgroups per CU (160 KiB)"""
    from siu3r_amd import build as B

    res = B.kernel_resources("photo_loss.hip")
    names = ("photo_ssim_kernelILb1", "photo_ssim_kernelILb0", "photo_l1_kernel", "photo_finalize_kernel")
    for n in names:
        assert any(n in k for k in res), (n, sorted(res))
    for k, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert 2 * r["LDS Size [bytes/block]"] <= 160 * 1024, (k, r)
