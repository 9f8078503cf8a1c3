"""GPU tests of the gsplat-family HIP backward (csrc/raster_bwd_k3.hip, composite_rgb_bwd_kernel<K3> in csrc/raster_bwd.hip,
raster._RasterizeK3 / _RasterizeK3RGB and the viewer helpers) and the seams that expose it (compat/gsplat.rasterization,
SplattingCUDA.forward(render_qc_logits=True)): gradients against the float64 dense reference (tests/dense_gsplat64.py), unchanged forward
bits, multi-view sums, fits that lower their loss, error paths; and the matrix-core kernel's code object (no GPU needed for that one)."""
import os

import pytest
import torch

import dense_gsplat64 as DG
from scenes import default_K, look_at_camera, random_scene

# relative L2 error bar of every gradient tensor against the float64 reference (the K2 backward's bar)
REL_BAR = 5e-3
H, W = 48, 64


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _poses(V, H=H, W=W):
    vm = torch.stack([torch.linalg.inv(look_at_camera(s)) for s in range(V)])
    K = default_K()
    Ks = torch.tensor([[K[0, 0] * W, 0, K[0, 2] * W], [0, K[1, 1] * H, K[1, 2] * H], [0, 0, 1]], dtype=torch.float32)[None].repeat(V, 1, 1)
    return vm, Ks


def _cams(vm, Ks, H=H, W=W):
    from siu3r_amd import raster

    return [raster.make_cam_k3(vm[v], float(Ks[v, 0, 0]), float(Ks[v, 1, 1]), float(Ks[v, 0, 2]), float(Ks[v, 1, 2]), W, H) for v in range(len(vm))]


def _masks(vm, Ks, means, cov6):
    """tile masks and depth keys of the forward (the projection alone decides them; a no-grad call of the same inputs)"""
    from siu3r_amd import raster

    with torch.no_grad():
        o = raster.rasterize_views_k3(_cams(vm, Ks), means.cuda(), cov6.cuda(), torch.full((means.shape[0],), 0.5, device="cuda"),
                                      torch.zeros(means.shape[0], 1, device="cuda"), pose_dev=(vm.cuda(), Ks.cuda()))
    st = o["state"]
    return [DG.tile_mask_from_rect(st["rect"][v].cpu(), W, H) for v in range(len(vm))], [st["rec"][v, :, 2].cpu() for v in range(len(vm))]


def _scene(G, seed, C):
    means, cov, opac, _ = random_scene(G, seed=seed, spread=1.2)
    feats = torch.rand(G, C, generator=torch.Generator().manual_seed(seed)) * 2 - 0.5
    return means, cov, opac, feats


CONFIGS = [  # (channels, views, covariance layout, background, finite_features)
    (3, 1, "6", True, True),
    (3, 2, "33", False, True),
    (5, 1, "33", True, True),
    (21, 2, "6", False, True),
    (32, 1, "6", True, True),
    (64, 3, "33", False, True),
    (64, 1, "6", True, False),
    (168, 2, "33", True, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("C,V,layout,with_bg,finite", CONFIGS)
def test_gradients_match_the_float64_reference(C, V, layout, with_bg, finite):
    from siu3r_amd import raster
    from siu3r_amd.compat.gsplat import rasterization

    G = 400
    means, cov, opac, feats = _scene(G, 3 + C + V, C)
    covx = cov if layout == "33" else raster.cov6_from_cov3x3(cov)
    vm, Ks = _poses(V)
    bg = torch.rand(V, C, generator=torch.Generator().manual_seed(C)) if with_bg else None
    leaves = [t.cuda().requires_grad_() for t in (means, covx, opac, feats, vm)] + ([bg.cuda().requires_grad_()] if with_bg else [])
    out, alphas, _ = rasterization(leaves[0], None, None, leaves[2], leaves[3], leaves[4], Ks.cuda(), W, H, covars=leaves[1], sh_degree=None,
                                   backgrounds=leaves[5] if with_bg else None, finite_features=finite)
    torch.manual_seed(C)
    w_c, w_a = torch.randn(V, H, W, C), torch.randn(V, H, W, 1)
    loss = (out * w_c.cuda()).sum() + (alphas * w_a.cuda()).sum()
    got = torch.autograd.grad(loss, leaves)
    masks, keys = _masks(vm, Ks, means, raster.cov6_from_cov3x3(cov))
    ref_leaves = [t.detach().cpu().double().requires_grad_() for t in leaves]
    cams = _cams(vm, Ks)
    ref_loss = 0.0
    for v in range(V):
        col, a = DG.render(cams[v], ref_leaves[0], ref_leaves[1], ref_leaves[3], ref_leaves[2], masks[v], viewmat=ref_leaves[4][v],
                           depth_key=keys[v], bg=ref_leaves[5][v] if with_bg else None)
        ref_loss = ref_loss + (col * w_c[v].double()).sum() + (a * w_a[v, ..., 0].double()).sum()
    ref = torch.autograd.grad(ref_loss, ref_leaves)
    names = ["means", "covars", "opacities", "colors", "viewmats", "backgrounds"]
    for name, g, r in zip(names, got, ref):
        e = _rel(g, r)
        assert e <= REL_BAR, (name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_viewer_argument_list_gradients(degree):
    """quats + scales, SH colours [G,K,3] with sh_degree, a white background, two views: gradients of every input but Ks"""
    from siu3r_amd.compat.gsplat import rasterization

    G, V = 300, 2
    g = torch.Generator().manual_seed(degree)
    means, _, opac, _ = random_scene(G, seed=11 + degree, spread=1.2)
    quats = torch.randn(G, 4, generator=g)
    scales = 0.02 + 0.1 * torch.rand(G, 3, generator=g)
    sh = (torch.rand(G, 25, 3, generator=g) * 2 - 1) * 0.5
    vm, Ks = _poses(V)
    bg = torch.ones(3)
    leaves = [t.cuda().requires_grad_() for t in (means, quats, scales, opac, sh, vm, bg)]
    Ksd = Ks.cuda().requires_grad_()
    out, alphas, _ = rasterization(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], leaves[5], Ksd, W, H, sh_degree=degree,
                                   backgrounds=leaves[6], packed=True, absgrad=False, sparse_grad=False)
    w_c, w_a = torch.randn(V, H, W, 3, generator=g), torch.randn(V, H, W, 1, generator=g)
    loss = (out * w_c.cuda()).sum() + (alphas * w_a.cuda()).sum()
    loss.backward()
    assert Ksd.grad is None  # gsplat gives Ks no gradient
    masks, keys = _masks(vm, Ks, means, DG.quat_scale_to_cov6(quats, scales).float())
    ref = [t.detach().cpu().double().requires_grad_() for t in leaves]
    cams = _cams(vm, Ks)
    ref_loss = 0.0
    cov6 = DG.quat_scale_to_cov6(ref[1], ref[2])
    for v in range(V):
        rgb = DG.sh_eval(ref[0], torch.linalg.inv(ref[5][v])[:3, 3], ref[4], degree)
        col, a = DG.render(cams[v], ref[0], cov6, rgb, ref[3], masks[v], viewmat=ref[5][v], depth_key=keys[v], bg=ref[6])
        ref_loss = ref_loss + (col * w_c[v].double()).sum() + (a * w_a[v, ..., 0].double()).sum()
    ref_loss.backward()
    for name, t, r in zip(["means", "quats", "scales", "opacities", "sh", "viewmats", "backgrounds"], leaves, ref):
        assert _rel(t.grad, r.grad) <= REL_BAR, (name, _rel(t.grad, r.grad))


@pytest.mark.gpu
def test_forward_bits_unchanged_under_grad():
    from siu3r_amd.compat.gsplat import rasterization

    G, V = 500, 2
    means, cov, opac, feats = _scene(G, 5, 168)
    vm, Ks = _poses(V)
    quats = torch.randn(G, 4, generator=torch.Generator().manual_seed(0))
    scales = 0.02 + 0.1 * torch.rand(G, 3, generator=torch.Generator().manual_seed(1))
    sh = torch.rand(G, 16, 3, generator=torch.Generator().manual_seed(2)) - 0.5
    bg = torch.rand(3).cuda()
    calls = [
        lambda t: rasterization(t[0], None, None, t[2], t[3], t[4], Ks.cuda(), W, H, covars=t[1]),
        lambda t: rasterization(t[0], None, None, t[2], t[3][:, :21], t[4], Ks.cuda(), W, H, covars=t[1]),
        lambda t: rasterization(t[0], None, None, t[2], t[3][:, :64], t[4], Ks.cuda(), W, H, covars=t[1], finite_features=False),
        lambda t: rasterization(t[0], None, None, t[2], t[3][:, :3], t[4], Ks.cuda(), W, H, covars=t[1], backgrounds=bg),
        lambda t: rasterization(t[0], t[5], t[6], t[2], t[7], t[4], Ks.cuda(), W, H, sh_degree=3, backgrounds=torch.ones(3).cuda()),
    ]
    base = [t.cuda() for t in (means, cov, opac, feats, vm, quats, scales, sh)]
    for call in calls:
        with torch.no_grad():
            c0, a0, _ = call(base)
        c1, a1, _ = call([t.clone().requires_grad_() for t in base])
        assert c1.grad_fn is not None and torch.equal(c0, c1.detach()) and torch.equal(a0, a1.detach())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 168])
def test_multi_view_call_equals_the_sum_of_single_views(C):
    from siu3r_amd import raster

    G, V = 600, 3
    means, cov, opac, feats = _scene(G, 8, C)
    vm, Ks = _poses(V)
    cov6 = raster.cov6_from_cov3x3(cov)
    fn = raster.rasterize_views_k3_rgb if C == 3 else raster.rasterize_views_k3
    w = torch.randn(V, H, W, C).cuda()

    def grads(views):
        leaves = [t.cuda().requires_grad_() for t in (means, cov6, opac, feats)]
        o = fn(_cams(vm[views], Ks[views]), *leaves, pose_dev=(vm[views].cuda(), Ks[views].cuda()))
        loss = (o["colors"] * w[views]).sum() + o["alphas"].sum()
        return torch.autograd.grad(loss, leaves)

    together = grads(list(range(V)))
    single = [grads([v]) for v in range(V)]
    for i in range(4):
        s = sum(sg[i] for sg in single)
        assert _rel(together[i], s) <= 1e-5, (i, _rel(together[i], s))


@pytest.mark.gpu
def test_splatting_qc_logit_render_gradients():
    """SplattingCUDA.forward(render_qc_logits=True) with the camera tensors on the device (the pose_c2w route): gradients of means,
    covariances, opacities and the per-Gaussian query-class logits against the reference.  The renderer rescales means x10 and covariances
    x100 in place (the reference's quirk, recorded by autograd as the reference's torch products are): the Gaussians handed in receive
    x10 / x100 the gradient of the rescaled buffers it renders, and the render is the same bits as without grad."""
    from siu3r_amd import raster
    from siu3r_amd.gaussian_renderer import SplattingCUDA
    from siu3r_amd.gaussians_types import Gaussians

    G, v, q, c = 300, 2, 2, 4
    means, cov, opac, _ = random_scene(G, seed=21, spread=1.2)
    means, cov = means * 0.1, cov * 0.01  # the renderer scales them back
    qcl = torch.randn(G, q, c, generator=torch.Generator().manual_seed(0))
    c2w = torch.stack([look_at_camera(s) for s in range(v)])
    c2w[:, :3, 3] *= 0.1
    K = default_K()[None].repeat(v, 1, 1)
    leaves = [t.cuda().requires_grad_() for t in (means, cov, opac, qcl)]
    r = SplattingCUDA()

    def render(m, cv):  # the Gaussians as a network hands them over: non-leaf tensors, rescaled in place by the renderer
        gs = Gaussians(means=m[None], covariances=cv[None], harmonics=torch.zeros(1, G, 3, 25, device="cuda"), opacities=leaves[2][None],
                       seg_query_class_logits=leaves[3][None])
        return r.forward(gs, c2w[None].cuda(), K[None].cuda(), (H, W), render_color=False, render_qc_logits=True)["render_qc_logits"][0]

    m_buf, c_buf = leaves[0] * 1.0, leaves[1] * 1.0
    out = render(m_buf, c_buf)  # [v, q, c, h, w]
    with torch.no_grad():
        out0 = render(leaves[0].detach().clone(), leaves[1].detach().clone())
    assert torch.equal(out.detach(), out0)  # the recorded rescale is the kernel's product: same bits
    with pytest.raises(RuntimeError, match="leaf"):  # as in the reference: a leaf that requires grad cannot be rescaled in place
        render(leaves[0], leaves[1])
    wq = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    got = torch.autograd.grad((out * wq.cuda()).sum(), leaves)
    # the reference renders what the renderer rendered: the rescaled buffers, world->camera = inverse of the x10-translated extrinsics
    ref_leaves = [m_buf.detach().cpu().double().requires_grad_(), c_buf.detach().cpu().double().requires_grad_()] + \
                 [t.detach().cpu().double().requires_grad_() for t in leaves[2:]]
    ref_loss = 0.0
    for j in range(v):
        e = c2w[j].clone()
        e[:3, 3] = e[:3, 3] * r.scale_factor
        w2c = torch.linalg.inv(e.double()).float()
        cam = raster.make_cam_k3(w2c, float(K[j, 0, 0]) * W, float(K[j, 1, 1]) * H, float(K[j, 0, 2]) * W, float(K[j, 1, 2]) * H, W, H,
                                 near_plane=1.0, far_plane=r.far * r.scale_factor)
        with torch.no_grad():
            o = raster.rasterize_views_k3([cam], m_buf.detach(), c_buf.detach(), leaves[2].detach(), torch.zeros(G, 1, device="cuda"))
        mask = DG.tile_mask_from_rect(o["state"]["rect"][0].cpu(), W, H)
        col, _ = DG.render(cam, ref_leaves[0], ref_leaves[1], ref_leaves[3].reshape(G, q * c), ref_leaves[2], mask, depth_key=o["state"]["rec"][0, :, 2].cpu())
        ref_loss = ref_loss + (col.reshape(H, W, q, c).permute(2, 3, 0, 1) * wq[j].double()).sum()
    ref = torch.autograd.grad(ref_loss, ref_leaves)
    # d loss / d means = 10 d loss / d (rescaled means), d loss / d covariances = 100 d loss / d (rescaled covariances)
    ref = [ref[0] * r.scale_factor, ref[1] * r.scale_factor ** 2, ref[2], ref[3]]
    for name, g_, r_ in zip(["means", "covariances", "opacities", "qc_logits"], got, ref):
        assert _rel(g_, r_) <= REL_BAR, (name, _rel(g_, r_))


@pytest.mark.gpu
def test_feature_fit_with_fixed_geometry_lowers_the_loss():
    """Adam on 168-channel features towards a target render of other features, geometry fixed.  Measured on one MI355X (this loop; the same
    loop on the float64 dense reference takes far longer than a test may): the MSE falls from 0.185 to 8.3e-4 in 60 steps (x 0.0045); the bar is x 0.25."""
    from siu3r_amd import raster

    G, C, V = 800, 168, 2
    means, cov, opac, feats = _scene(G, 30, C)
    vm, Ks = _poses(V)
    cams = _cams(vm, Ks)
    geo = [t.cuda() for t in (means, raster.cov6_from_cov3x3(cov), opac)]
    pose = (vm.cuda(), Ks.cuda())
    with torch.no_grad():
        target = raster.rasterize_views_k3(cams, *geo, feats.cuda(), pose_dev=pose)["colors"]
    f = torch.zeros(G, C, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([f], lr=0.05)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = ((raster.rasterize_views_k3(cams, *geo, f, pose_dev=pose)["colors"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0] / 4, (losses[0], losses[-1])


@pytest.mark.gpu
def test_gsplat_style_fit_lowers_the_l1_loss():
    """means, quats, log-scales, logit opacities and SH (degree 1) from a perturbed start, through the shim, towards the render of the
    unperturbed scene.  Measured on one MI355X (this loop; on the float64 reference it takes far longer than a test may): the L1 loss falls from 0.052 to 0.0021
    in 80 steps (x 0.040); the bar is x 0.75."""
    from siu3r_amd.compat.gsplat import rasterization

    G, V = 600, 2
    g = torch.Generator().manual_seed(5)
    means, _, opac, _ = random_scene(G, seed=31, spread=1.0)
    quats = torch.randn(G, 4, generator=g)
    log_s = torch.log(0.03 + 0.08 * torch.rand(G, 3, generator=g))
    logit_o = torch.logit(opac.clamp(0.05, 0.95))
    sh = (torch.rand(G, 4, 3, generator=g) * 2 - 1) * 0.5
    vm, Ks = _poses(V)
    vm, Ks = vm.cuda(), Ks.cuda()

    def render(m, q, ls, lo, s):
        out, _, _ = rasterization(m, q, torch.exp(ls), torch.sigmoid(lo), s, vm, Ks, W, H, sh_degree=1, backgrounds=torch.ones(3, device="cuda"))
        return out

    with torch.no_grad():
        target = render(*(t.cuda() for t in (means, quats, log_s, logit_o, sh)))
    noise = lambda t, s: t + s * torch.randn(t.shape, generator=g)
    params = [noise(means, 0.03), noise(quats, 0.2), noise(log_s, 0.2), noise(logit_o, 0.5), noise(sh, 0.2)]
    params = [p.cuda().requires_grad_() for p in params]
    opt = torch.optim.Adam([{"params": params[:1], "lr": 2e-3}, {"params": params[1:], "lr": 1e-2}])
    losses = []
    for _ in range(80):
        opt.zero_grad()
        loss = (render(*params) - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.75 * losses[0], (losses[0], losses[-1])


@pytest.mark.gpu
def test_error_paths():
    from siu3r_amd import raster

    G = 200
    means, cov, opac, feats = _scene(G, 40, 3)
    vm, Ks = _poses(1)
    cams = _cams(vm, Ks)
    leaves = [t.cuda().requires_grad_() for t in (means, raster.cov6_from_cov3x3(cov), opac, feats)]
    with pytest.raises(ValueError, match="deferred"):
        raster.rasterize_views_k3_rgb(cams, *leaves, check_overflow="deferred")
    with torch.no_grad():  # without grad the deferred check stays available
        raster.rasterize_views_k3_rgb(cams, *leaves, check_overflow="deferred")
    raster.check_pending()
    o = raster.rasterize_views_k3(cams, *leaves)
    # an upstream gradient that requires grad: the gradient the backward returns carries the once-differentiable guard, and
    # differentiating it again is refused by name (not merely "does not require grad")
    wt = torch.rand(o["colors"].shape, device="cuda", requires_grad=True)
    (g,) = torch.autograd.grad((o["colors"] * wt).sum(), leaves[0], create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


@pytest.mark.gpu
def test_host_pose_tensors_get_host_gradients():
    """viewmats on the host (the shim's feature route) and a host camera centre (sh_eval) that require grad get their gradients back on the
    host, equal to those of the same tensors on the device"""
    from siu3r_amd import raster
    from siu3r_amd.compat.gsplat import rasterization

    G, V, C = 300, 2, 40
    means, cov, opac, feats = _scene(G, 50, C)
    vm, Ks = _poses(V)
    args = [t.cuda() for t in (means, raster.cov6_from_cov3x3(cov), opac, feats)]
    grads = []
    for dev in ("cpu", "cuda"):
        v = vm.clone().to(dev).requires_grad_()
        out, alphas, _ = rasterization(args[0], None, None, args[2], args[3], v, Ks.cuda(), W, H, covars=args[1])
        (out.sum() + alphas.sum()).backward()
        assert v.grad is not None and v.grad.device == v.device
        grads.append(v.grad)
    assert _rel(grads[0], grads[1]) <= 1e-6
    sh = (torch.rand(G, 9, 3, generator=torch.Generator().manual_seed(3)) - 0.5).cuda()
    cgrads = []
    for dev in ("cpu", "cuda"):
        cp = torch.tensor([0.1, -0.2, 0.05], device=dev, requires_grad=True)
        raster.sh_eval(args[0], cp, sh, 2).sum().backward()
        assert cp.grad is not None and cp.grad.device == cp.device
        cgrads.append(cp.grad)
    assert _rel(cgrads[0], cgrads[1]) <= 1e-6


@pytest.mark.gpu
def test_backward_reuses_or_builds_the_quadrant_lists():
    """the matrix-core forward leaves its per-quadrant lists for the backward; after the 32-channel forward (tune(0, 1)) the backward builds
    them itself: the same walk, the same gradients up to the order of the float atomics"""
    from siu3r_amd import raster

    G, V, C = 500, 2, 64
    means, cov, opac, feats = _scene(G, 60, C)
    vm, Ks = _poses(V)
    cams = _cams(vm, Ks)
    w = torch.randn(V, H, W, C).cuda()
    grads = []
    for form in (0, 1):
        raster.tune(0, form)
        try:
            leaves = [t.cuda().requires_grad_() for t in (means, raster.cov6_from_cov3x3(cov), opac, feats)]
            o = raster.rasterize_views_k3(cams, *leaves, pose_dev=(vm.cuda(), Ks.cuda()))
            assert bool(o["state"]["feat_ws_lists"]) == (form == 0)
            grads.append(torch.autograd.grad((o["colors"] * w).sum() + o["alphas"].sum(), leaves))
        finally:
            raster.tune(0, 0)
    for a, b in zip(*grads):
        assert _rel(a, b) <= 1e-5


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs the ROCm LLVM tools")
def test_matrix_core_backward_code_object():
    """the N-channel composite backward runs on the matrix cores, adds with hardware float atomics (no compare-and-swap loop) and
    keeps everything in registers"""
    import re

    from siu3r_amd import build as B
    from test_abi import _device_disassembly

    text = _device_disassembly("raster_bwd_k3.hip")
    m = re.search(r"<(_Z\S*composite_feat_bwd_kernel\S*)>:\n(.*?)(?:\n\n|\Z)", text, re.S)
    assert m, "composite_feat_bwd_kernel missing"
    body = m.group(2)
    assert "v_mfma_f32_32x32x2_f32" in body and "global_atomic_add_f32" in body and "cmpswap" not in body
    res = [r for name, r in B.kernel_resources("raster_bwd_k3.hip").items() if "composite_feat_bwd_kernel" in name]
    assert res and res[0]["ScratchSize [bytes/lane]"] == 0, res
