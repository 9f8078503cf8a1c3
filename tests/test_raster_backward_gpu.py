"""GPU tests of the K2 rasterizer's HIP backward (csrc/raster_bwd.hip, raster._RasterizeK2) and the seams that expose it: gradients
against the float64 dense reference (tests/dense_raster64.py), directional derivatives at scale, multi-view sums, error paths and
test-time pose alignment."""
import math

import pytest
import torch

import dense_raster64 as DR
from scenes import default_K, look_at_camera, random_scene

pytestmark = pytest.mark.gpu

# relative L2 error bar of every gradient tensor against the float64 reference.  Measured: 1e-6 .. 2e-5 where the two forwards take the
# same branches everywhere; up to 2.2e-3 (covariances, two views of precomputed colours) where a few pixels fall on different sides of
# alpha_min / t_min in fp32 and float64 (backward section)
REL_BAR = 5e-3


def _cam(H, W, seed, degree, band4=False, bg=(0.1, 0.2, 0.3), near=0.2, scale=1.0):
    from siu3r_amd import cuda_splatting as cs, raster

    c2w = look_at_camera(seed)
    c2w[:3, 3] *= scale
    K = default_K()[None]
    fov = cs.get_fov(K)
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([near]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(c2w)
    return raster.make_cam_k2(w2c, proj @ w2c, float(tan[0]), float(tan[1]), c2w[:3, 3].tolist(), list(bg), W, H, sh_degree=degree, sh_band4=band4)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


CONFIGS = [  # (sh degree, planar layout, band4, cov stride, views)
    (0, False, False, 6, 1),
    (1, True, False, 9, 2),
    (3, False, False, 9, 3),
    (4, True, True, 6, 1),
    (4, False, True, 9, 2),
    (4, False, False, 6, 1),
    (-1, False, False, 6, 2),
]


@pytest.mark.parametrize("deg,planar,band4,stride,V", CONFIGS)
def test_gradients_match_the_float64_reference(deg, planar, band4, stride, V):
    from siu3r_amd import raster

    H, W, G = 64, 96, 1500
    torch.manual_seed(deg + 10 * V)
    means, cov, opac, sh = random_scene(G, seed=3 + V, n_sh=25, spread=1.2)
    cams = [_cam(H, W, s, deg, band4) for s in range(V)]
    if deg < 0:
        cols = torch.rand(G, 1, 3) * 1.5 - 0.25  # precomputed colours, any sign
    elif planar:
        cols = sh.clone()  # [G, 3, 25]
    else:
        cols = sh.permute(0, 2, 1)[:, :max(1, (deg + 1) ** 2)].contiguous()  # [G, n, 3]
    covx = cov if stride == 9 else raster.cov6_from_cov3x3(cov)
    leaves = [t.cuda().requires_grad_() for t in (means, covx, cols, opac)]
    xi = torch.zeros(V, 6, device="cuda", requires_grad=True)
    o = raster.rasterize_views_k2(cams, *leaves, sh_planar=planar, pose_delta=xi)
    w1, w2, w3 = torch.randn(V, 3, H, W), torch.randn(V, H, W), torch.randn(V, H, W)
    loss = (o["image"] * w1.cuda()).sum() + (o["depth"] * w2.cuda()).sum() + (o["opacity"] * w3.cuda()).sum()
    got = torch.autograd.grad(loss, leaves + [xi])
    st = o["state"]
    ref_leaves = [t.detach().cpu().double().requires_grad_() for t in leaves]
    ref_xi = torch.zeros(V, 6, dtype=torch.float64, requires_grad=True)
    ref_loss = 0.0
    for v in range(V):
        mask = DR.tile_mask_from_rect(st["rect"][v].cpu(), W, H)
        img, d, a = DR.render(cams[v], ref_leaves[0], ref_leaves[1], ref_leaves[2], ref_leaves[3], mask, sh_planar=planar, xi=ref_xi[v],
                              depth_key=st["rec"][v, :, 2].cpu())
        ref_loss = ref_loss + (img * w1[v].double()).sum() + (d * w2[v].double()).sum() + (a * w3[v].double()).sum()
        # the same function up to fp32 rounding; a pixel where float64 and fp32 fall on different sides of alpha_min / t_min may differ more
        diff = (img.detach() - o["image"][v].detach().cpu().double()).abs()
        assert float((diff > 1e-4).double().mean()) <= 1e-3 and float(diff.max()) < 1e-2, float(diff.max())
    want = torch.autograd.grad(ref_loss, ref_leaves + [ref_xi])
    errs = {n: _rel(g, w) for n, g, w in zip(("means", "cov", "colors", "opacities", "pose"), got, want)}
    print("relative L2 errors", (deg, planar, band4, stride, V), {k: f"{e:.2e}" for k, e in errs.items()})
    if stride == 9:  # the gradient lands on exactly the entries the forward reads
        assert float(got[1].reshape(G, 9)[:, [3, 6, 7]].abs().max()) == 0.0
    for n, e in errs.items():
        assert e <= REL_BAR, (n, e, errs)


def _compat_settings(H, W, seed, degree=3, bg=(0.1, 0.2, 0.3)):
    from siu3r_amd import cuda_splatting as cs
    from siu3r_amd.compat.diff_gaussian_rasterization import GaussianRasterizationSettings

    c2w = look_at_camera(seed)
    K = default_K()[None]
    fov = cs.get_fov(K)
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([0.2]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(c2w)
    return GaussianRasterizationSettings(H, W, float(tan[0]), float(tan[1]), torch.tensor(bg), 1.0, w2c.T.contiguous().cuda(),
                                         (proj @ w2c).T.contiguous().cuda(), None, degree, c2w[:3, 3].cuda(), False, False)


def test_compat_means2d_theta_rho_and_forward_bits():
    from siu3r_amd.compat.diff_gaussian_rasterization import GaussianRasterizer, make_cam

    H, W, G = 64, 96, 1200
    means, cov, opac, sh = random_scene(G, seed=11, n_sh=16, spread=1.2)
    from siu3r_amd import raster

    cov6 = raster.cov6_from_cov3x3(cov).cuda()
    shs = sh.permute(0, 2, 1).contiguous().cuda()
    s = _compat_settings(H, W, 4)
    r = GaussianRasterizer(s)
    with torch.no_grad():
        base = r(means3D=means.cuda(), means2D=None, shs=shs, opacities=opac.cuda()[:, None], cov3D_precomp=cov6)
    leaves = [means.cuda().requires_grad_(), cov6.clone().requires_grad_(), shs.clone().requires_grad_(), opac.cuda()[:, None].clone().requires_grad_()]
    m2d = torch.zeros(G, 3, device="cuda", requires_grad=True)
    theta = torch.zeros(3, device="cuda", requires_grad=True)
    rho = torch.zeros(3, device="cuda", requires_grad=True)
    out = r(means3D=leaves[0], means2D=m2d, shs=leaves[2], opacities=leaves[3], cov3D_precomp=leaves[1], theta=theta, rho=rho)
    for a, b in zip(out, base):
        assert torch.equal(a, b)
    assert out[0].grad_fn is not None
    w1, w2, w3 = torch.randn(3, H, W), torch.randn(1, H, W), torch.randn(1, H, W)
    loss = (out[0] * w1.cuda()).sum() + (out[2] * w2.cuda()).sum() + (out[3] * w3.cuda()).sum()
    loss.backward()
    cam = make_cam(s)
    ref = [t.detach().cpu().double().requires_grad_() for t in leaves]
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    off = torch.zeros(G, 2, dtype=torch.float64, requires_grad=True)  # the pixel-space mean gradient of the reference: a free offset
    o = raster.rasterize_views_k2([cam], *(t.detach() for t in leaves[:3]), leaves[3].detach().reshape(-1))
    st = o["state"]
    mask = DR.tile_mask_from_rect(st["rect"][0].cpu(), W, H)
    img, d, a = DR.render(cam, ref[0], ref[1], ref[2], ref[3].reshape(-1), mask, xi=xi, depth_key=st["rec"][0, :, 2].cpu(), mean2d_offset=off)
    rl = (img * w1.double()).sum() + (d * w2[0].double()).sum() + (a * w3[0].double()).sum()
    want = torch.autograd.grad(rl, ref + [xi, off])
    errs = {n: _rel(g.grad, w) for n, g, w in zip(("means", "cov", "shs", "opac"), leaves, want)}
    errs["rho"] = _rel(rho.grad, want[4][:3])
    errs["theta"] = _rel(theta.grad, want[4][3:])
    errs["means2D"] = _rel(m2d.grad[:, :2], want[5] * torch.tensor([W / 2, H / 2], dtype=torch.float64))
    print("compat relative L2 errors", {k: f"{e:.2e}" for k, e in errs.items()})
    for n, e in errs.items():
        assert e <= REL_BAR, (n, e, errs)
    # means2D: d loss / d NDC in the first two columns, nothing in the third
    assert float(m2d.grad[:, 2].abs().max()) == 0.0
    vis = (st["radii"][0, :, 0] > 0).nonzero()[:, 0].cpu()
    assert vis.numel() > 0
    # the same screen-space gradient, through the raw pixel-space holder of the autograd function
    hold = torch.zeros(G, 2, device="cuda", requires_grad=True)
    o2 = raster.rasterize_views_k2([cam], leaves[0].detach(), leaves[1].detach(), leaves[2].detach(), leaves[3].detach().reshape(-1), means2d=hold)
    ((o2["image"][0] * w1.cuda()).sum() + (o2["depth"][0] * w2[0].cuda()).sum() + (o2["opacity"][0] * w3[0].cuda()).sum()).backward()
    tol = 1e-5 * float(hold.grad.abs().max()) * W  # (float atomics: the sums of two backward runs differ in the last bits)
    assert torch.allclose(m2d.grad[:, 0], hold.grad[:, 0] * (W / 2), rtol=1e-4, atol=tol)
    assert torch.allclose(m2d.grad[:, 1], hold.grad[:, 1] * (H / 2), rtol=1e-4, atol=tol)
    # non-zero on the visible Gaussians, zero on the culled ones
    assert float(hold.grad[vis].abs().sum()) > 0 and float(hold.grad[(st["radii"][0, :, 0] == 0)].abs().sum()) == 0.0


def test_directional_derivatives_at_scale():
    """50k Gaussians, 256 x 256, six views in one call: <grad, d> against fp32 central differences of the HIP forward."""
    from siu3r_amd import raster

    H = W = 256
    G, V = 50000, 6
    means, cov, opac, sh = random_scene(G, seed=21, n_sh=16, spread=1.5)
    cams = [_cam(H, W, s, 3) for s in range(V)]
    # alpha_min, t_min -> 0: the forward is then continuous in opacity and colour (a finite difference across the 1/255 cut-off or the
    # saturation test measures their jumps, not the derivative on the branch); the tile rects still cut the footprints, so pose
    # directions cross them (larger tolerance)
    for c in cams:
        c.alpha_min, c.t_min = 1e-20, 1e-30
    cov6 = raster.cov6_from_cov3x3(cov).cuda()
    shs = sh.permute(0, 2, 1).contiguous().cuda()
    opac = (opac * 0.6).cuda()
    w1, w2, w3 = torch.randn(V, 3, H, W, device="cuda"), torch.randn(V, H, W, device="cuda"), torch.randn(V, H, W, device="cuda")

    def loss_of(o):
        return (o["image"] * w1).sum() + (o["depth"] * w2).sum() * 0.1 + (o["opacity"] * w3).sum()

    leaves = [shs.clone().requires_grad_(), opac.clone().requires_grad_()]
    xi = torch.zeros(V, 6, device="cuda", requires_grad=True)
    o = raster.rasterize_views_k2(cams, means.cuda(), cov6, leaves[0], leaves[1], pose_delta=xi)
    g_sh, g_op, g_xi = torch.autograd.grad(loss_of(o), leaves + [xi])
    m_leaf, c_leaf = means.cuda().requires_grad_(), cov6.clone().requires_grad_()
    gm_ = torch.autograd.grad(loss_of(raster.rasterize_views_k2(cams, m_leaf, c_leaf, shs, opac)), [m_leaf, c_leaf])
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, base, grad, eps in (("sh", shs, g_sh, 1e-3), ("opacity", opac, g_op, 1e-3)):
            d = torch.randn(base.shape, generator=gen).cuda()
            lp = loss_of(raster.rasterize_views_k2(cams, means.cuda(), cov6, *( (base + eps * d, opac) if name == "sh" else (shs, base + eps * d))))
            lm = loss_of(raster.rasterize_views_k2(cams, means.cuda(), cov6, *( (base - eps * d, opac) if name == "sh" else (shs, base - eps * d))))
            fd, an = float(lp - lm) / (2 * eps), float((grad * d).sum())
            print(f"directional derivative {name}: fd {fd:.6e} analytic {an:.6e}")
            assert abs(fd - an) <= 2e-2 * abs(an), (name, fd, an)
        # means and covariances move the integer tile rects too; along the (preconditioned) gradient, <g, d> >= 0 sums over every
        # Gaussian and outweighs the random-signed jumps of the few rects that change.  Covariances: d = cov * cov * g, scaled so that
        # no entry changes by more than eps of itself
        for name, base, grad, eps in (("means", means.cuda(), gm_[0], 1e-3), ("cov", cov6, gm_[1], 1e-3)):
            d = grad / grad.abs().max() if name == "means" else base * base * grad / (base * grad).abs().max()
            args_p = (base + eps * d, cov6) if name == "means" else (means.cuda(), base + eps * d)
            args_m = (base - eps * d, cov6) if name == "means" else (means.cuda(), base - eps * d)
            fd = float(loss_of(raster.rasterize_views_k2(cams, *args_p, shs, opac)) - loss_of(raster.rasterize_views_k2(cams, *args_m, shs, opac))) / (2 * eps)
            an = float((grad * d).sum())
            print(f"directional derivative {name} (along the gradient): fd {fd:.6e} analytic {an:.6e}")
            # measured: means 12 % (the tile-rect and frame-edge jumps; on fixed rects the means gradient agrees to 1e-6 .. 3e-4 with
            # the float64 reference above): a check of sign and scale at 50k Gaussians
            assert abs(fd - an) <= 0.2 * abs(an), (name, fd, an)
        # pose: the perturbed render of view v uses exp(xi^) w2c and the matching projection
        for v in (0, 3):
            d = torch.randn(6, generator=gen) * torch.tensor([1, 1, 1, 1, 1, 1.0])
            eps = 2e-4

            def perturbed(sign):
                cs = list(cams)
                w2c, P = DR.cam_tensors(cams[v])
                E = DR.se3_exp((sign * eps * d).double())
                c = _cam(H, W, v, 3)
                c.alpha_min, c.t_min = 1e-20, 1e-30
                from siu3r_amd.raster import _set

                _set(c.w2c, (E @ w2c).float().reshape(-1).tolist())
                _set(c.proj, (P @ torch.linalg.inv(w2c) @ E @ w2c).float().reshape(-1).tolist())
                cs[v] = c
                return loss_of(raster.rasterize_views_k2(cs, means.cuda(), cov6, shs, opac))

            fd, an = float(perturbed(1) - perturbed(-1)) / (2 * eps), float((g_xi[v].cpu() * d).sum())
            print(f"directional derivative pose view {v}: fd {fd:.6e} analytic {an:.6e}")
            assert abs(fd - an) <= 0.1 * abs(an) + 1e-2 * float(g_xi[v].norm()), (v, fd, an)


def test_multiview_pose_and_gaussian_gradients_match_single_calls():
    from siu3r_amd import cuda_splatting as cs

    H, W, G, b = 64, 96, 2000, 3
    means, cov, opac, sh = random_scene(G, seed=31, n_sh=16, spread=1.2)
    ext = torch.stack([look_at_camera(s) for s in range(b)]).cuda()
    K = default_K()[None].repeat(b, 1, 1).cuda()
    near, far = torch.full((b,), 0.5), torch.full((b,), 100.0)
    bg = torch.tensor([[0.1, 0.2, 0.3]]).repeat(b, 1)
    w = torch.randn(b, 3, H, W, device="cuda")
    wd = torch.randn(b, H, W, device="cuda")

    def run(views):
        leaves = [t.cuda().requires_grad_() for t in (means, cov, sh, opac)]
        rot = torch.zeros(len(views), 3, device="cuda", requires_grad=True)
        tr = torch.zeros(len(views), 3, device="cuda", requires_grad=True)
        n = len(views)
        img, dep = cs.render_cuda(ext[views], K[views], near[views], far[views], (H, W), bg[views], *(t[None].expand(n, *t.shape) for t in leaves),
                                  cam_rot_delta=rot, cam_trans_delta=tr)
        ((img * w[views]).sum() + (dep * wd[views]).sum()).backward()
        return [t.grad for t in leaves], rot.grad, tr.grad, img.detach()

    g_all, rot_all, tr_all, img_all = run(list(range(b)))
    singles = [run([v]) for v in range(b)]
    for v in range(b):
        assert torch.equal(img_all[v], singles[v][3][0])
        assert _rel(rot_all[v], singles[v][1][0]) < 1e-5 and _rel(tr_all[v], singles[v][2][0]) < 1e-5
    for i in range(4):
        assert _rel(g_all[i], sum(s[0][i] for s in singles)) < 1e-5, i


def test_render_cuda_forward_bits_unchanged_with_grad():
    from siu3r_amd import cuda_splatting as cs

    H, W, G, b = 64, 96, 2000, 2
    means, cov, opac, sh = random_scene(G, seed=41, n_sh=25)
    ext = torch.stack([look_at_camera(s) for s in range(b)]).cuda()
    K = default_K()[None].repeat(b, 1, 1).cuda()
    args = (ext, K, torch.full((b,), 0.5), torch.full((b,), 100.0), (H, W), torch.zeros(b, 3))
    g = [t.cuda()[None].expand(b, *t.shape) for t in (means, cov, sh, opac)]
    with torch.no_grad():
        ref = cs.render_cuda(*args, *g)
    gg = [t.cuda().requires_grad_() for t in (means, cov, sh, opac)]
    out = cs.render_cuda(*args, *(t[None].expand(b, *t.shape) for t in gg), cam_rot_delta=torch.zeros(b, 3, device="cuda", requires_grad=True),
                         cam_trans_delta=torch.zeros(b, 3, device="cuda", requires_grad=True))
    assert out[0].grad_fn is not None
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


def test_error_paths():
    from siu3r_amd import raster
    from siu3r_amd.compat.diff_gaussian_rasterization import GaussianRasterizer

    H, W, G = 32, 32, 200
    means, cov, opac, sh = random_scene(G, seed=51, n_sh=16)
    cam = _cam(H, W, 0, 3)
    cov6 = raster.cov6_from_cov3x3(cov).cuda()
    shs = sh.permute(0, 2, 1).contiguous().cuda()
    m = means.cuda().requires_grad_()
    with pytest.raises(ValueError, match="deferred"):
        raster.rasterize_views_k2([cam], m, cov6, shs, opac.cuda(), check_overflow="deferred")
    o = raster.rasterize_views_k2([cam], m, cov6, shs, opac.cuda())
    (g,) = torch.autograd.grad(o["image"].sum(), m, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), m)
    r = GaussianRasterizer(_compat_settings(H, W, 0))
    with pytest.raises(Exception, match="scale"):
        r(means3D=m, means2D=None, shs=shs, opacities=opac.cuda()[:, None], scales=torch.ones(G, 3, device="cuda"),
          rotations=torch.ones(G, 4, device="cuda"))


def test_align_pose_recovers_a_perturbed_camera():
    from siu3r_amd import cuda_splatting as cs
    from siu3r_amd.pose_align import _se3_exp, align_pose

    H = W = 128
    G = 20000
    means, cov, opac, sh = random_scene(G, seed=61, n_sh=4, spread=1.5, scale=(0.02, 0.1))
    g = [t.cuda() for t in (means, cov, sh, opac)]
    true = look_at_camera(3).cuda()
    K = default_K().cuda()
    with torch.no_grad():
        target, _ = cs.render_cuda(true[None], K[None], torch.tensor([0.5]), torch.tensor([100.0]), (H, W), torch.zeros(1, 3),
                                   *(t[None] for t in g))
    axis = torch.tensor([0.3, -0.8, 0.5])
    axis = axis / axis.norm()
    xi0 = torch.cat((torch.tensor([0.03, -0.03, 0.029]), axis * math.radians(3.0))).cuda()
    start = true @ _se3_exp(xi0)

    def errs(c2w):
        d = torch.linalg.inv(true) @ c2w
        ang = math.degrees(math.acos(max(-1.0, min(1.0, (float(torch.trace(d[:3, :3])) - 1) / 2))))
        return ang, float((c2w[:3, 3] - true[:3, 3]).norm())

    r0, t0 = errs(start)
    c2w, losses = align_pose(*g, target[0], K, start, 0.5, 100.0, (0, 0, 0), iters=400, lr=5e-3)
    r1, t1 = errs(c2w)
    print(f"align_pose: rotation {r0:.3f} -> {r1:.4f} deg, translation {t0:.4f} -> {t1:.5f}, loss {losses[0]:.4f} -> {losses[-1]:.5f}")
    assert r1 <= r0 / 10 and t1 <= t0 / 10, (r0, r1, t0, t1)


def test_depth_gradients_at_the_splatting_scale():
    """SplattingCUDA renders the scene scaled x10 (depths of tens of units, far = 1000): the part of the depth behind an entry is a
    difference of fp32 totals, so its rounding grows with the depth.  A depth-weighted loss at that scale against the float64 reference."""
    from siu3r_amd import raster

    H, W, G, V = 64, 96, 1500, 2
    means, cov, opac, sh = random_scene(G, seed=71, n_sh=16, spread=1.2)
    means, cov = means * 10.0, cov * 100.0
    cams = [_cam(H, W, s, 3, near=1.0, scale=10.0) for s in range(V)]
    shs = sh.permute(0, 2, 1).contiguous()
    leaves = [t.cuda().requires_grad_() for t in (means, cov, shs, opac)]
    xi = torch.zeros(V, 6, device="cuda", requires_grad=True)
    o = raster.rasterize_views_k2(cams, *leaves, pose_delta=xi)
    w2, w1 = torch.randn(V, H, W), 0.1 * torch.randn(V, 3, H, W)
    loss = (o["depth"] * w2.cuda()).sum() + (o["image"] * w1.cuda()).sum()
    got = torch.autograd.grad(loss, leaves + [xi])
    st = o["state"]
    ref = [t.detach().cpu().double().requires_grad_() for t in leaves]
    ref_xi = torch.zeros(V, 6, dtype=torch.float64, requires_grad=True)
    rl = 0.0
    for v in range(V):
        mask = DR.tile_mask_from_rect(st["rect"][v].cpu(), W, H)
        img, d, a = DR.render(cams[v], *ref, mask, xi=ref_xi[v], depth_key=st["rec"][v, :, 2].cpu())
        rl = rl + (d * w2[v].double()).sum() + (img * w1[v].double()).sum()
    want = torch.autograd.grad(rl, ref + [ref_xi])
    errs = {n: _rel(g, w) for n, g, w in zip(("means", "cov", "shs", "opacities", "pose"), got, want)}
    print("relative L2 errors at the x10 scale (depth-weighted)", {k: f"{e:.2e}" for k, e in errs.items()})
    for n, e in errs.items():
        assert e <= REL_BAR, (n, e, errs)


def test_splatting_cuda_pose_gradients_match_per_view_render_calls():
    """SplattingCUDA.forward hands cam_rot_delta / cam_trans_delta [b,v,3] to render_cuda per batch item: the gradients equal those of
    per-view render_cuda calls on the x10-scaled scene (translation_scale = 10)."""
    from siu3r_amd import cuda_splatting as cs
    from siu3r_amd.gaussian_renderer import SplattingCUDA
    from siu3r_amd.gaussians_types import Gaussians

    H, W, G, b, v = 64, 96, 2000, 2, 2
    scenes = [random_scene(G, seed=81 + i, n_sh=16, spread=1.2) for i in range(b)]
    means, cov, opac, sh = (torch.stack([sc[k] for sc in scenes]) for k in range(4))
    ext = torch.stack([torch.stack([look_at_camera(2 * i + j, jitter=0.1) for j in range(v)]) for i in range(b)]).cuda()
    K = default_K()[None, None].repeat(b, v, 1, 1).cuda()
    rot = torch.zeros(b, v, 3, device="cuda", requires_grad=True)
    tr = torch.zeros(b, v, 3, device="cuda", requires_grad=True)
    w, wd = torch.randn(b, v, 3, H, W, device="cuda"), torch.randn(b, v, H, W, device="cuda")
    g = Gaussians(means.cuda(), cov.cuda(), sh.cuda(), opac.cuda())
    out = SplattingCUDA().forward(g, ext, K, (H, W), cam_rot_delta=rot, cam_trans_delta=tr)
    ((out["render_color"] * w).sum() + (out["render_depth"] * wd).sum()).backward()
    assert rot.grad is not None and tr.grad is not None and float(rot.grad.abs().sum()) > 0
    for i in range(b):
        for j in range(v):
            r1 = torch.zeros(1, 3, device="cuda", requires_grad=True)
            t1 = torch.zeros(1, 3, device="cuda", requires_grad=True)
            img, dep = cs.render_cuda(ext[i, j][None], K[i, j][None], torch.tensor([1.0]), torch.tensor([1000.0]), (H, W), torch.zeros(1, 3),
                                      (means[i] * 10.0).cuda()[None], (cov[i] * 100.0).cuda()[None], sh[i].cuda()[None], opac[i].cuda()[None],
                                      cam_rot_delta=r1, cam_trans_delta=t1, translation_scale=10.0)
            assert torch.equal(img.detach().clamp(0.0, 1.0)[0], out["render_color"][i, j].detach())
            ((img.clamp(0.0, 1.0)[0] * w[i, j]).sum() + (dep[0] * wd[i, j]).sum()).backward()
            assert _rel(rot.grad[i, j], r1.grad[0]) < 1e-5 and _rel(tr.grad[i, j], t1.grad[0]) < 1e-5, (i, j)
