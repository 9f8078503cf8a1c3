"""csrc/density.hip on the GPU against tests/dense_density64.py (float64, written from the rules): statistics, plan, apply, and the
statistics through the real rasterizer backward.

Float32 bar (accumulate, split children): the float64 restatement is evaluated on the SAME float32 inputs upcast; the same restatement in
float32 runs on the CPU; the kernel's error against float64 may be at most 2 x that float32 error (another operation order), with a floor of
1e-6 -- the bar tests/test_photo_loss_gpu.py uses.  Integers, kept rows, cloned rows and moments are compared bit for bit."""
import math

import pytest
import torch

import dense_density64 as D
from scenes import default_K, look_at_camera, random_scene

pytestmark = pytest.mark.gpu

FIELDS = ("means", "scales", "rotations", "opacities", "harmonics")


def _stats(G, grad_accum=None, seen=None, max_radius=None):
    from siu3r_amd.density import DensityStats

    s = DensityStats(G, "cuda")
    for name, v in (("grad_accum", grad_accum), ("seen", seen), ("max_radius", max_radius)):
        if v is not None:
            getattr(s, name).copy_(v)
    return s


def _rel(x, ref):
    """largest elementwise relative error; where the reference is 0 the value must be 0 too"""
    x, ref = x.double().cpu(), ref.double().cpu()
    zero = ref == 0
    assert bool((x[zero] == 0).all())
    return float(((x - ref).abs()[~zero] / ref.abs()[~zero]).max()) if bool((~zero).any()) else 0.0


# ---- 1. statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,G", [(1, 10007), (6, 10007), (6, 1), (1, 255)])
def test_accumulate_against_float64(V, G):
    g = torch.Generator().manual_seed(V * 100 + G)
    g2d = torch.randn(V, G, 2, generator=g) * 1e-5
    radii = torch.randint(1, 60, (V, G, 2), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 4, (V, G), generator=g)
    radii[kind == 0] = 0          # culled: the gradient row is garbage
    radii[..., 0][kind == 1] = 0  # one positive radius is enough to count
    g2d[kind == 0] = float("nan")
    g2d[..., 1][(kind == 0) & (torch.rand(V, G, generator=g) < 0.5)] = 1e30
    acc0 = torch.rand(G, generator=g) * 1e-3
    seen0 = torch.randint(0, 5, (G,), generator=g, dtype=torch.int32)
    rad0 = torch.randint(0, 80, (G,), generator=g, dtype=torch.int32)
    sx, sy = V * 512 / 2, V * 384 / 2
    ref = D.accumulate(g2d, radii, sx, sy, acc0, seen0, rad0)
    cmp32 = D.accumulate(g2d, radii, sx, sy, acc0, seen0, rad0, dtype=torch.float32)
    outs = []
    for _ in range(2):
        s = _stats(G, acc0, seen0, rad0)
        s.accumulate(g2d.cuda(), radii.cuda(), sx, sy)
        outs.append(s)
    s = outs[0]
    assert torch.equal(s.seen.cpu().long(), ref[1]) and torch.equal(s.max_radius.cpu().long(), ref[2])
    assert bool(torch.isfinite(s.grad_accum).all())
    e_hip, e_32 = _rel(s.grad_accum, ref[0]), _rel(cmp32[0], ref[0])
    print(f"\naccumulate V={V} G={G}: float32 restatement (CPU) {e_32:.2e}, hip {e_hip:.2e} (largest relative error against float64)")
    assert e_hip <= max(2.0 * e_32, 1e-6)
    for a, b in zip((outs[0].grad_accum, outs[0].seen, outs[0].max_radius), (outs[1].grad_accum, outs[1].seen, outs[1].max_radius)):
        assert torch.equal(a, b)


# ---- 2. statistics through the real backward ----------------------------------------------------------------------------------------
H, W = 96, 128
NEAR, FAR = 0.5, 100.0


def _scene(G=20000, seed=0):
    means, cov, opac, sh = random_scene(G, seed=seed, n_sh=4)
    return means.cuda(), cov.cuda(), opac.cuda(), sh.cuda()


def _render_views(c2w, K, means, cov, opac, sh, **kw):
    from siu3r_amd.cuda_splatting import render_cuda

    V = c2w.shape[0]
    e = lambda x: x[None].expand(V, *x.shape)
    return render_cuda(c2w, K, torch.full((V,), NEAR), torch.full((V,), FAR), (H, W), torch.zeros(V, 3), e(means), e(cov), e(sh), e(opac), **kw)


def _single_view_norms(c2w, K, means, cov, opac, sh, targets):
    """per view: one single-view render with the means2d holder, loss = the mean over THAT view; the NDC norms hypot(W/2 gx, H/2 gy)
    in torch (float32, added in view order: the arithmetic the kernel does, so that what differs is the backward itself), summed over
    the views that see the Gaussian -> [G], and the radii [V,G,2]"""
    from siu3r_amd import raster

    G = means.shape[0]
    total = torch.zeros(G, dtype=torch.float32, device="cuda")
    radii = []
    for v in range(c2w.shape[0]):
        cam = raster.make_cam_k2(None, None, None, None, None, [0.0, 0.0, 0.0], W, H, sh_degree=1, near=NEAR, far=FAR)
        hold = torch.zeros(G, 2, device="cuda", requires_grad=True)
        o = raster.rasterize_views_k2([cam], means, cov, sh.permute(0, 2, 1).contiguous(), opac, pose_c2w=(c2w[v:v + 1], K[v:v + 1], 1.0), means2d=hold)
        ((o["image"] - targets[v:v + 1]) ** 2).mean().backward()
        vis = (o["radii"][0] > 0).any(-1)
        norm = torch.hypot(hold.grad[:, 0] * (W / 2), hold.grad[:, 1] * (H / 2))
        total = torch.where(vis, total + norm, total)
        radii.append(o["radii"])
    return total.double(), torch.cat(radii)


def test_accumulate_through_the_rasterizer_backward():
    """A 4-view render_cuda with a holder against 4 single-view renders with the means2d holder.  The loss of the multi-view call is the
    mean over all views, so its per-view gradient is 1 / V of the single-view one, which the statistics' factor V undoes (V = 4: both
    scalings are exact).  What is left is the order of the composite backward's float atomics.  Bar, as the issue sets it: the spread
    between two repeated runs of the single-view passes on this board (largest difference of the summed norms, normalised by the
    largest norm) times 4 for the different summation.  Gradients of two backward runs are not the same bits for the same reason, so
    the comparison of `density_stats=None` with the call without the keyword demands torch.equal of every forward output and, for the
    gradients, at most 4 x the spread of two runs WITHOUT the keyword (the same factor, the same cause)."""
    from siu3r_amd.density import DensityStats

    V = 4
    means, cov, opac, sh = _scene()
    G = means.shape[0]
    c2w = torch.stack([look_at_camera(seed=s) for s in range(V)]).cuda()
    K = default_K()[None].repeat(V, 1, 1).cuda()
    targets = torch.rand(V, 3, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    a, radii = _single_view_norms(c2w, K, means, cov, opac, sh, targets)
    b, _ = _single_view_norms(c2w, K, means, cov, opac, sh, targets)
    top = float(a.max())
    spread = float((a - b).abs().max()) / top

    def run(**kw):
        leaves = [t.clone().requires_grad_(True) for t in (means, cov, opac, sh)]
        img, depth = _render_views(c2w, K, *leaves, **kw)
        ((img - targets) ** 2).mean().backward()
        return img.detach(), depth.detach(), [t.grad for t in leaves]

    stats = DensityStats(G, "cuda")
    img_s, depth_s, grads_s = run(density_stats=stats)
    err = float((stats.grad_accum.double() - a).abs().max()) / top
    print(f"\nstatistics through the backward, {V} views {H}x{W}, {G} Gaussians: spread of two single-view runs {spread:.3e}, bar 4 x = {4 * spread:.3e}, "
          f"holder against the single-view sum {err:.3e} (normalised by the largest norm {top:.3e})")
    vis = (radii > 0).any(-1)
    assert torch.equal(stats.seen.long(), vis.sum(0))
    assert torch.equal(stats.max_radius, torch.where(vis[..., None], radii, torch.zeros_like(radii)).amax((0, 2)))
    assert bool((vis.sum(0) > 1).any()) and bool((~vis).any())  # seen by several views, and some culled
    assert err <= 4 * spread
    # a second backward adds on top
    run(density_stats=stats)
    assert torch.equal(stats.seen.long(), 2 * vis.sum(0))
    # None = no keyword = the holder's forward, bit for bit; the gradients up to the atomics' run-to-run spread
    img_0, depth_0, grads_0 = run()
    img_1, depth_1, grads_1 = run()
    img_n, depth_n, grads_n = run(density_stats=None)
    for x in (img_1, img_n, img_s):
        assert torch.equal(x, img_0)
    for x in (depth_1, depth_n, depth_s):
        assert torch.equal(x, depth_0)
    for name, g0, g1, gn, gs in zip(("means", "cov", "opac", "sh"), grads_0, grads_1, grads_n, grads_s):
        repeat = float((g0 - g1).abs().max())
        print(f"  grad {name}: two runs without the keyword differ by {repeat:.3e}, None by {float((gn - g0).abs().max()):.3e}, "
              f"with a holder by {float((gs - g0).abs().max()):.3e} (max |grad| {float(g0.abs().max()):.3e})")
        assert float((gn - g0).abs().max()) <= 4 * repeat and float((gs - g0).abs().max()) <= 4 * repeat


# ---- 3. plan ------------------------------------------------------------------------------------------------------------------------
def _random_plan_inputs(G, seed):
    g = torch.Generator().manual_seed(seed)
    seen = torch.randint(0, 7, (G,), generator=g, dtype=torch.int32)
    grad_accum = torch.rand(G, generator=g) * seen * 4e-4  # averages uniform in [0, 4e-4] around the 2e-4 threshold
    grad_accum[seen == 0] = 1.0  # never seen: whatever the sum holds, it does not densify
    max_radius = torch.randint(0, 60, (G,), generator=g, dtype=torch.int32)
    log_scales = torch.randn(G, 3, generator=g) - 3.5
    logit_op = torch.randn(G, generator=g) * 4
    return grad_accum, seen, max_radius, log_scales, logit_op


def _check_plan(inputs, thr, grow=True):
    from siu3r_amd import density

    ga, seen, rad, ls, lo = inputs
    G = ga.shape[0]
    ref_a, ref_o, ref_t = D.plan(ga, seen, rad, ls, lo, grow=grow, **thr)
    outs = []
    for _ in range(2):
        a, o, t = density.plan(_stats(G, ga, seen, rad), ls.cuda(), lo.cuda(), grow=grow, **thr)
        outs.append((a, o, t))
    a, o, t = outs[0]
    assert a.dtype == torch.int32 and o.dtype == torch.int32
    assert torch.equal(a.cpu().long(), ref_a), "actions"
    assert torch.equal(o.cpu().long(), ref_o), "offsets"
    assert tuple(t.tolist()) == ref_t, (t.tolist(), ref_t)
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    return ref_a, ref_t


@pytest.mark.parametrize("G", [1, 255, 100003, 2100000])
@pytest.mark.parametrize("rules", ["default", "all"])
def test_plan_random_inputs_are_bit_exact(G, rules):
    from siu3r_amd.density import DensityControl

    c = DensityControl() if rules == "default" else DensityControl(max_screen_radius=40, max_world_scale_frac=0.02)
    thr = c.thresholds(5.0)
    inputs = _random_plan_inputs(G, seed=G + len(rules))
    ref_a, tot = _check_plan(inputs, thr)
    print(f"\nplan G={G} ({rules}): rows out {tot[0]}, pruned {tot[1]}, cloned {tot[2]}, split {tot[3]}")
    if G > 1000:
        assert min(tot) > 0  # every action occurs
    _, tot0 = _check_plan(inputs, thr, grow=False)
    assert tot0 == (G - tot[1], tot[1], 0, 0)


def test_plan_on_threshold_rows():
    thr = dict(grad_threshold=0.25, log_dense_scale=-2.0, logit_min_opacity=-5.0)
    f = lambda v, to: float(torch.nextafter(torch.tensor(v), torch.tensor(to)))
    # (grad_accum, seen, max_radius, top log-scale, logit opacity) -> action
    rows = [((0.5, 2, 0, -3.0, 0.0), D.CLONE), ((f(0.5, 0.0), 2, 0, -3.0, 0.0), D.KEEP),        # >= for the gradient
            ((0.75, 3, 0, -3.0, 0.0), D.CLONE), ((f(0.75, 0.0), 3, 0, -3.0, 0.0), D.KEEP),
            ((1.0, 1, 0, -2.0, 0.0), D.CLONE), ((1.0, 1, 0, f(-2.0, 0.0), 0.0), D.SPLIT),           # > for the scale
            ((0.0, 1, 0, -3.0, -5.0), D.KEEP), ((0.0, 1, 0, -3.0, f(-5.0, -10.0)), D.PRUNE),        # < for the opacity
            ((9.0, 0, 0, -1.5, 0.0), D.KEEP),                                                       # never seen
            ((9.0, 3, 0, -1.5, -9.0), D.PRUNE), ((9.0, 3, 0, -3.0, -9.0), D.PRUNE),                # a prune wins
            ((0.0, 1, 20, -3.0, 0.0), D.KEEP), ((0.0, 1, 21, -3.0, 0.0), D.PRUNE),                  # > for the screen radius
            ((0.0, 1, 0, -1.0, 0.0), D.KEEP), ((0.0, 1, 0, f(-1.0, 0.0), 0.0), D.PRUNE)]            # > for the world scale
    t = torch.tensor([r for r, _ in rows], dtype=torch.float64)
    ls = torch.stack((t[:, 3] - 1.0, t[:, 3], t[:, 3] - 0.5), -1).float()
    inputs = (t[:, 0].float(), t[:, 1].int(), t[:, 2].int(), ls, t[:, 4].float())
    ref_a, _ = _check_plan(inputs, dict(thr, max_screen_radius=20, log_max_world_scale=-1.0))
    assert ref_a.tolist() == [a for _, a in rows]
    ref_a, _ = _check_plan(inputs, thr)  # the two optional rules off
    assert ref_a.tolist()[-4:] == [D.KEEP] * 4
    _check_plan(inputs, dict(thr, max_screen_radius=20, log_max_world_scale=-1.0), grow=False)


# ---- 4. apply -----------------------------------------------------------------------------------------------------------------------
def _params(G, n_sh, seed, frozen=("rotations",)):
    g = torch.Generator().manual_seed(seed)
    p = dict(means=torch.randn(G, 3, generator=g) * 2, scales=torch.log(0.01 + 0.3 * torch.rand(G, 3, generator=g)),
             rotations=torch.randn(G, 4, generator=g) * (0.5 + torch.rand(G, 1, generator=g)), opacities=torch.randn(G, generator=g) * 3,
             harmonics=torch.randn(G, 3, n_sh, generator=g))
    m = {k: (torch.randn(p[k].shape, generator=g), torch.rand(p[k].shape, generator=g) + 0.1) for k in FIELDS if k not in frozen}
    noise = torch.randn(G, 2, 3, generator=g)
    return p, m, noise


def _cuda(d):
    return {k: (tuple(x.cuda() for x in v) if isinstance(v, tuple) else v.cuda()) for k, v in d.items()}


@pytest.mark.parametrize("n_sh", [4, 25])  # rows of 3, 3, 4, 1 and 12 / 75 floats
def test_apply_against_float64(n_sh):
    from siu3r_amd import density

    G = 10007
    p, m, noise = _params(G, n_sh, seed=n_sh)
    ga, seen, rad, _, _ = _random_plan_inputs(G, seed=7)
    thr = dict(grad_threshold=2e-4, log_dense_scale=math.log(0.2), logit_min_opacity=-3.0)
    action, offset, totals = density.plan(_stats(G, ga, seen, rad), p["scales"].cuda(), p["opacities"].cuda(), **thr)
    rows_out, pruned, cloned, split = totals.tolist()
    assert min(rows_out, pruned, cloned, split, G - pruned - cloned - split) > 500
    outs = [density.apply(_cuda(p), _cuda(m), action, offset, rows_out, noise.cuda()) for _ in range(2)]
    new_p, new_m = outs[0]
    a, o = action.cpu().long(), offset.cpu().long()
    ref_p, _ = D.apply(p, m, a, o, rows_out, noise)
    c32_p, _ = D.apply(p, m, a, o, rows_out, noise, dtype=torch.float32)
    keep, clone, spl = a == D.KEEP, a == D.CLONE, a == D.SPLIT
    assert set(new_m) == set(m) and "rotations" not in new_m
    for k in FIELDS:
        x = new_p[k].cpu()
        assert x.shape == (rows_out, *p[k].shape[1:]) and x.dtype == torch.float32
        assert torch.equal(x[o[keep]], p[k][keep]), f"{k}: kept rows"
        assert torch.equal(x[o[clone]], p[k][clone]) and torch.equal(x[o[clone] + 1], p[k][clone]), f"{k}: cloned rows"
        if k not in ("means", "scales"):
            assert torch.equal(x[o[spl]], p[k][spl]) and torch.equal(x[o[spl] + 1], p[k][spl]), f"{k}: split rows copy the parent"
        if k in m:
            for j in range(2):
                y = new_m[k][j].cpu()
                assert torch.equal(y[o[keep]], m[k][j][keep]) and torch.equal(y[o[clone]], m[k][j][clone]), f"{k}: moments of the originals"
                assert not bool(y[o[clone] + 1].any()) and not bool(y[o[spl]].any()) and not bool(y[o[spl] + 1].any()), f"{k}: moments of new rows"
    # split children against float64, in units of the parent's largest scale (log-scales: absolute = relative in the scale)
    kids = torch.cat((o[spl], o[spl] + 1))
    unit = p["scales"].double().exp().max(-1).values[spl].repeat(2)[:, None]
    err = lambda x, k: float(((x[k].cpu().double()[kids] - ref_p[k][kids]).abs() / (unit if k == "means" else 1.0)).max())
    for k in ("means", "scales"):
        e_hip, e_32 = err(new_p, k), err(c32_p, k)
        print(f"\napply n_sh={n_sh}: split children's {k}: float32 restatement (CPU) {e_32:.2e}, hip {e_hip:.2e}")
        assert e_hip <= max(2.0 * e_32, 1e-6)
    moved = (new_p["means"].cpu()[kids] - p["means"][spl].repeat(2, 1)).norm(dim=-1)
    assert float(moved.min()) > 0
    for k in FIELDS:
        assert torch.equal(outs[0][0][k], outs[1][0][k])
        if k in m:
            assert torch.equal(outs[0][1][k][0], outs[1][1][k][0]) and torch.equal(outs[0][1][k][1], outs[1][1][k][1])


def test_all_keep_plan_returns_every_tensor_bit_identical():
    from siu3r_amd import density

    G = 70001
    p, m, noise = _params(G, 25, seed=3)
    p["opacities"] = p["opacities"].abs()
    action, offset, totals = density.plan(_stats(G), p["scales"].cuda(), p["opacities"].cuda(), grad_threshold=2e-4, log_dense_scale=-4.0, logit_min_opacity=-5.0)
    assert totals.tolist() == [G, 0, 0, 0] and bool((action == D.KEEP).all()) and torch.equal(offset.cpu().long(), torch.arange(G))
    new_p, new_m = density.apply(_cuda(p), _cuda(m), action, offset, G, noise.cuda())
    for k in FIELDS:
        assert torch.equal(new_p[k].cpu(), p[k])
        if k in m:
            assert torch.equal(new_m[k][0].cpu(), m[k][0]) and torch.equal(new_m[k][1].cpu(), m[k][1])


def test_split_children_have_the_parents_covariance():
    """25,000 copies of one anisotropic Gaussian, all split: N = 50,000 offsets d = child mean - parent mean, which the rule draws from
    N(0, Sigma), Sigma = R diag(s^2) R^T.  The offsets have a known zero mean, so C = sum d d^T / N estimates Sigma with
    Var(C_ij) = (Sigma_ii Sigma_jj + Sigma_ij^2) / N (Isserlis), and the sample mean has Var(mean_i) = Sigma_ii / N.  Bar: 5 standard
    errors per entry (nine entries and three means: a chance of 12 x 5.7e-7 of a false alarm with honest normals, and the noise is
    seeded), plus 1e-6 of the largest entry for the float32 rounding of mean + offset."""
    from siu3r_amd import density

    N = 25000
    s = torch.tensor([0.5, 0.1, 0.02])
    q = torch.tensor([0.3, -0.5, 0.2, 0.8]) * 1.7
    mean = torch.tensor([1.0, -2.0, 3.0])
    p = dict(means=mean.repeat(N, 1), scales=s.log().repeat(N, 1), rotations=q.repeat(N, 1), opacities=torch.zeros(N), harmonics=torch.zeros(N, 3, 1))
    noise = torch.randn(N, 2, 3, generator=torch.Generator().manual_seed(11))
    stats = _stats(N, torch.ones(N), torch.ones(N, dtype=torch.int32))
    action, offset, totals = density.plan(stats, p["scales"].cuda(), p["opacities"].cuda(), grad_threshold=2e-4, log_dense_scale=-3.0, logit_min_opacity=-5.0)
    assert totals.tolist() == [2 * N, 0, 0, N]
    new_p, _ = density.apply(_cuda(p), {}, action, offset, 2 * N, noise.cuda())
    d = new_p["means"].cpu().double() - mean.double()
    n = d.shape[0]
    assert n == 50000
    R = D.rotation(q.double()[None])[0]
    sigma = R @ torch.diag(s.double() ** 2) @ R.T
    C = d.T @ d / n
    se = ((sigma.diag()[:, None] * sigma.diag()[None, :] + sigma ** 2) / n).sqrt()
    z = (C - sigma).abs() / se
    zm = d.mean(0).abs() / (sigma.diag() / n).sqrt()
    print(f"\n{n} split children: covariance off by at most {float(z.max()):.2f} standard errors, the mean by {float(zm.max()):.2f}")
    assert bool(((C - sigma).abs() <= 5.0 * se + 1e-6 * sigma.abs().max()).all()) and float(zm.max()) <= 5.0 + 1e-3
    assert torch.allclose(new_p["scales"].cpu().double().exp(), (s.double() / 1.6).expand(n, 3), rtol=1e-6)


# ---- 5. densify_and_prune -----------------------------------------------------------------------------------------------------------
def test_densify_and_prune_cap_and_frozen_fields():
    from siu3r_amd import density

    G = 30011
    p, m, noise = _params(G, 4, seed=9, frozen=("rotations", "means"))
    ga, seen, rad, _, _ = _random_plan_inputs(G, seed=13)
    control = density.DensityControl(percent_dense=0.01, min_opacity=0.05)
    extent = 12.0
    thr = control.thresholds(extent)
    ref_a, ref_o, ref_t = D.plan(ga, seen, rad, p["scales"], p["opacities"], **thr)
    new_p, new_m, info = density.densify_and_prune(_cuda(p), _cuda(m), _stats(G, ga, seen, rad), control, extent, noise.cuda())
    assert info == dict(rows_in=G, rows_out=ref_t[0], pruned=ref_t[1], kept=G - ref_t[1] - ref_t[2] - ref_t[3], cloned=ref_t[2], split=ref_t[3], capped=False)
    assert ref_t[0] > G and min(ref_t) > 0 and new_p["means"].shape[0] == ref_t[0]
    keep = ref_a == D.KEEP
    for k in ("rotations", "means"):  # frozen: no moments, kept rows are the source's bits
        assert k not in new_m and torch.equal(new_p[k].cpu()[ref_o[keep]], p[k][keep])
    # a cap below the planned size: the event only prunes, and says so
    capped = density.DensityControl(percent_dense=0.01, min_opacity=0.05, max_gaussians=ref_t[0] - 1)
    cp, cm, cinfo = density.densify_and_prune(_cuda(p), _cuda(m), _stats(G, ga, seen, rad), capped, extent, noise.cuda())
    a0, o0, t0 = D.plan(ga, seen, rad, p["scales"], p["opacities"], grow=False, **thr)
    assert cinfo == dict(rows_in=G, rows_out=G - ref_t[1], pruned=ref_t[1], kept=G - ref_t[1], cloned=0, split=0, capped=True) and t0[0] == G - ref_t[1]
    alive = a0 == D.KEEP
    for k in FIELDS:
        assert torch.equal(cp[k].cpu(), p[k][alive]), f"{k}: a prune-only event is an order-preserving compaction"
        if k in m:
            assert torch.equal(cm[k][0].cpu(), m[k][0][alive]) and torch.equal(cm[k][1].cpu(), m[k][1][alive])
    # a cap that is not hit changes nothing
    roomy = density.DensityControl(percent_dense=0.01, min_opacity=0.05, max_gaussians=ref_t[0])
    rp, _, rinfo = density.densify_and_prune(_cuda(p), _cuda(m), _stats(G, ga, seen, rad), roomy, extent, noise.cuda())
    assert rinfo == info and all(torch.equal(rp[k], new_p[k]) for k in FIELDS)
