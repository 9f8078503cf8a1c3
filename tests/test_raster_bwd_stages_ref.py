"""CPU proofs of tests/dense_raster_bwd64.py, the float64 reference that tests/test_raster_bwd_stages_gpu.py holds every stage of the two
rasterizer backward passes to:

  (a) the references are right: they agree with central differences of the float64 forward on rows of every branch, and the composite
      reference pulled back through project_bwd64 reproduces torch.autograd.grad of dense_raster64.render / dense_gsplat64.render;
  (b) the metric rejects wrong answers: at every case shape, answers with one branch wrong (the Jacobian clamp, the alpha_max clamp or the
      colour clamp passing gradient, limx / limy or lim*_pos / lim*_neg swapped, an SH basis constant of each band off in its fourth digit,
      a dropped term, < against <= at t_min) fail assert_elems_close with the derived bounds;
  (c) every crafted case populates the branches it is for, the derived constants hold (exp_det_sel, the margin: above it the float32
      walk takes the float64 branch at every pixel) and at most 1 % of a case's pixels lie below the margin."""
import copy

import numpy as np
import pytest
import torch

import dense_gsplat64 as DG
import dense_raster64 as DR
import dense_raster_bwd64 as B

DD = torch.float64
PROJ_OUT = ("g_means", "g_cov", "g_opac", "g_colors", "pose")


# ---- (a) the references are right ---------------------------------------------------------------------------------------------------------
def _objective(c, v, leaves, pose):
    """sum over the live Gaussians of view v of <grad, record>"""
    rec, _ = B.project64(c["mode"], c["cams"][v], leaves[0], leaves[1], leaves[2], leaves[3] if c["colors"] is not None else None, pose)
    r = c["rect"][v].long()
    live = ((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]) != 0).to(DD)
    n = 10 if c["mode"] == 0 else 9
    return (rec[:, :n] * c["grad"][v, :, :n].to(DD) * live[:, None]).sum()


@pytest.mark.parametrize("name", ["k2_deg3", "k2_deg4_band4", "k2_precomputed", "k3_two"])
def test_projection_reference_matches_central_differences(name):
    """directional derivatives over the rows of one clamp class at a time (six Gaussians per class), every input and the pose"""
    c, ref = B.proj_case(name), B.proj_ref(name)
    cls, _ = B.clamp_class(ref["aux"][0])
    gen = torch.Generator().manual_seed(3)
    base = [c["means"].to(DD), c["cov6"].to(DD), c["opac"].to(DD)] + ([c["colors"].to(DD)] if c["colors"] is not None else [])
    names = ["g_means", "g_cov", "g_opac", "g_colors"]
    for k in range(6):
        rows = torch.nonzero(cls == k).flatten()[:6]
        for i, x in enumerate(base):
            d = torch.zeros_like(x)
            d[rows] = torch.randn(d[rows].shape, generator=gen, dtype=DD)
            want = float((ref[names[i]][0] * d).sum())
            h = 1e-6
            fd = 0.0
            for v in range(c["V"]):
                fp = _objective(c, v, [b + h * d if j == i else b for j, b in enumerate(base)], None)
                fm = _objective(c, v, [b - h * d if j == i else b for j, b in enumerate(base)], None)
                fd += float(fp - fm) / (2 * h)
            scale = float((ref[names[i]][1] * d.abs()).sum()) + 1e-30
            assert abs(fd - want) <= 1e-6 * scale, (name, k, names[i], fd, want)
    for v in range(c["V"]):  # the pose: mode 0 (rho, theta) of the left perturbation, mode 1 the entries of [R | t]
        got, S = ref["pose"][0][v], ref["pose"][1][v]
        if c["mode"] == 0:
            for j in range(6):
                e = torch.zeros(6, dtype=DD)
                e[j] = 1e-6
                fd = float(_objective(c, v, base, e) - _objective(c, v, base, -e)) / 2e-6
                assert abs(fd - float(got[j])) <= 1e-6 * float(S[j]), (name, v, j, fd, float(got[j]))
        else:
            vm = DG.cam_w2c(c["cams"][v])
            for j in range(12):
                e = torch.zeros(4, 4, dtype=DD)
                e[j // 4, j % 4] = 1e-6
                fd = float(_objective(c, v, base, vm + e) - _objective(c, v, base, vm - e)) / 2e-6
                assert abs(fd - float(got[j // 4, j % 4])) <= 1e-6 * float(S[j // 4, j % 4]), (name, v, j)
            assert float(got[3].abs().max()) == 0.0 and float(S[3].abs().max()) == 0.0


def test_mode1_projection_is_dense_gsplat64_project():
    c = B.proj_case("k3_two")
    for cam in c["cams"]:
        rec, _ = B.project64(1, cam, c["means"], c["cov6"], c["opac"], c["colors"])
        want = DG.project(cam, c["means"], c["cov6"])
        for k, w in zip((B.MX, B.MY, B.CA, B.CB, B.CC, B.ZZ), want):
            assert float((rec[:, k] - w).abs().max()) <= 1e-12 * float(w.abs().max())


def _all_lists(cam, depth32):
    """every Gaussian on every tile, front to back by (fp32 depth key, index)"""
    T = (-(-cam.width // 16)) * (-(-cam.height // 16))
    order = np.array(sorted(range(len(depth32)), key=lambda i: (depth32[i], i)), np.int32)
    return np.arange(T + 1) * len(order), np.tile(order, T)


def _rec12(rec10):
    r = np.zeros((rec10.shape[0], 12))
    r[:, 0], r[:, 1], r[:, 2], r[:, 4:8], r[:, 8:11] = rec10[:, B.MX], rec10[:, B.MY], rec10[:, B.ZZ], rec10[:, B.CA:B.OP + 1], rec10[:, B.RR:B.BB + 1]
    return r


def test_composite_and_projection_reference_reproduce_autograd_of_the_k2_render():
    c = B.proj_case("k2_deg2_wide")
    cam, G = c["cams"][0], c["G"]
    H, W = cam.height, cam.width
    leaves = [t.to(DD).requires_grad_() for t in (c["means"], c["cov6"], c["colors"], c["opac"])]
    xi = torch.zeros(6, dtype=DD, requires_grad=True)
    with torch.no_grad():
        rec10, _ = B.project64(0, cam, c["means"], c["cov6"], c["opac"], c["colors"])
    key = rec10[:, B.ZZ].float()
    mask = torch.ones((G, (-(-W // 16)) * (-(-H // 16))), dtype=torch.bool)
    gen = torch.Generator().manual_seed(5)
    g_img, g_d, g_a = (torch.randn(s, generator=gen, dtype=DD) for s in ((3, H, W), (H, W), (H, W)))
    img, dep, alp = DR.render(cam, leaves[0], leaves[1], leaves[2], leaves[3], mask, xi=xi, depth_key=key)
    want = torch.autograd.grad((img * g_img).sum() + (dep * g_d).sum() + (alp * g_a).sum(), leaves + [xi])
    comp = B.composite_bwd64("k2", cam, _rec12(rec10.numpy()), _all_lists(cam, key.numpy()), g_img.numpy(), g_a.numpy(), g_d.numpy())
    assert comp["counts"]["blend"] > 2000
    for got, ref in ((comp["out"], img), (comp["depth"], dep), (comp["alpha"], alp)):
        assert float((torch.from_numpy(got) - ref.detach()).abs().max()) <= 1e-12
    rect = torch.ones((1, G, 4), dtype=torch.int32) * torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    pb = B.project_bwd64(0, [cam], c["means"], c["cov6"], c["opac"], c["colors"], rect, comp["grad"][None])
    for n, w in zip(("g_means", "g_cov", "g_colors", "g_opac"), want):
        assert float((pb[n][0] - w).abs().max()) <= 1e-9 * float(w.abs().max()), n
    assert float((pb["pose"][0][0] - want[4]).abs().max()) <= 1e-9 * float(want[4].abs().max())


def test_composite_and_projection_reference_reproduce_autograd_of_the_k3_render():
    c = B.proj_case("k3_two")
    cam, G, C = copy.copy(c["cams"][0]), c["G"], 5
    cam.alpha_max = 0.6  # (many alphas on the clamp)
    H, W = cam.height, cam.width
    gen = torch.Generator().manual_seed(7)
    feats = torch.randn(G, C, generator=gen, dtype=DD)
    opac = c["opac"].to(DD).clone()
    leaves = [t.to(DD).clone().requires_grad_() for t in (c["means"], c["cov6"], feats, opac)]
    vm = DG.cam_w2c(cam).requires_grad_()
    with torch.no_grad():
        rec10, _ = B.project64(1, cam, c["means"], c["cov6"], opac, None)
    key = rec10[:, B.ZZ].float()
    mask = torch.ones((G, (-(-W // 16)) * (-(-H // 16))), dtype=torch.bool)
    g_out, g_a = torch.randn(H, W, C, generator=gen, dtype=DD), torch.randn(H, W, generator=gen, dtype=DD)
    col, alp = DG.render(cam, leaves[0], leaves[1], leaves[2], leaves[3], mask, viewmat=vm, depth_key=key)
    want = torch.autograd.grad((col * g_out).sum() + (alp * g_a).sum(), leaves + [vm])
    comp = B.composite_bwd64("feat", cam, _rec12(rec10.numpy()), _all_lists(cam, key.numpy()), g_out.numpy(), g_a.numpy(), feats=feats.numpy())
    assert comp["counts"]["blend"] > 2000 and comp["counts"]["clamped"] > 0
    assert float((torch.from_numpy(comp["out"]) - col.detach()).abs().max()) <= 1e-12
    assert float((torch.from_numpy(comp["g_feats"]) - want[2]).abs().max()) <= 1e-9 * float(want[2].abs().max())
    rect = torch.ones((1, G, 4), dtype=torch.int32) * torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    pb = B.project_bwd64(1, [cam], c["means"], c["cov6"], opac, None, rect, comp["grad"][None])
    for n, w in zip(("g_means", "g_cov", "g_opac"), (want[0], want[1], want[3])):
        assert float((pb[n][0] - w).abs().max()) <= 1e-9 * float(w.abs().max()), n
    assert float((pb["pose"][0][0] - want[4]).abs().max()) <= 1e-9 * float(want[4].abs().max())


@pytest.mark.parametrize("name", ["k2_small", "k3_small", "feat_c5"])
def test_composite_reference_matches_central_differences_of_its_own_forward(name):
    """d (sum of the outputs against the upstream gradients) / d (record entry) for Gaussians of every group: a blended one with the
    alpha_max clamp on some pixels, one of an opaque stack, one with an indefinite conic, Gaussian 0"""
    c = B.comp_case(name)
    refs, ups = B.comp_ref(c)
    r0, cam, kind = refs[0], c["cams"][0], c["kind"]
    both = np.flatnonzero((r0["hit_clamped"] > 0) & (r0["hit_free"] > 0))
    rec = c["rec"][0].astype(np.float64)
    indefinite = np.flatnonzero(rec[:, 4] * rec[:, 6] - rec[:, 5] ** 2 < 0)
    rows = [0, int(both[0]), int(indefinite[0]), int(np.argmax(r0["n_add"]))]

    def f(rc):
        o = B.composite_bwd64(kind, cam, rc, c["lists"][0], ups["g_out"][0], ups["g_alpha"][0], ups["g_depth"][0], c["feats"])
        return float((o["out"] * ups["g_out"][0]).sum() + (o["alpha"] * ups["g_alpha"][0]).sum() + (o["depth"] * ups["g_depth"][0]).sum() if kind == "k2"
                     else (o["out"] * ups["g_out"][0]).sum() + (o["alpha"] * ups["g_alpha"][0]).sum())

    slot_of = {B.MX: 0, B.MY: 1, B.CA: 4, B.CB: 5, B.CC: 6, B.OP: 7, B.RR: 8, B.GG: 9, B.BB: 10, B.ZZ: 2}
    for g in rows:
        for k in (B.MX, B.CB, B.OP) + ((B.GG, B.ZZ) if kind == "k2" else (B.GG,) if kind == "k3" else ()):
            h = 1e-7 * max(1.0, abs(rec[g, slot_of[k]]))
            rp, rm = rec.copy(), rec.copy()
            rp[g, slot_of[k]] += h
            rm[g, slot_of[k]] -= h
            fd = (f(rp) - f(rm)) / (2 * h)
            # (the objective is piecewise smooth: the step stays far inside the margin of all but a few pixels, whose jumps are of the
            # size of one pixel's term)
            assert abs(fd - r0["grad"][g, k]) <= 2e-5 * r0["S"][g, k] + 1e-12, (name, g, k, fd, r0["grad"][g, k])


def test_viewer_helper_references_match_central_differences():
    gen = torch.Generator().manual_seed(11)
    q, s, g6 = torch.randn(7, 4, generator=gen, dtype=DD), torch.rand(7, 3, generator=gen, dtype=DD) + 0.2, torch.randn(7, 6, generator=gen, dtype=DD)
    (gq, _), (gs, _) = B.quat_scale_cov6_bwd64(q, s, g6)
    f = lambda q_, s_: float((DG.quat_scale_to_cov6(q_, s_) * g6).sum())
    for x, gx, i in ((q, gq, 0), (s, gs, 1)):
        d = torch.randn(x.shape, generator=gen, dtype=DD)
        fd = (f(*(x + 1e-6 * d if j == i else y for j, y in enumerate((q, s)))) - f(*(x - 1e-6 * d if j == i else y for j, y in enumerate((q, s))))) / 2e-6
        assert abs(fd - float((gx * d).sum())) <= 1e-7 * float((gx * d).abs().sum())
    m, cp, sh, g3 = torch.randn(9, 3, generator=gen, dtype=DD), torch.tensor([0.1, -0.2, 3.0], dtype=DD), torch.randn(9, 25, 3, generator=gen, dtype=DD) * 0.3, torch.randn(9, 3, generator=gen, dtype=DD)
    sh[::3, 0, :2] = -6.0  # two channels clamped at 0 on every third row
    for deg in range(5):
        (gsh, _), (gm, _), (gc, _), lin = B.sh_eval_bwd64(m, cp, sh, deg, g3)
        assert float(lin.abs().min()) > 1e-4 and (lin < 0).any() and (lin > 0).any()
        assert float(gsh[:, (deg + 1) ** 2:].abs().max()) == 0.0 if deg < 4 else True
        f = lambda m_, c_, s_: float((DG.sh_eval(m_, c_, s_, deg) * g3).sum())
        for i, (x, gx) in enumerate(((m, gm), (cp, gc), (sh, gsh))):
            d = torch.randn(x.shape, generator=gen, dtype=DD)
            args = lambda sg: [x + sg * 1e-6 * d if j == i else y for j, y in enumerate((m, cp, sh))]
            fd = (f(*args(1)) - f(*args(-1))) / 2e-6
            assert abs(fd - float((gx * d).sum())) <= 1e-6 * float((gx * d).abs().sum()), (deg, i)


# ---- (b) the metric rejects wrong answers -------------------------------------------------------------------------------------------------
def _proj_rejected(c, ref, mutate):
    bad = B.project_bwd64(c["mode"], c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], c["rect"], c["grad"], mutate)
    return any(B.rejects(bad[n][0], ref[n][0], ref[n][1], B.PROJ_BOUND) for n in PROJ_OUT if n in ref)


@pytest.mark.parametrize("name", list(B.PROJ_CASES))
def test_projection_metric_rejects_wrong_answers(name):
    c, ref = B.proj_case(name), B.proj_ref(name)
    for n in PROJ_OUT:  # the reference passes its own metric, and a copy rounded to fp32 (what a perfect kernel would store) does too
        if n in ref:
            assert not B.rejects(ref[n][0], ref[n][0], ref[n][1], B.PROJ_BOUND)
    assert _proj_rejected(c, ref, dict(clamp_through=True)), "the Jacobian clamp passing gradient"
    assert _proj_rejected(c, ref, dict(swap_xy=True)), "limx / limy swapped"
    if c["mode"] == 1:
        assert _proj_rejected(c, ref, dict(swap_posneg=True)), "lim*_pos / lim*_neg swapped"
    if c["mode"] == 0 and c["deg"] >= 0:
        assert _proj_rejected(c, ref, dict(colour_through=True)), "the colour clamp passing gradient"
        for band, k in enumerate((0, 2, 6, 12, 20)):
            if band <= c["deg"] and (band < 4 or c["cams"][0].sh_band4):
                assert _proj_rejected(c, ref, dict(sh_scale={k: 5e-4})), f"SH constant of band {band} off in its fourth digit"
    for n in ("g_means", "g_cov", "g_opac"):  # one term of one Gaussian dropped: the smallest view's contribution of the last live row
        r = c["rect"].long()
        live = ((r[..., 2] - r[..., 0]) * (r[..., 3] - r[..., 1]) != 0)
        g = int(torch.nonzero(live.any(0)).flatten()[-1])
        v = int(torch.nonzero(live[:, g]).flatten()[0])
        grad2 = c["grad"].clone()
        grad2[v, g, B.OP if n == "g_opac" else B.CA if n == "g_cov" else B.MX] = 0
        bad = B.project_bwd64(c["mode"], c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], c["rect"], grad2)
        assert B.rejects(bad[n][0], ref[n][0], ref[n][1], B.PROJ_BOUND), f"{n}: a dropped term"


@pytest.mark.parametrize("name", list(B.COMP_CASES))
def test_composite_metric_rejects_wrong_answers(name):
    """the alpha_max clamp passing gradient; and one record term dropped, for EVERY non-zero element in turn: the share of elements that
    can be replaced by 0 unnoticed.  Such elements exist under any bound of this form (their terms cancel to below the tolerance; a
    feature dot product over 168 channels cancels by a factor of 13 on its own), so the test holds the share down, over all elements and
    over the Gaussians of middling condition (second and third quartile of tolerance / S), where a loose metric would show first."""
    c = B.comp_case(name)
    refs, _ = B.comp_ref(c)
    for v, r in enumerate(refs):
        bound, chain = r["bound"], r["chain"]
        assert not B.rejects(r["grad"], r["grad"], r["S"], bound, chain)
        if r["counts"]["clamped"]:
            bad = B.comp_ref(c, through_alpha_max=True)[0][v]
            assert B.rejects(bad["grad"], r["grad"], r["S"], bound, chain), "alpha_max passing gradient"
        else:
            assert c["scene"] == "qlen"
        tol = B.tolerance(r["grad"], r["S"], bound, chain).numpy()
        caught = np.abs(r["grad"]) > tol  # (dropping the term moves the element by |ref|)
        nz = r["grad"] != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            cond = np.where(nz, tol / r["S"], np.nan)
        lo, hi = np.nanpercentile(cond, 25), np.nanpercentile(cond, 75)
        mid = nz & (cond >= lo) & (cond <= hi)
        med, mx = B.effective_bound(r["grad"], r["S"], bound, chain)
        print(f"{name} view {v}: tolerance / S median {med / B.U24:.0f} u, max {mx / B.U24:.0f} u; a dropped term is caught at "
              f"{caught[nz].mean():.4f} of the non-zero elements, {caught[mid].mean():.4f} of the middle half")
        assert caught[nz].mean() >= 0.90 and caught[mid].mean() >= 0.95
        for k in (B.MX, B.CB, B.OP):  # and at the Gaussian of median condition of a slot
            col = np.where(nz[:, k], cond[:, k], np.inf)
            g = int(np.argsort(col)[nz[:, k].sum() // 2])
            bad = r["grad"].copy()
            bad[g, k] = 0.0
            assert B.rejects(bad, r["grad"], r["S"], bound, chain) == bool(caught[g, k])
        if c["kind"] == "feat":
            tf = B.tolerance(r["g_feats"], r["S_feats"], bound, r["chain_feats"]).numpy()
            nzf = r["g_feats"] != 0
            assert (np.abs(r["g_feats"]) > tf)[nzf].mean() >= 0.95, "g_feats: a dropped term"


@pytest.mark.parametrize("kind", ["k2", "k3"])
def test_composite_metric_rejects_the_other_saturation_comparison(kind):
    """a pixel whose transmittance lands exactly on t_min: mode 0 blends the entry (T' < t_min is false), mode 1 stops in front of it.
    Not "at every case shape": in a real case such a pixel has margin 0 (exact equality is the only place where the two comparisons
    differ) and its upstream gradient is zeroed, so no crafted case can contain one that counts; the swap is shown on a two-splat scene at
    the frame sizes of the full cases, with thresholds that are binary fractions, where the metric tells the two answers apart."""
    c = B.comp_case("k2_full" if kind == "k2" else "k3_full")
    cam = c["cams"][0]
    off = 0.5 if kind == "k3" else 0.0
    cam2 = copy.copy(cam)
    cam2.alpha_max, cam2.t_min = 1.0, 0.25  # (binary fractions: 1 - 0.75 is t_min exactly, in either precision)
    rec = np.zeros((2, 12))  # two splats centred on pixel (20, 20): opacity 0.75 in front, 0.5 behind it
    rec[:, 0], rec[:, 1] = 20.0 + off, 20.0 + off
    rec[:, 4], rec[:, 6], rec[:, 2], rec[:, 7] = 0.02, 0.02, (1.0, 2.0), (0.75, 0.5)
    T =(-(-cam.width // 16)) * (-(-cam.height // 16))
    lists = (np.arange(T + 1) * 2, np.tile(np.array([0, 1], np.int32), T))
    g = np.random.default_rng(1)
    g_out = g.normal(size=(3, cam.height, cam.width) if kind == "k2" else (cam.height, cam.width, 3))
    g_a, g_d = g.normal(size=(cam.height, cam.width)), g.normal(size=(cam.height, cam.width))
    right = B.composite_bwd64(kind, cam2, rec, lists, g_out, g_a, g_d)
    wrong = B.composite_bwd64(kind, cam2, rec, lists, g_out, g_a, g_d, sat_le=(kind == "k2"))
    assert right["margin"][20, 20] == 0.0
    assert B.rejects(wrong["grad"], right["grad"], right["S"], right["bound"], right["chain"])


# ---- (c) constants and coverage -------------------------------------------------------------------------------------------------------------
def test_exp_det_sel_constant():
    x = -np.concatenate((np.random.default_rng(0).uniform(0, 87, 2000000), np.linspace(0, 87, 1000001))).astype(np.float32)
    rel = np.abs(B.exp_det_sel32(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1.0) / (1.0 - x.astype(np.float64))
    print(f"exp_det_sel32: max relative error per (1 + |x|) = {rel.max():.3e}")
    assert 0.5 * B.EXP_DET_MEASURED <= rel.max() <= B.EXP_DET_MEASURED
    assert B.exp_det_sel32(np.float32(0.0)) == 1.0 and B.exp_det_sel32(np.float32(-87.5)) == 0.0


@pytest.mark.parametrize("name", list(B.PROJ_CASES))
def test_projection_cases_populate_their_branches(name):
    c, ref = B.proj_case(name), B.proj_ref(name)
    r = c["rect"].long()
    live = ((r[..., 2] - r[..., 0]) * (r[..., 3] - r[..., 1]) != 0)
    for v, aux in enumerate(ref["aux"]):
        cls, dist = B.clamp_class(aux)
        assert float(dist.min()) > 1e-4, "a clamp decision within fp32 reach of its limit (x / z carries a few roundings: 1e-6)"
        assert float((aux["k_pt"] * aux["k_cov"] * aux["k_det"]).max()) < 16, "an ill-conditioned row: the weighted scale would hide errors"
        if v == 0 and c["G"] > 1:
            n = np.bincount(cls[live[0]].numpy(), minlength=6)
            assert n.min() >= 8, n
        if c["mode"] == 0 and c["deg"] >= 0:
            assert float(aux["lin"].abs().min()) > 1e-3, "a colour within fp32 reach of 0"
            if v == 0 and c["G"] > 1:
                nneg = (aux["lin"] < 0).sum(-1)[live[0]]
                assert np.bincount(nneg.numpy(), minlength=4).min() >= 8
    if c["G"] == 1:
        assert int(B.clamp_class(ref["aux"][0])[0][0]) == 5
    if c["V"] > 1:
        assert int((live.any(0) & ~live.all(0)).sum()) >= 8 and int((~live.any(0)).sum()) >= 1
    lens = [B.lens_limits(c["mode"], cam)[2] for cam in c["cams"]]
    if c["mode"] == 0:
        assert all(abs(l[0] - l[2]) > 0.1 for l in lens), "tanfovx == tanfovy"
    else:
        assert all(abs(l[0] - l[1]) > 0.1 and abs(l[2] - l[3]) > 0.1 for l in lens), "a centred principal point"
    assert float(c["grad"].abs().min()) >= 0.1


@pytest.mark.parametrize("name", list(B.COMP_CASES))
def test_composite_cases_populate_their_branches_and_keep_the_margin_cap(name):
    c = B.comp_case(name)
    refs, ups = B.comp_ref(c)
    assert len(refs) == c["V"]
    for v, r in enumerate(refs):
        n = r["counts"]
        low = int((r["margin"] < B.MARGIN).sum())
        print(f"{name} view {v}: {n}, pixels below the margin {low} of {r['margin'].size}")
        assert low <= B.ZERO_SHARE_CAP * r["margin"].size
        bad, low2, _ = B.walk32_agrees(c["kind"], c["cams"][v], c["rec"][v], c["lists"][v], r["margin"])
        assert bad == 0 and low2 == low, "the float32 walk leaves the float64 branch above the margin"
        assert n["blend"] > 5000 and n["below_alpha_min"] > 1000 and n["saturated"] > 0 and n["entries_behind_saturation"] > 0
        assert n["longest_list"] <= 512
        rec = c["rec"][v]
        if c["scene"] != "qlen":
            assert int(((r["hit_clamped"] > 0) & (r["hit_free"] > 0)).sum()) >= 2, "no Gaussian with pixels on both sides of alpha_max"
            assert n["clamped"] >= 2 and n["sigma_skip"] >= 100 and n["empty_tiles"] >= 1
            dead = rec[:, 7] < c["cams"][v].alpha_min
            assert dead.sum() >= 8 and r["n_add"][dead].sum() == 0
            live = (c["rect"][v][:, 2] - c["rect"][v][:, 0]) > 0
            assert np.unique(rec[live, 2]).size <= live.sum() - 30, "no equal depth keys"
            assert r["n_add"][0] > 500, "Gaussian 0 is not heavy"
        if c["scene"] == "full":
            bs, ent = c["bins"][v]
            ts = c["lists"][v][0]
            assert bs[1] - bs[0] > 256 + 20 and ts[1] - ts[0] > 256 and ts[1] - ts[0] < bs[1] - bs[0], "bin 0 / tile 0: two staging slices, entries that do not cover"
        if name in ("k2_ragged", "k3_full", "feat_full"):
            assert c["W"] % 16 and c["H"] % 16, "no pixels off the frame in the last tile row and column"
        if c["kind"] == "feat":
            ql = B.quadrant_lists_ref(c["cams"][v], rec, c["lists"][v])
            lens = sorted(set(len(x) for x in ql.values()))
            if c["scene"] == "qlen":
                assert {0, 1, 31, 32, 33}.issubset(lens) and max(lens) > 64, lens
                # tile (3, 3), quadrant 0: its list holds the forty slivers, none of which reaches a pixel centre of the quadrant: its
                # second chunk of 32 entries blends nothing while the quadrant's pixels are still walking
                sl = ql[(3 * 6 + 3, 0)]
                slivers = np.arange(c["G"] - 40, c["G"])
                assert np.isin(slivers, sl).all() and np.isin(sl[32:], slivers).all() and len(sl) > 32
                assert r["n_add"][slivers].min() > 0, "the slivers blend in their own quadrant"
                w = c["walk_cache"][v][3 * 6 + 3][0]
                px, py, inside, _ = B._tile_pixels(c["cams"][v], 3 * 6 + 3, True)
                q0 = (px % 16 < 8) & (py % 16 < 8)
                ids = c["lists"][v][1][c["lists"][v][0][21]:c["lists"][v][0][22]]
                assert not w["bl"][np.isin(ids, slivers)][:, q0].any() and not w["saturated"][q0].any()
            assert r["n_add"][0] > 500


def test_upstream_modes_zero_what_they_say():
    c = B.comp_case("k2_ragged")
    for mode in B.COMP_MODES:
        refs, ups = B.comp_ref(c, mode)
        r = refs[0]
        zero = {"all": (), "depth_only": (B.RR, B.GG, B.BB), "alpha_only": (B.RR, B.GG, B.BB, B.ZZ), "one_colour": (B.RR, B.BB, B.ZZ)}[mode]
        for k in zero:
            assert np.abs(r["grad"][:, k]).max() == 0.0 and r["S"][:, k].max() == 0.0
        assert np.abs(r["grad"][:, B.OP]).max() > 0
        low = r["margin"] < B.MARGIN
        assert low.any() and np.abs(ups["g_alpha"][0][low]).max() == 0 and np.abs(ups["g_depth"][0][low]).max() == 0
