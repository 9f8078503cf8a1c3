"""CPU tests of the anti-aliased K2 path and the 3-D smoothing filter: invariants of the float64 restatements (tests/dense_antialias64.py),
the float32 emulation of the kernel's operation order inside the derived bound, the filter's rules on hand-placed cameras, the control's
validation and the drop-in settings tuple.  The GPU tests (tests/test_antialias_gpu.py) hold the kernels to the same references."""
import math

import numpy as np
import pytest
import torch

import dense_antialias64 as A
import dense_raster_bwd64 as B

DD = torch.float64


def _visible(c):
    keep = torch.ones(c["G"], dtype=torch.bool)
    keep[list(c["expect_culled"])] = False
    return keep


def test_compensation_preserves_the_footprint_integral():
    """comp sqrt(det1) = sqrt(det0) above the floor: the dilated footprint integrates to what the undilated one does"""
    c = A.aa_case()
    vis = _visible(c)
    for r in A.aa_forward_ref(c["cams"], c):
        a = r["aux"]
        ok = vis & ~a["floor"]
        lhs, rhs = a["comp"] * a["det1"].sqrt(), a["det0"].sqrt()
        assert int(ok.sum()) >= 58 and float(((lhs - rhs).abs() / rhs)[ok].max()) < 1e-13
        assert bool((a["comp"][ok] < 1.0).all()) and bool((a["comp"][ok] > 0.0).all())
        assert torch.equal(r["rec7"][vis], (c["opac"].double() * a["comp"])[vis])


def test_comp_tends_to_one_for_a_large_splat_and_sits_on_the_floor_for_a_point():
    c = A.aa_case()
    for r in A.aa_forward_ref(c["cams"], c):
        a = r["aux"]
        cover, floor = A.SPECIAL["cover"], A.SPECIAL["floor"]
        assert 1.0 - float(a["comp"][cover]) < 2e-3, "a splat of hundreds of pixels loses nothing"
        assert bool(a["floor"][floor]) and float(a["comp"][floor]) == math.sqrt(2.5e-5) and float(a["r"][floor]) < 1e-3 * A.AA_FLOOR
        assert int(a["floor"][_visible(c)].sum()) == 1, "only the crafted point is on the floor"
        rel = ((a["r"] - A.AA_FLOOR).abs() / A.AA_FLOOR)[_visible(c)]
        assert float(rel.min()) > 0.5, "no crafted row is near the floor: float32 and float64 take the same branch"


def test_the_floor_passes_no_gradient_to_the_covariance():
    c = A.aa_case()
    cam = c["cams"][0]
    cov = c["cov6"].double().requires_grad_()
    op = c["opac"].double().requires_grad_()
    rec, aux = A.aa_record64(cam, c["means"], cov, op, c["colors"])
    vis = _visible(c)
    g_cov, g_op = torch.autograd.grad(rec[vis, A.OP].sum(), (cov, op))
    fl = A.SPECIAL["floor"]
    assert float(g_cov[fl].abs().max()) == 0.0 and float(g_op[fl]) == math.sqrt(2.5e-5)
    others = vis.clone()
    others[fl] = False
    assert bool((g_cov[others].abs().amax(-1) > 0).all()), "above the floor the compensation depends on the covariance"
    assert torch.allclose(g_op[others], aux["comp"].detach()[others], rtol=0, atol=0)


def test_condition_products_of_the_crafted_set():
    """the coverage condition of the weighted bounds: both condition products stay <= 16 on every compared row"""
    c = A.aa_case()
    vis = _visible(c)
    worst = 0.0
    for r in A.aa_forward_ref(c["cams"], c):
        a = r["aux"]
        kc = a["k_pt"] * a["k_cov"]
        k1, k0 = (kc * a["k_det"])[vis], torch.where(a["floor"], torch.ones_like(kc), kc * a["k_det0"])[vis]
        worst = max(worst, float(k1.max()), float(k0.max()))
        assert float(a["k_det0"][A.SPECIAL["thin"]]) > 3.0, "the diagonal splat does cancel in c00' c11' - c01^2"
    print(f"largest condition product on the crafted set: {worst:.2f}")
    assert worst <= 16.0, worst


def test_float32_emulation_of_the_kernel_order_stays_inside_the_bound():
    c = A.aa_case()
    vis = _visible(c)
    for v, r in enumerate(A.aa_forward_ref(c["cams"], c)):
        comp32, r32 = A.comp_emul32(c["cams"][v], c["means"].numpy(), c["cov6"].numpy())
        assert np.array_equal(r32[vis.numpy()] <= np.float32(A.AA_FLOOR), r["floor"][vis].numpy())
        w = B.assert_elems_close(torch.from_numpy(comp32)[vis], r["comp"][vis], (r["comp"] * r["rel"])[vis], A.AA_FWD_BOUND, name=f"comp emulation view {v}")
        assert w <= 1.0
        rec7 = torch.from_numpy(c["opac"].numpy() * comp32)
        B.assert_elems_close(rec7[vis], r["rec7"][vis], (r["rec7"].abs() * r["rel"])[vis], A.AA_FWD_BOUND, name=f"record opacity emulation view {v}")
        # a wrong answer is told apart: the compensation of the dilated determinant alone (det1 in place of det0 + the dilation's share)
        wrong = torch.sqrt(torch.clamp((r["aux"]["det1"] - 0.3 * (r["aux"]["c00p"] + r["aux"]["c11p"])) / r["aux"]["det1"], min=A.AA_FLOOR))
        assert B.rejects(wrong[vis], r["comp"][vis], (r["comp"] * r["rel"])[vis], A.AA_FWD_BOUND)


def test_kahan_determinant_recovers_what_the_naive_form_loses():
    """det0 of a needle on the diagonal from EXACT float32 entries: the naive form is off by thousands of ulps, conic_det's form by two"""
    rng = np.random.default_rng(1)
    f32 = np.float32
    a = rng.uniform(1.0, 2.0, 1000).astype(f32)
    cc = rng.uniform(1.0, 2.0, 1000).astype(f32)
    b = (np.sqrt(a.astype(np.float64) * cc) * (1.0 - 1e-5)).astype(f32)
    exact = a.astype(np.float64) * cc - b.astype(np.float64) ** 2
    naive = a * cc - b * b
    w = b * b
    e = (-b.astype(np.float64) * b + w).astype(f32)
    kahan = (a.astype(np.float64) * cc - w).astype(f32) + e
    assert float(np.max(np.abs(kahan - exact) / exact)) <= 2 * 2.0 ** -23
    assert float(np.max(np.abs(naive - exact) / exact)) > 1000 * 2.0 ** -24


def test_backward_reference_adds_the_compensation_term_in_front_of_the_chain():
    """the autograd pull-back of the anti-aliased record = the classic one with the opacity gradient scaled by comp, plus a covariance /
    mean / pose term that exists only above the floor"""
    c = A.aa_case()
    rect = torch.zeros((c["V"], c["G"], 4), dtype=torch.int32)
    rect[:] = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    rect[:, list(c["expect_culled"])] = 0
    aa = A.project_bwd_aa64(c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], rect, c["grad"])
    classic = B.project_bwd64(0, c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], rect, c["grad"])
    live, vis = ((rect[..., 2] - rect[..., 0]) != 0), _visible(c)
    want_op = torch.where(live, aa["comp"] * c["grad"][..., A.OP].double(), torch.zeros((), dtype=DD)).sum(0)
    assert torch.allclose(aa["g_opac"][0], want_op, rtol=1e-12, atol=0)
    only_op = c["grad"].clone()
    only_op[..., :A.OP], only_op[..., A.OP + 1:] = 0, 0
    term = A.project_bwd_aa64(c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], rect, only_op)
    fl = A.SPECIAL["floor"]
    assert float(term["g_cov"][0][fl].abs().max()) == 0.0 and float(term["g_means"][0][fl].abs().max()) == 0.0
    assert float(term["g_cov"][0][0].abs().max()) > 0.0
    for n in ("g_means", "g_cov"):
        assert torch.allclose(aa[n][0][vis], (classic[n][0] + term[n][0])[vis], rtol=1e-9, atol=1e-12), n  # (the classic reference leaves the NaN row NaN)
    assert torch.equal(aa["g_colors"][0][vis], classic["g_colors"][0][vis])


# ---- the 3-D filter --------------------------------------------------------------------------------------------------------------------------
def _one_cam(W=64, H=48):
    c2w = torch.eye(4)[None]
    Kn = torch.tensor([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]])
    return c2w, Kn, W, H


def test_filter_rules_on_hand_placed_cameras():
    c2w, Kn, W, H = _one_cam()
    c2w = torch.cat([c2w, c2w])
    c2w[1, 2, 3] = -1.0  # the second camera one unit further back: it sees everything one unit deeper
    Kn = torch.cat([Kn, Kn])
    Kn[1, 0, 0] = 2.0  # focal = the largest fx = 2 W
    means = torch.tensor([[0.0, 0.0, 2.0],      # seen by both: d = 2 (the first camera is nearer)
                          [0.0, 0.0, -0.5],     # behind the first, 0.5 in front of the second: d = 0.5
                          [0.0, 0.0, -3.0],     # behind every camera: unseen
                          [-1.2, 0.0, 2.0],     # pixel x = -0.1 W of camera 0: outside the frame, inside the margin: seen, d = 2
                          [-1.5, 0.0, 2.0],     # pixel x = -0.25 W of camera 0 (unseen there); camera 1 (fx = 2 W): x = -W + W / 2: unseen
                          [0.0, 0.0, 5.0],      # the farthest seen point: d = 5 (camera 0)
                          [0.0, 0.0, 0.1]])     # closer than z_near to camera 0, 1.1 from camera 1: d = 1.1
    r = A.filter3d64(means, c2w, Kn, W, H)
    assert r["seen"].tolist() == [[True, False, False, True, False, True, False], [True, True, False, False, False, True, True]]
    assert torch.allclose(r["d"], torch.tensor([2.0, 0.5, 0.0, 2.0, 0.0, 5.0, 1.1], dtype=DD), atol=1e-7)
    assert r["focal"] == 2.0 * W and r["dmax"] == 5.0
    want = math.sqrt(0.2) * torch.tensor([2.0, 0.5, 5.0, 2.0, 5.0, 5.0, 1.1], dtype=DD) / (2.0 * W)  # unseen rows: the global maximum
    assert torch.allclose(r["filter"], want, atol=1e-9)
    none = A.filter3d64(means[[2, 4]], c2w, Kn, W, H)
    assert float(none["filter"].abs().max()) == 0.0 and not bool(none["seen"].any()), "nothing seen: zeros"
    off = A.filter3d64(means[:1], c2w[:1], torch.tensor([[[1.0, 0.0, 0.9], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]]), W, H, margin=0.05)
    assert bool(off["seen"][0, 0]) and not bool(A.filter3d64(means[:1] + torch.tensor([0.4, 0.0, 0.0]), c2w[:1],
                                                             torch.tensor([[[1.0, 0.0, 0.9], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]]), W, H, margin=0.05)["seen"][0, 0]), \
        "the principal point of Kn, not the image centre, places the pixel"


def test_filter_case_covers_every_rule_and_is_decided():
    c = A.filter_case()
    r = A.filter3d64(c["means"], c["c2w"], c["Kn"], c["W"], c["H"])
    seen_any = r["seen"].any(0)
    assert bool(r["decided"].all()), torch.nonzero(~r["decided"]).reshape(-1).tolist()
    assert not bool(seen_any[240:244].any()) and bool(seen_any[244:248].all()) and not bool(seen_any[248:253].any())
    assert bool(seen_any[253]) and bool(seen_any[254]) and not bool(seen_any[255])
    assert abs(r["dmax"] - 9.0) < 0.05 and float(r["d"][seen_any].min()) < 0.3
    partly = (r["seen"].sum(0) > 0) & (r["seen"].sum(0) < c["V"])
    assert int(partly.sum()) >= 4, "some rows are seen by some views only"
    assert torch.equal(r["filter"][~seen_any], r["filter"][253].expand(int((~seen_any).sum())))
    assert abs(r["focal"] - 0.95 * c["W"]) < 1e-4


def test_apply_reference():
    c = A.apply_case()
    sf, of = A.apply64(c["scales"], c["opac"], c["filt"])
    s, f, o = c["scales"].double(), c["filt"].double(), c["opac"].double()
    assert torch.allclose(sf[1], s[1]) and float(of[1]) == float(o[1]), "no filter: the input back"
    vol = (s.prod(-1) / sf.prod(-1))
    assert torch.allclose(of[3:], (o * vol)[3:], rtol=1e-12), "opacity x volume ratio: the integral is preserved"
    assert 0.0 < float(of[0]) < 1e-30
    (gs, Ss), (go, So) = A.apply_bwd64(c["scales"], c["opac"], c["filt"], c["g_sf"], c["g_of"])
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(go).all()) and bool((Ss >= gs.abs() * (1 - 1e-12)).all())


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------
def test_mipfilter_validate():
    from siu3r_amd.mip import MipFilter

    MipFilter().validate()
    MipFilter(filter_2d=False).validate()
    MipFilter(filter_3d=False).validate()
    for kw, match in ((dict(filter_2d=False, filter_3d=False), "neither"), (dict(every=0), "every"), (dict(every=-5), "every"),
                      (dict(variance_3d=0.0), "variance_3d"), (dict(variance_3d=-1.0), "variance_3d"), (dict(variance_3d=float("nan")), "variance_3d")):
        with pytest.raises(ValueError, match=match):
            MipFilter(**kw).validate()
    d = MipFilter()
    assert (d.filter_2d, d.filter_3d, d.variance_3d, d.every) == (True, True, 0.2, 100)


def test_antialiasing_is_the_last_settings_field():
    from siu3r_amd.compat.diff_gaussian_rasterization import GaussianRasterizationSettings as S

    assert S._fields[-1] == "antialiasing" and S._field_defaults["antialiasing"] is False
    assert S._fields[:13] == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "projmatrix_raw",
                              "sh_degree", "campos", "prefiltered", "debug")


def test_new_symbols_are_declared_exported_and_documented():
    from siu3r_amd import _lib

    l = _lib.lib()
    text = open(_lib.os.path.join(_lib._HERE, "..", "include", "siu3r_hip.h")).read()
    for s in ("siu3r_raster_project_aa", "siu3r_raster_project_c2w_aa", "siu3r_raster_project_bwd_aa", "siu3r_mip_filter3d_ws", "siu3r_mip_filter3d",
              "siu3r_mip_apply", "siu3r_mip_apply_bwd"):
        assert s in _lib.SIGNATURES and hasattr(l, s) and f"{s}(" in text, s
    assert len(_lib.SIGNATURES["siu3r_raster_project_aa"]) == len(_lib.SIGNATURES["siu3r_raster_project"]) + 1
    assert len(_lib.SIGNATURES["siu3r_raster_project_c2w_aa"]) == len(_lib.SIGNATURES["siu3r_raster_project_c2w"]) + 1
    assert _lib.SIGNATURES["siu3r_raster_project_bwd_aa"] == _lib.SIGNATURES["siu3r_raster_project_bwd"]
    assert l.siu3r_mip_filter3d_ws.restype is _lib.C.c_int64 and l.siu3r_mip_filter3d_ws(3) >= 4 * (16 * 3 + 1) and l.siu3r_abi_version() == 13


def test_front_end_keywords_exist_and_default_off():
    import inspect

    from siu3r_amd import cuda_splatting, prune, raster, refine

    for fn in (raster.rasterize_views_k2, raster.contributions_k2, cuda_splatting.render_cuda, prune.gaussian_contributions):
        assert inspect.signature(fn).parameters["antialiased"].default is False, fn
    assert inspect.signature(refine.refine_gaussians).parameters["antialias"].default is None
    assert "antialiased" in raster.RasterState.__slots__ and raster.RasterState().antialiased is None
