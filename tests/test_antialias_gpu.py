"""GPU tests of the anti-aliased K2 path (siu3r_raster_project_aa / _c2w_aa, siu3r_raster_project_bwd_aa, raster.rasterize_views_k2 /
contributions_k2 with antialiased=True, the drop-in `antialiasing` field) and of the 3-D smoothing filter (siu3r_mip_filter3d,
siu3r_mip_apply / _bwd, mip.py, refine_gaussians(antialias=)): the kernels against the float64 restatements and bounds of
tests/dense_antialias64.py, per element; the classic outputs bit for bit where the anti-aliased calls promise them unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_antialias64 as A
import dense_raster64 as DR
import dense_raster_bwd64 as B
from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _render, _truth
from scenes import default_K, look_at_camera, random_scene
from test_raster_stages_gpu import SENT, _Guarded

pytestmark = pytest.mark.gpu
U24 = B.U24


def _f(shape):
    return _Guarded(shape, torch.float32)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).contiguous().cuda()


def _p(t):
    return None if t is None else (t.t if isinstance(t, _Guarded) else t).data_ptr()


def _call(name, *args):
    from siu3r_amd import _lib
    from siu3r_amd.ops import _stream

    rc = getattr(_lib.lib(), name)(*args, _stream())
    torch.cuda.synchronize()
    return rc


def _ok(name, *args):
    from siu3r_amd import _lib

    _lib.check(_call(name, *args), name)


def _refused(name, match, *args):
    from siu3r_amd import _lib

    assert _call(name, *args) != 0, f"{name} accepted a call it documents as an error"
    assert match in _lib.lib().siu3r_last_error().decode(), _lib.lib().siu3r_last_error().decode()


def _cov(c, stride):
    if stride == 6:
        return _dev(c["cov6"])
    cov = torch.full((c["G"], 9), float("nan"))  # [G,3,3]: the entries the kernels must not read are NaN
    cov[:, [0, 1, 2, 4, 5, 8]] = c["cov6"]
    return cov.cuda()


def _cams_for(c, entry):
    """the host blocks of an entry point: "host" carries the poses, "c2w" only the planes (the device derives the rest)"""
    from siu3r_amd import raster

    if entry == "host":
        return c["cams"], ()
    cams = [raster.make_cam_k2(None, None, None, None, None, [0.1, 0.2, 0.3], c["W"], c["H"], sh_degree=-1, near=0.2, far=1000.0) for _ in range(c["V"])]
    return cams, (_dev(c["c2w"]), _dev(c["Kn"]))


def _project(c, entry, stride, aa, want_comp=True, keep=None):
    """one projection call on the crafted set -> outputs (CPU tensors), the camera blocks the kernel used"""
    from siu3r_amd import raster

    cams, pose = _cams_for(c, entry)
    V, G = c["V"], c["G"]
    arr = raster._cam_array(cams)
    cams_dev = _Guarded((V * C.sizeof(cams[0]) // 4,))
    means, opac, cov, colors = _dev(c["means"]), _dev(c["opac"]), _cov(c, stride), _dev(c["colors"])
    o = dict(rec=_f((V, G, 12)), radii=_Guarded((V, G, 2)), rect=_Guarded((V, G, 4)), tiles=_Guarded((V, G)), keys=_Guarded((V, G)),
             stats=_Guarded((V, 4), torch.int64))
    if aa and want_comp:
        o["comp"] = _f((V, G))
    name = {("host", False): "siu3r_raster_project", ("host", True): "siu3r_raster_project_aa", ("c2w", False): "siu3r_raster_project_c2w",
            ("c2w", True): "siu3r_raster_project_c2w_aa"}[(entry, aa)]
    args = [arr, V, _p(cams_dev), *((_p(pose[0]), _p(pose[1]), 1.0) if pose else ()), G, _p(means), _p(cov), stride, _p(opac), _p(colors), 1, 0,
            *[_p(o[k]) for k in ("rec", "radii", "rect", "tiles", "keys", "stats")], *([_p(o.get("comp"))] if aa else [])]
    _ok(name, *args)
    for k, b in o.items():
        assert b.guards_intact(), f"{name}: {k} written outside the buffer"
    assert cams_dev.guards_intact()
    blocks = (type(cams[0]) * V).from_buffer_copy(cams_dev.t.cpu().numpy().tobytes())
    if keep is not None:
        keep.update(arr=arr, cams_dev=cams_dev, dev=dict(means=means, opac=opac, cov=cov, colors=colors, rect=o["rect"].t))
    return {k: b.t.cpu() for k, b in o.items()}, blocks


# ---- 1: the projection stage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "c2w"])
@pytest.mark.parametrize("stride", [6, 9])
def test_projection_stage(entry, stride):
    c = A.aa_case()
    classic, blocks0 = _project(c, entry, stride, aa=False)
    got, blocks = _project(c, entry, stride, aa=True)
    assert bytes(blocks) == bytes(blocks0), "the camera blocks of the two calls are the same bytes"
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    for k in ("radii", "rect", "tiles", "keys", "stats"):
        assert torch.equal(got[k], classic[k]), f"{k} differs from the classic projection"
    live = (got["rect"][..., 2] - got["rect"][..., 0]) * (got["rect"][..., 3] - got["rect"][..., 1]) != 0
    # slots 8 .. 11 of a culled row are not written by either call (sentinel); every written slot but 7 is the classic call's bits
    others = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
    assert torch.equal(bits(got["rec"][..., others]), bits(classic["rec"][..., others])), "a record slot other than the opacity moved"
    assert torch.equal(bits(got["rec"][..., 7][~live]), bits(classic["rec"][..., 7][~live])), "a culled row's opacity slot is the classic one"
    assert float(got["comp"][~live].abs().max()) == 0.0 and bool((got["comp"][~live] == 0).all()), "comp is 0 where the rect is empty"
    for g in c["expect_culled"]:
        assert not bool(live[:, g].any()), g
    for name in ("floor", "thin", "cover", "clamp"):
        assert bool(live[0, A.SPECIAL[name]]), f"the {name} row is visible in view 0"
    cams = [blocks[v] for v in range(c["V"])]
    refs = A.aa_forward_ref(cams, c)
    for v, r in enumerate(refs):
        m = live[v]
        on_floor = got["comp"][v] < float(np.sqrt(A.AA_FLOOR)) * (1.0 + 1e-5)  # (no crafted row is within a factor 1.5 of the floor)
        assert torch.equal(r["floor"][m], on_floor[m]), "float32 and float64 agree on who is on the floor"
        B.assert_elems_close(got["comp"][v][m], r["comp"][m], (r["comp"] * r["rel"])[m], A.AA_FWD_BOUND, name=f"{entry} stride {stride} view {v} comp")
        B.assert_elems_close(got["rec"][v, :, 7][m], r["rec7"][m], (r["rec7"].abs() * r["rel"])[m], A.AA_FWD_BOUND, name=f"{entry} stride {stride} view {v} rec[7]")
        # the record holds exactly the product of the two floats
        assert torch.equal(bits(got["rec"][v, :, 7][m]), bits((c["opac"] * got["comp"][v])[m]))
    assert bool(refs[0]["floor"][A.SPECIAL["floor"]]) and float(got["comp"][0, A.SPECIAL["cover"]]) > 0.998
    # comp is optional: NULL leaves every other output as it is
    again, _ = _project(c, entry, stride, aa=True, want_comp=False)
    for k in ("radii", "rect", "tiles", "keys", "stats"):
        assert torch.equal(again[k], got[k])
    assert torch.equal(bits(again["rec"][..., :8]), bits(got["rec"][..., :8]))


# ---- 2: the projection backward ----------------------------------------------------------------------------------------------------------
def _project_bwd(c, st, stride, grad, name="siu3r_raster_project_bwd_aa", m2d=True, pose=True):
    V, G, d = c["V"], c["G"], st["dev"]
    rows = -(-G // 256)
    out = dict(g_means=_f((G, 3)), g_cov=_f((G, stride)), g_opac=_f((G,)), g_colors=_f((G, 1, 3)), g_mean2d=_f((V, G, 2)) if m2d else None,
               part=_f((rows, V, 6)) if pose else None)
    _ok(name, st["arr"], V, _p(st["cams_dev"]), G, _p(d["means"]), _p(d["cov"]), stride, _p(d["opac"]), _p(d["colors"]), 1, 0, _p(d["rect"]), _p(grad),
        *[_p(out[k]) for k in ("g_means", "g_cov", "g_opac", "g_colors", "g_mean2d", "part")])
    for k, b in out.items():
        assert b is None or b.guards_intact(), f"{name}: {k} written outside the buffer"
    return {k: None if b is None else b.t.cpu() for k, b in out.items()}


@pytest.mark.parametrize("stride", [6, 9])
def test_projection_backward(stride):
    c = A.aa_case()
    V, G = c["V"], c["G"]
    st = {}
    fwd, blocks = _project(c, "host", stride, aa=True, keep=st)
    rect = fwd["rect"]
    live = (rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1]) != 0
    out = _project_bwd(c, st, stride, _dev(c["grad"]))
    ref = A.project_bwd_aa64(c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], rect, c["grad"])
    tag = f"aa backward stride {stride}"
    B.assert_elems_close(out["g_means"], *ref["g_means"], A.AA_BWD_BOUND, name=f"{tag} g_means")
    B.assert_elems_close(out["g_opac"], *ref["g_opac"], A.AA_BWD_BOUND, name=f"{tag} g_opac")
    gc = out["g_cov"]
    if stride == 9:
        assert float(gc[:, [3, 6, 7]].abs().max()) == 0.0, "the lower triangle gets exactly 0"
        gc = gc[:, [0, 1, 2, 4, 5, 8]]
    B.assert_elems_close(gc, *ref["g_cov"], A.AA_BWD_BOUND, name=f"{tag} g_cov")
    B.assert_elems_close(out["g_colors"], *ref["g_colors"], A.AA_BWD_BOUND, name=f"{tag} g_colors")
    assert torch.equal(out["g_mean2d"][live], c["grad"][..., :2][live]) and bool((out["g_mean2d"][~live] == SENT).all())
    want, S = B.partial_rows64(*ref["pose_g"], 6)
    B.assert_elems_close(out["part"], want, S, A.AA_BWD_BOUND + 9 * U24, name=f"{tag} pose partial rows")
    # the classic kernel on the same inputs: colours and the pixel-space means do not pass through the compensation
    classic = _project_bwd(c, st, stride, _dev(c["grad"]), name="siu3r_raster_project_bwd")
    assert torch.equal(out["g_colors"], classic["g_colors"]) and torch.equal(out["g_mean2d"], classic["g_mean2d"])
    assert not torch.equal(out["g_cov"], classic["g_cov"]) and not torch.equal(out["g_opac"], classic["g_opac"])
    # the opacity slot alone: the floor row receives exactly comp * grad[OP] (summed over the views in order) and nothing in g_cov or g_means
    only = c["grad"].clone()
    only[..., :A.OP], only[..., A.OP + 1:] = 0, 0
    o2 = _project_bwd(c, st, stride, _dev(only), m2d=False, pose=False)
    fl = A.SPECIAL["floor"]
    assert bool(live[:, fl].all()) and bool(ref["floor"][:, fl].all())
    want_fl = torch.zeros((), dtype=torch.float32)
    for v in range(V):
        want_fl = want_fl + fwd["comp"][v, fl] * only[v, fl, A.OP]
    assert float(o2["g_opac"][fl]) == float(want_fl), (float(o2["g_opac"][fl]), float(want_fl))
    assert float(o2["g_cov"][fl].abs().max()) == 0.0 and float(o2["g_means"][fl].abs().max()) == 0.0, "on the floor comp is a constant"
    th = A.SPECIAL["thin"]
    assert float(o2["g_cov"][th].abs().max()) > 0.0 and float(o2["g_means"][th].abs().max()) > 0.0, "above it the compensation reaches the covariance"
    only_ref = A.project_bwd_aa64(c["cams"], c["means"], c["cov6"], c["opac"], c["colors"], rect, only)
    g2 = o2["g_cov"] if stride == 6 else o2["g_cov"][:, [0, 1, 2, 4, 5, 8]]
    B.assert_elems_close(g2, *only_ref["g_cov"], A.AA_BWD_BOUND, name=f"{tag} compensation term alone, g_cov")
    B.assert_elems_close(o2["g_means"], *only_ref["g_means"], A.AA_BWD_BOUND, name=f"{tag} compensation term alone, g_means")


# ---- 3, 4: end to end ----------------------------------------------------------------------------------------------------------------------
REL_BAR = 5e-3  # the bar of the end-to-end K2 gradient tests (tests/test_raster_backward_gpu.py)


def _cam(Hh, Ww, seed, degree, bg=(0.1, 0.2, 0.3)):
    from siu3r_amd import cuda_splatting as cs, raster

    c2w = look_at_camera(seed)
    K = default_K()[None]
    fov = cs.get_fov(K)
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([0.2]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(c2w)
    return raster.make_cam_k2(w2c, proj @ w2c, float(tan[0]), float(tan[1]), c2w[:3, 3].tolist(), list(bg), Ww, Hh, sh_degree=degree)


def _small_frame():
    """V = 2 views of 32 x 32, G = 48 Gaussians between a fifth of a pixel and a few pixels wide: the compensation runs from 0.17 to 0.97"""
    from siu3r_amd import raster

    Hh = Ww = 32
    means, cov, opac, sh = random_scene(48, seed=9, n_sh=4, spread=0.5, depth=(1.5, 4.0), scale=(0.004, 0.15))
    cams = [_cam(Hh, Ww, s, 1) for s in (0, 1)]
    return Hh, Ww, cams, means, raster.cov6_from_cov3x3(cov), opac, sh.permute(0, 2, 1).contiguous()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_end_to_end_against_the_dense_float64_renderer():
    from siu3r_amd import raster

    Hh, Ww, cams, means, cov6, opac, shs = _small_frame()
    V, G = len(cams), means.shape[0]
    leaves = [t.cuda().requires_grad_() for t in (means, cov6, shs, opac)]
    xi = torch.zeros(V, 6, device="cuda", requires_grad=True)
    o = raster.rasterize_views_k2(cams, *leaves, pose_delta=xi, antialiased=True)
    plain = raster.rasterize_views_k2(cams, *(t.detach() for t in leaves))
    assert o["state"].antialiased and not plain["state"].antialiased
    assert torch.equal(o["radii"], plain["radii"]) and not torch.equal(o["image"], plain["image"])
    assert float(o["opacity"].detach().sum()) < float(plain["opacity"].sum()), "the compensation only lowers opacities"
    with torch.no_grad():
        again = raster.rasterize_views_k2(cams, *(t.detach() for t in leaves), antialiased=True)
    for k in ("image", "depth", "opacity", "n_touched"):
        assert torch.equal(o[k], again[k]), f"{k}: the forward bits do not depend on grad mode"
    g = torch.Generator().manual_seed(3)
    w1, w2, w3 = torch.randn(V, 3, Hh, Ww, generator=g), torch.randn(V, Hh, Ww, generator=g), torch.randn(V, Hh, Ww, generator=g)
    loss = (o["image"] * w1.cuda()).sum() + (o["depth"] * w2.cuda()).sum() + (o["opacity"] * w3.cuda()).sum()
    got = torch.autograd.grad(loss, leaves + [xi])
    st = o["state"]
    ref_leaves = [t.detach().cpu().double().requires_grad_() for t in leaves]
    ref_xi = torch.zeros(V, 6, dtype=torch.float64, requires_grad=True)
    ref_loss, comps = 0.0, []
    for v in range(V):
        mask = DR.tile_mask_from_rect(st["rect"][v].cpu(), Ww, Hh)
        vis = mask.any(1)
        rec, aux = A.aa_record64(cams[v], ref_leaves[0], ref_leaves[1], ref_leaves[3], ref_leaves[2], ref_xi[v])
        op_v = torch.where(vis, rec[:, A.OP], ref_leaves[3])  # the per-view compensated opacities (a culled row takes no part)
        comps.append(aux["comp"].detach()[vis])
        img, d, a = DR.render(cams[v], ref_leaves[0], ref_leaves[1], ref_leaves[2], op_v, mask, xi=ref_xi[v], depth_key=st["rec"][v, :, 2].cpu())
        ref_loss = ref_loss + (img * w1[v].double()).sum() + (d * w2[v].double()).sum() + (a * w3[v].double()).sum()
        for name, x, y in (("image", img, o["image"][v]), ("depth", d, o["depth"][v]), ("opacity", a, o["opacity"][v])):
            diff = (x.detach() - y.detach().cpu().double()).abs()
            print(f"end to end view {v} {name}: max |diff| {float(diff.max()):.3e}, share above 1e-4 {float((diff > 1e-4).double().mean()):.4f}")
            assert float((diff > 1e-4).double().mean()) <= 1e-3 and float(diff.max()) < 1e-2, (name, float(diff.max()))
    comps = torch.cat(comps)
    assert float(comps.min()) < 0.3 and float(comps.max()) > 0.95, "the frame spans strong and negligible compensation"
    want = torch.autograd.grad(ref_loss, ref_leaves + [ref_xi])
    errs = {n: _rel(g_, w_) for n, g_, w_ in zip(("means", "cov", "colors", "opacities", "pose"), got, want)}
    print("anti-aliased end to end, relative L2 errors", {k: f"{e:.2e}" for k, e in errs.items()})
    for n, e in errs.items():
        assert e <= REL_BAR, (n, e, errs)


def test_contributions_follow_the_compensated_opacities():
    from siu3r_amd import raster

    Hh, Ww, cams, means, cov6, opac, _ = _small_frame()
    V, G = len(cams), means.shape[0]
    means, cov6, opac = means.cuda(), cov6.cuda(), opac.cuda()
    pre = []
    for cam in cams:  # precomputed colours without a background: a colour channel of a pixel is exactly its weight of the one-hot Gaussian
        c2 = type(cam)()
        C.memmove(C.byref(c2), C.byref(cam), C.sizeof(cam))
        c2.sh_degree = -1
        c2.bg[0] = c2.bg[1] = c2.bg[2] = 0.0
        pre.append(c2)
    wmaps = torch.zeros((V, Hh * Ww, G), device="cuda")
    for g0 in range(0, G, 3):
        cols = torch.zeros((G, 1, 3), device="cuda")
        for ch in range(min(3, G - g0)):
            cols[g0 + ch, 0, ch] = 1.0
        img = raster.rasterize_views_k2(pre, means, cov6, cols, opac, want_n_touched=False, antialiased=True)["image"]
        n = min(3, G - g0)
        wmaps[:, :, g0:g0 + n] = img.reshape(V, 3, -1)[:, :n].permute(0, 2, 1)
    got = raster.contributions_k2(cams, means, cov6, opac, antialiased=True)
    plain = raster.contributions_k2(cams, means, cov6, opac)
    assert int((wmaps != 0).sum()) > 0
    assert torch.equal(got["wmax"].view(torch.int32), wmaps.amax(1).view(torch.int32)), "wmax is the maximum of the anti-aliased forward's weights"
    assert torch.equal(got["count"], (wmaps != 0).sum(1).to(torch.int32))
    assert not torch.equal(got["wmax"], plain["wmax"])


# ---- 5, 6: the 3-D filter ------------------------------------------------------------------------------------------------------------------
def test_filter3d_parity_and_reproducibility():
    from siu3r_amd import _lib, mip

    c = A.filter_case()
    ref = A.filter3d64(c["means"], c["c2w"], c["Kn"], c["W"], c["H"])
    assert bool(ref["decided"].all())
    means, c2w, Kn = _dev(c["means"]), _dev(c["c2w"]), _dev(c["Kn"])
    got = mip.compute_filter3d(means, c2w, Kn, c["W"], c["H"])
    again = mip.compute_filter3d(means, c2w, Kn, c["W"], c["H"])
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs give the same bits"
    B.assert_elems_close(got.cpu(), ref["filter"], ref["S"], A.FILTER_BOUND, name="3-D filter")
    unseen = ~ref["seen"].any(0)
    assert int(unseen.sum()) >= 10 and len(set(got.cpu()[unseen].tolist())) == 1, "every unseen row takes the one global maximum"
    assert bool((got > 0).all()) and bool(torch.isfinite(got).all())
    # the entry point itself, guarded; other parameters; nothing seen at all
    out, ws = _f((c["G"],)), torch.empty(int(_lib.lib().siu3r_mip_filter3d_ws(c["V"])) // 4, device="cuda")
    _ok("siu3r_mip_filter3d", _p(c2w), _p(Kn), c["V"], c["W"], c["H"], _p(means), c["G"], 0.2, 0.15, 0.2, _p(out), _p(ws))
    assert out.guards_intact() and torch.equal(out.t.view(torch.int32), got.view(torch.int32))
    ref2 = A.filter3d64(c["means"], c["c2w"], c["Kn"], c["W"], c["H"], z_near=0.5, margin=0.0, variance=0.7)
    got2 = mip.compute_filter3d(means, c2w, Kn, c["W"], c["H"], z_near=0.5, margin=0.0, variance=0.7).cpu()
    B.assert_elems_close(got2[ref2["decided"]], ref2["filter"][ref2["decided"]], ref2["S"][ref2["decided"]], A.FILTER_BOUND, name="3-D filter, other parameters")
    assert int(ref2["decided"].sum()) >= c["G"] - 4 and int(ref2["seen"].any(0).sum()) < int(ref["seen"].any(0).sum())
    behind = c["means"][240:244]
    zeros = mip.compute_filter3d(_dev(behind), c2w, Kn, c["W"], c["H"])
    assert float(zeros.abs().max()) == 0.0, "nothing seen: the filter is all zeros"
    one = mip.compute_filter3d(means[253:254], c2w[:1], Kn[0], c["W"], c["H"])  # (a [3,3] Kn is expanded)
    assert one.shape == (1,) and float(one) > 0


def test_apply_forward_and_backward():
    from siu3r_amd import mip

    c = A.apply_case()
    s, o, f = (_dev(c[k]) for k in ("scales", "opac", "filt"))
    s.requires_grad_()
    o.requires_grad_()
    sf, of = mip.apply_filter3d(s, o, f)
    rsf, rof = A.apply64(c["scales"], c["opac"], c["filt"])
    B.assert_elems_close(sf.detach().cpu(), rsf, rsf.abs(), A.APPLY_S_BOUND, name="apply scales_f")
    B.assert_elems_close(of.detach().cpu(), rof, rof.abs(), A.APPLY_O_BOUND, name="apply opac_f")
    assert float(of[0].detach()) > 0.0, "three tiny ratios: the result is not flushed"
    g_sf, g_of = _dev(c["g_sf"]), _dev(c["g_of"])
    gs, go = torch.autograd.grad([sf, of], [s, o], [g_sf, g_of])
    (rgs, Ss), (rgo, So) = A.apply_bwd64(c["scales"], c["opac"], c["filt"], c["g_sf"], c["g_of"])
    B.assert_elems_close(gs.cpu(), rgs, Ss, A.APPLY_BWD_BOUND, name="apply backward g_scales")
    B.assert_elems_close(go.cpu(), rgo, So, A.APPLY_O_BOUND, name="apply backward g_opac")
    # the raw entry points, guarded
    G = c["G"]
    o_sf, o_of, o_gs, o_go = _f((G, 3)), _f((G,)), _f((G, 3)), _f((G,))
    sd, od = s.detach(), o.detach()
    _ok("siu3r_mip_apply", _p(sd), _p(od), _p(f), G, _p(o_sf), _p(o_of))
    _ok("siu3r_mip_apply_bwd", _p(sd), _p(od), _p(f), _p(g_sf), _p(g_of), G, _p(o_gs), _p(o_go))
    for b, t in ((o_sf, sf), (o_of, of), (o_gs, gs), (o_go, go)):
        assert b.guards_intact() and torch.equal(b.t.view(torch.int32), t.detach().view(torch.int32))
    with pytest.raises(ValueError):
        mip.apply_filter3d(s, o, f[:-1])


# ---- 7: the drop-in ------------------------------------------------------------------------------------------------------------------------
def test_drop_in_antialiasing_field():
    from siu3r_amd import cuda_splatting as cs, raster
    from siu3r_amd.compat.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, make_cam

    Hh, Ww, _, means, cov6, opac, shs = _small_frame()
    c2w = look_at_camera(0)
    fov = cs.get_fov(default_K()[None])
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([0.2]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(c2w)
    base = (Hh, Ww, float(tan[0]), float(tan[1]), torch.tensor([0.1, 0.2, 0.3]), 1.0, w2c.T.contiguous().cuda(), (proj @ w2c).T.contiguous().cuda(), None, 1,
            c2w[:3, 3].cuda(), False, False)
    s_aa, s_off = GaussianRasterizationSettings(*base, antialiasing=True), GaussianRasterizationSettings(*base)
    assert s_off.antialiasing is False
    op = opac.cuda()[:, None].clone().requires_grad_()
    args = dict(means3D=means.cuda(), means2D=None, shs=shs.cuda(), cov3D_precomp=cov6.cuda())
    out = GaussianRasterizer(s_aa)(opacities=op, **args)
    ref = raster.rasterize_views_k2([make_cam(s_aa)], means.cuda(), cov6.cuda(), shs.cuda(), opac.cuda(), antialiased=True)
    off = GaussianRasterizer(s_off)(opacities=op.detach(), **args)
    plain = raster.rasterize_views_k2([make_cam(s_off)], means.cuda(), cov6.cuda(), shs.cuda(), opac.cuda())
    for a, b in ((out[0], ref["image"][0]), (out[2][0], ref["depth"][0]), (out[3][0], ref["opacity"][0]), (out[4], ref["n_touched"][0]),
                 (off[0], plain["image"][0]), (off[3][0], plain["opacity"][0])):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], off[0])
    out[0].sum().backward()
    assert op.grad is not None and float(op.grad.abs().sum()) > 0 and bool(torch.isfinite(op.grad).all())


# ---- 8: refinement -------------------------------------------------------------------------------------------------------------------------
def _refine_job(G=3000):
    from siu3r_amd.refine import covariances_from

    truth = _truth(G=G)
    train, Kt = _cams([0, 1, 2])
    targets = _render(train, Kt, truth["means"], covariances_from(truth["rotations"], truth["scales"]), truth["harmonics"], truth["opacities"])[0]
    g = torch.Generator().manual_seed(5)
    n = lambda *s: torch.randn(*s, generator=g).cuda()
    start = dict(truth)
    start["harmonics"] = truth["harmonics"] + 0.15 * n(G, 3, 4)
    start["opacities"] = torch.sigmoid(torch.logit(truth["opacities"]) + 0.7 * n(G))
    start["scales"] = torch.exp(torch.log(truth["scales"]) + 0.2 * n(G, 3))
    return {k: v.clone() for k, v in start.items()}, targets, train, Kt


def _refine(optimizer, **kw):
    from siu3r_amd.refine import refine_gaussians

    start, targets, c2w, Kn = _refine_job()
    return refine_gaussians(*(start[k] for k in FIELDS), targets, c2w, Kn, NEAR, FAR, BG, iters=kw.pop("iters", 8), optimizer=optimizer, **kw)


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_refinement_without_a_control_is_the_loop_as_it_was(optimizer, monkeypatch):
    """antialias=None against a call without the keyword.  Where the loop is reproducible the bits are compared: the results of iters = 0,
    and the first logged loss (one forward).  Two runs WITHOUT the keyword already differ from the second loss on -- the composite backward
    sums with float atomics -- so there the losses are held to four times that spread (plus eight fp32 roundings of the loss itself, for
    the case that the two plain runs happen to agree), as tests/test_prune_gpu.py does for prune=None, the fields to four times the median
    difference of the two plain runs; and the None run is watched: it calls neither filter function and hands the render no `antialiased`
    keyword."""
    from siu3r_amd import refine

    z0, _ = _refine(optimizer, iters=0)
    z1, _ = _refine(optimizer, iters=0, antialias=None)
    assert set(z0) == set(z1) and "filter_3d" not in z1
    for k in z0:
        assert not torch.is_tensor(z0[k]) or torch.equal(z0[k], z1[k]), f"iters = 0: antialias=None changed {k}"
    (a, la), (a2, la2) = _refine(optimizer), _refine(optimizer)

    def forbidden(*_a, **_k):
        raise AssertionError("antialias=None reached the 3-D filter")

    seen_kw = []
    real_render = refine.render_cuda
    monkeypatch.setattr(refine, "compute_filter3d", forbidden)
    monkeypatch.setattr(refine, "apply_filter3d", forbidden)
    monkeypatch.setattr(refine, "render_cuda", lambda *ar, **kw: (seen_kw.append(sorted(kw)), real_render(*ar, **kw))[1])
    b, lb = _refine(optimizer, antialias=None)
    monkeypatch.undo()
    assert len(seen_kw) == 8 and all("antialiased" not in kw for kw in seen_kw) and seen_kw[0] == ["density_stats", "return_aux"]
    assert set(a) == set(b) and "filter_3d" not in b and len(lb) == 8
    assert la[0] == la2[0] == lb[0], "the first loss is one forward: the same bits"
    spread = max(abs(x - y) for x, y in zip(la, la2))
    worst = max(abs(x - y) for x, y in zip(la, lb))
    print(f"refinement [{optimizer}] losses: two runs without the keyword differ by {spread:.3e}, antialias=None from the first by {worst:.3e}")
    # (a loss is one fp32 number: when the two plain runs happen to agree, a few of its ulps are still no difference of the code path)
    assert worst <= 4 * spread + 8 * U24 * max(la), (la, lb, spread)
    # the fields by their MEDIAN difference: Adam turns the noise of a gradient that is nearly zero into a step of either sign, so the
    # largest difference of two plain runs is set by a handful of elements and says little about a third run
    for k in FIELDS + ("covariances",):
        own, other = float((a[k] - a2[k]).abs().median()), float((a[k] - b[k]).abs().median())
        assert other <= 4 * own + 1e-6 * float(a[k].abs().max()), (k, own, other)


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_refinement_with_the_filters(optimizer):
    from siu3r_amd import mip
    from siu3r_amd.refine import covariances_from

    start, targets, c2w, Kn = _refine_job()
    G = start["means"].shape[0]
    a, la = _refine(optimizer)
    out, losses = _refine(optimizer, antialias=mip.MipFilter())
    assert len(losses) == 8 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    f3 = out["filter_3d"]
    assert f3.shape == (G,) and bool(torch.isfinite(f3).all()) and bool((f3 > 0).all())
    assert torch.equal(f3, mip.compute_filter3d(start["means"], c2w, Kn, W, H)), "every = 100: the filter of the first render's means"
    assert losses[0] != la[0] and bool((out["scales"] > 0).all())
    # the returned covariances are the ones the last render would use: the filtered scales; bake fuses the filter into the fields
    sf, of = mip.apply_filter3d(out["scales"], out["opacities"], f3)
    assert torch.equal(out["covariances"], covariances_from(out["rotations"], sf))
    assert not torch.equal(out["covariances"], covariances_from(out["rotations"], out["scales"]))
    baked = mip.bake(out)
    assert "filter_3d" not in baked and torch.equal(baked["covariances"], out["covariances"]) and torch.equal(baked["scales"], sf) and torch.equal(baked["opacities"], of)
    assert torch.equal(baked["means"], out["means"]) and mip.bake(a) is a
    # each filter alone
    o2, l2 = _refine(optimizer, antialias=mip.MipFilter(filter_3d=False))
    assert "filter_3d" not in o2 and all(np.isfinite(l2)) and l2[-1] < l2[0] and l2[0] != la[0]
    assert torch.equal(o2["covariances"], covariances_from(o2["rotations"], o2["scales"]))
    o3, l3 = _refine(optimizer, antialias=mip.MipFilter(filter_2d=False, every=3))
    assert o3["filter_3d"].shape == (G,) and all(np.isfinite(l3)) and l3[-1] < l3[0]
    assert not torch.equal(o3["filter_3d"], f3), "every = 3: recomputed from means that have moved"
    with pytest.raises(ValueError, match="neither"):
        _refine(optimizer, antialias=mip.MipFilter(filter_2d=False, filter_3d=False))


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_refinement_with_events_and_moving_cameras(optimizer):
    from siu3r_amd import mip
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.density import DensityControl
    from siu3r_amd.prune import ContributionPrune

    start, targets, c2w, Kn = _refine_job()
    G = start["means"].shape[0]
    # density and pruning events change the row count: the filter follows
    dens = DensityControl(grad_threshold=1e-5, start=2, every=3, scene_extent=5.0)
    o4, l4 = _refine(optimizer, antialias=mip.MipFilter(every=4), density=dens, prune=ContributionPrune(min_weight=0.02, start=4, every=2, stop=4, final=True))
    G4 = o4["means"].shape[0]
    assert len(o4["density_events"]) == 2 and len(o4["prune_events"]) == 2 and G4 != G, (G, G4, o4["density_events"], o4["prune_events"])
    assert o4["density_events"][0]["rows_out"] != G and o4["prune_events"][-1]["rows_out"] == G4
    assert o4["filter_3d"].shape == (G4,) and o4["covariances"].shape == (G4, 3, 3) and bool((o4["filter_3d"] > 0).all()) and all(np.isfinite(l4))
    assert torch.equal(o4["covariances"], mip.bake(o4)["covariances"])
    assert torch.equal(o4["filter_3d"], mip.compute_filter3d(o4["means"], c2w, Kn, W, H)), "after the final pruning event: the filter of the kept rows"
    # moving cameras: the filter is computed from the state's poses
    o5, l5 = _refine(optimizer, antialias=mip.MipFilter(every=2), cameras=CameraControl(pose=True, exposure=False, fixed=(0,)))
    assert o5["filter_3d"].shape == (G,) and all(np.isfinite(l5)) and o5["camera_steps"] == 8 and not torch.equal(o5["c2w"], c2w)
    assert bool((o5["filter_3d"] > 0).all())


# ---- 9: error paths ------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    from siu3r_amd import _lib, raster

    c = A.aa_case()
    V, G = c["V"], c["G"]
    st = {}
    fwd, _ = _project(c, "host", 6, aa=True, keep=st)
    d = st["dev"]
    k3 = [raster.make_cam_k3(torch.eye(4), 50.0, 50.0, 32.0, 24.0, c["W"], c["H"]) for _ in range(V)]
    arr3 = raster._cam_array(k3)
    o = dict(rec=_f((V, G, 12)), radii=_Guarded((V, G, 2)), rect=_Guarded((V, G, 4)), tiles=_Guarded((V, G)), keys=_Guarded((V, G)), stats=_Guarded((V, 4), torch.int64),
             comp=_f((V, G)))
    tail = lambda means=d["means"]: [G, _p(means), _p(d["cov"]), 6, _p(d["opac"]), _p(d["colors"]), 1, 0,
                                     *[_p(o[k]) for k in ("rec", "radii", "rect", "tiles", "keys", "stats", "comp")]]
    c2w, Kn = _dev(c["c2w"]), _dev(c["Kn"])
    _refused("siu3r_raster_project_aa", "mode 0", arr3, V, _p(st["cams_dev"]), *tail())
    _refused("siu3r_raster_project_c2w_aa", "mode 0", arr3, V, _p(st["cams_dev"]), _p(c2w), _p(Kn), 1.0, *tail())
    _refused("siu3r_raster_project_aa", "null per-Gaussian pointer", st["arr"], V, _p(st["cams_dev"]), *tail(means=None))
    c2w_cams, _ = _cams_for(c, "c2w")
    _refused("siu3r_raster_project_c2w_aa", "null pose pointer", raster._cam_array(c2w_cams), V, _p(st["cams_dev"]), None, _p(Kn), 1.0, *tail())
    for b in o.values():
        assert b.untouched(), "a refused call wrote an output"
    g = [_f((G, 3)), _f((G, 6)), _f((G,)), _f((G, 1, 3))]
    bwd = lambda arr=st["arr"], grad=_dev(c["grad"]): [arr, V, _p(st["cams_dev"]), G, _p(d["means"]), _p(d["cov"]), 6, _p(d["opac"]), _p(d["colors"]), 1, 0,
                                                       _p(d["rect"]), _p(grad), *[_p(x) for x in g], None, None]
    _refused("siu3r_raster_project_bwd_aa", "mode 0", *bwd(arr=arr3))
    _refused("siu3r_raster_project_bwd_aa", "null pointer", *bwd(grad=None))
    for b in g:
        assert b.untouched()
    ws = torch.empty(int(_lib.lib().siu3r_mip_filter3d_ws(V)) // 4, device="cuda")
    out = _f((G,))
    _refused("siu3r_mip_filter3d", "null pointer", _p(c2w), _p(Kn), V, c["W"], c["H"], None, G, 0.2, 0.15, 0.2, _p(out), _p(ws))
    _refused("siu3r_mip_filter3d", "null pointer", _p(c2w), _p(Kn), V, c["W"], c["H"], _p(d["means"]), G, 0.2, 0.15, 0.2, _p(out), None)
    _refused("siu3r_mip_filter3d", "variance", _p(c2w), _p(Kn), V, c["W"], c["H"], _p(d["means"]), G, 0.2, 0.15, 0.0, _p(out), _p(ws))
    _refused("siu3r_mip_filter3d", "bad view count", _p(c2w), _p(Kn), 0, c["W"], c["H"], _p(d["means"]), G, 0.2, 0.15, 0.2, _p(out), _p(ws))
    _refused("siu3r_mip_apply", "null pointer", _p(d["means"]), None, _p(d["opac"]), G, _p(g[0]), _p(out))
    _refused("siu3r_mip_apply_bwd", "null pointer", _p(d["means"]), _p(d["opac"]), _p(d["opac"]), None, _p(d["opac"]), G, _p(g[0]), _p(out))
    assert out.untouched() and g[0].untouched()
    with pytest.raises(ValueError, match="K3"):
        raster.rasterize_views_k2(k3, d["means"], d["cov"], d["colors"], d["opac"], antialiased=True)
    with pytest.raises(ValueError, match="K3"):
        raster.contributions_k2(k3, d["means"], d["cov"], d["opac"], antialiased=True)
