"""Every stage of the two rasterizer backward passes (siu3r_amd/csrc/raster_bwd.hip, raster_bwd_k3.hip, raster_bwd_shared.h) called
directly through the C ABI on the crafted cases of tests/dense_raster_bwd64.py and held, element by element, to its float64 reference:
|got - ref| <= bound * S, for the composite stages + the derived error of the element's alpha / transmittance chains, with the bounds
and scales derived in that file's header (and proved on the CPU by tests/test_raster_bwd_stages_ref.py: the references against finite
differences and autograd of the dense renders, the metric against answers with one branch wrong, every case's branch population).
Every output lies inside a sentinel-filled parent (_Guarded of tests/test_raster_stages_gpu.py): guards stay intact and rows the
contract leaves alone keep the fill.

The composite stages compare two walks that must take the same branch at every pixel; a pixel within MARGIN derived errors of a threshold
gets an upstream gradient of exactly 0 (the kernels drop such pixels by design), at most 1 % of a case's pixels.  The crafted composite
cases hand the stages records, bins and lists made on the CPU (screen-space records with the branches placed by hand, binned by
tests/raster_stages_ref.py; only the composite forward runs, for the saved totals);
test_composite_backward_on_the_state_of_a_real_forward runs the same comparison on the state siu3r_raster_project, sort and bin left.

Where a line is run (case names as in PROJ_CASES / COMP_CASES):

  composite_rgb_bwd_kernel
    inside / K3 load                      k2_* (planar maps, depth), k3_full (channel-last, no depth); k2_ragged, k3_full: pixels off the frame
    done = no upstream gradient           every case (margin pixels); depth_only / alpha_only / one_colour modes
    base >= eend, second staging slice    *_full: 280 + entries of bin 0 on tile (0, 0); the empty last tile
    eend = min(bin_start, cap_e)          the clamp is never taken: cap_e > E in every case.  A view whose entries overflow cap_e is NaN in
                                          the forward and the front-end repeats the call before any backward (raster._with_retry)
    pass = entry_covers                   *_full: bin 0 holds entries that do not cover tile (0, 0)
    s_m & wbit (quadrant mask)            every case (small splats); opacity 0.003 rows: mask 0
    power > 0                             the sixteen indefinite conics of every full / small scene
    a < alpha_min, sat (< / <=)           every case; the opaque stacks (entries behind a saturated pixel)
    Q.w * ex > alpha_max                  the opacity 0.999 (mode 1: 0.9995) rows: pixels on and off the clamp for the same Gaussian
    ballot(gv[k] != 0) == 0               depth_only, alpha_only, one_colour: the skipped terms are exactly 0.0
    lane == 0 && s != 0 (LDS add)         depth_only / alpha_only / one_colour (a wave whose sum of a term is exactly 0: the term's upstream is 0)
    s != 0 global add                     rows of culled Gaussians and of opacity 0.003 stay 0
  composite_feat_bwd_kernel
    load4 aligned / tail, chn < C         feat_c1, c3, c5, c21 (feat_full), c32, c33 (feat_qlen), c63, c64, c168
    k0 + lane < n (padding reads rec 0)   feat_qlen: lists of 0, 1, 31, 32, 33, 70; Gaussian 0 heavy in every scene
    sigma >= 0, alpha_min, sat, alpha_max as above (feat_full, feat_c*)
    !any_w                                feat_qlen: forty slivers in the box of a quadrant none of whose pixels they reach
    k0 + i < n on the g_feats add         feat_qlen: the last chunk of the lists of 1, 31, 33 and 70 entries blends (any_w) and is partly
                                          padding (Gaussian 0's row, heavy in the scene, must get nothing from it)
    ballot(aw != 0) == 0                  every feat case (pixel pairs that blend nothing in a chunk)
  project_bwd_kernel / project_bwd_k3_kernel
    live, rect empty                      G = 1, 255, 256, 257; V = 3 with rows culled in some views, in all views
    g_mean2d / pose_part null             k2_deg1_planar, k2_deg4_band4 (no mean2d); k2_deg2_wide, k2_deg4_band4, k3_views (no pose)
    cxz == txz, cyz == tyz                clamp classes none / x+ / x- / y+ / y- / both, >= 8 rows each, tanfovx != tanfovy, cx, cy off centre
    sh_degree < 0                         k2_precomputed
    tri / [3,3]                           stride 6 and 9 (lower triangle of the input NaN, of the output exactly 0)
    sh_planar, q < channels * 3           k2_deg1_planar, k2_deg4_no_band4; k2_deg2_wide (16 coefficients at degree 2)
    g_colors (k3) null                    k3_views
  sh_color_bwd / sh_basis                 degrees 0 .. 4, band4 on and off, 0 .. 3 channels clamped at 0 (>= 8 rows each)
  block_sum_row, rows_reduce_kernel       1 partial row (G <= 256), 2 (G = 257), 257 and 1000 synthetic rows
  quat_scale_cov6_bwd_kernel              |q| from 1e-2 to 1e2, w < 0, G = 1 and 257
  sh_eval_bwd_kernel                      degrees 0 .. 4, 25 coefficients at a lower degree (tail exactly 0), clamped channels, g_campos over 3 workgroups
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dense_raster_bwd64 as B
import dense_raster_fwd64 as F
from test_raster_stages_gpu import SENT, _Guarded

pytestmark = pytest.mark.gpu
U24 = B.U24


def _f(shape):
    return _Guarded(shape, torch.float32)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).contiguous().cuda()


def _cam_blocks(cams):
    """the host array and its device copy (what siu3r_raster_project leaves in cams_dev)"""
    from siu3r_amd import raster

    arr = raster._cam_array(cams)
    assert raster.geometry(cams[0].width, cams[0].height, 1)["cam_bytes"] == C.sizeof(cams[0])
    return arr, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _call(name, *args):
    from siu3r_amd import _lib
    from siu3r_amd.ops import _stream

    rc = getattr(_lib.lib(), name)(*args, _stream())
    torch.cuda.synchronize()
    return rc


def _ok(name, *args):
    from siu3r_amd import _lib

    _lib.check(_call(name, *args), name)


def _p(t):
    return None if t is None else (t.t if isinstance(t, _Guarded) else t).data_ptr()


def _close(got, ref, S, bound, name, extra=None):
    """assert_elems_close; with SIU3R_RASTER_BWD_PARITY_LOG=file one JSON line per comparison: the largest |got - ref| / S (the plain
    S), the worst element as a fraction of its tolerance, and the tolerance itself as a multiple of S (median and largest element):
    tools/raster_bwd_parity.py groups the lines into profiles/raster_bwd_parity.json"""
    got = got.detach().cpu() if torch.is_tensor(got) else got
    w = B.assert_elems_close(got, ref, S, bound, name=name, extra=extra)
    if os.environ.get("SIU3R_RASTER_BWD_PARITY_LOG"):
        med, mx = B.effective_bound(ref, S, bound, extra)
        with open(os.environ["SIU3R_RASTER_BWD_PARITY_LOG"], "a") as f:
            f.write(json.dumps({"case": name, "max_err_over_S": B.observed(got, ref, S), "worst_ratio_to_bound": w, "bound_over_S_median": med,
                                "bound_over_S_max": mx}) + "\n")
    return w


# ---- projection backward ----------------------------------------------------------------------------------------------------------------
def _run_projection(c):
    mode, V, G = c["mode"], c["V"], c["G"]
    arr, cams_dev = _cam_blocks(c["cams"])
    means, opac, rect, grad = _dev(c["means"]), _dev(c["opac"]), _dev(c["rect"]), _dev(c["grad"])
    if c["stride"] == 6:
        cov = _dev(c["cov6"])
    else:  # [G,3,3]: the upper triangle; the entries the kernels must not read are NaN
        cov = torch.full((G, 9), float("nan"))
        cov[:, [0, 1, 2, 4, 5, 8]] = c["cov6"]
        cov = cov.cuda()
    out = dict(g_means=_f((G, 3)), g_cov=_f((G, c["stride"])), g_opac=_f((G,)))
    rows = -(-G // 256)
    from siu3r_amd import _lib

    assert int(_lib.lib().siu3r_raster_pose_partial_rows(G)) == rows
    if mode == 0:
        col = c["colors"]
        if c["planar"]:
            full = torch.zeros((G, 25, 3))
            full[:, :col.shape[1]] = col
            colors, channels = full.permute(0, 2, 1).contiguous().cuda(), 25
        else:
            colors, channels = col.cuda(), col.shape[1]
        out["g_colors"] = _f(tuple(colors.shape))
        out["g_mean2d"] = _f((V, G, 2)) if c["m2d"] else None
        out["part"] = _f((rows, V, 6)) if c["pose"] else None
        _ok("siu3r_raster_project_bwd", arr, V, _p(cams_dev), G, _p(means), _p(cov), c["stride"], _p(opac), _p(colors), channels, int(c["planar"]), _p(rect),
            _p(grad), _p(out["g_means"]), _p(out["g_cov"]), _p(out["g_opac"]), _p(out["g_colors"]), _p(out["g_mean2d"]), _p(out["part"]))
    else:
        out["g_colors"] = _f((G, 3)) if c["colors"] is not None else None
        out["part"] = _f((rows, V, 12)) if c["pose"] else None
        _ok("siu3r_raster_project_bwd_k3", arr, V, _p(cams_dev), G, _p(means), _p(cov), c["stride"], _p(rect), _p(grad), _p(out["g_means"]), _p(out["g_cov"]),
            _p(out["g_opac"]), _p(out["g_colors"]), _p(out["part"]))
    return out


@pytest.mark.parametrize("name", list(B.PROJ_CASES))
def test_projection_backward(name):
    c, ref = B.proj_case(name), B.proj_ref(name)
    mode, V, G = c["mode"], c["V"], c["G"]
    out = _run_projection(c)
    for k, b in out.items():
        assert b is None or b.guards_intact(), f"{k}: written outside the buffer"
    _close(out["g_means"].t, *ref["g_means"], B.PROJ_BOUND, f"{name} g_means")
    _close(out["g_opac"].t, *ref["g_opac"], B.PROJ_BOUND, f"{name} g_opac")
    gc = out["g_cov"].t.cpu()
    if c["stride"] == 9:
        assert float(gc[:, [3, 6, 7]].abs().max()) == 0.0, "the lower triangle gets exactly 0"
        gc = gc[:, [0, 1, 2, 4, 5, 8]]
    _close(gc, *ref["g_cov"], B.PROJ_BOUND, f"{name} g_cov")
    if out["g_colors"] is not None:
        got = out["g_colors"].t.cpu()
        want, S = ref["g_colors"]
        if c["planar"]:
            got = got.permute(0, 2, 1)
            pad = lambda t: torch.cat([t, torch.zeros((G, 25 - t.shape[1], 3), dtype=t.dtype)], 1)
            want, S = pad(want), pad(S)
        got = got.reshape(want.shape)
        _close(got, want, S, B.PROJ_BOUND, f"{name} g_colors")
        assert not bool((got[want == 0] != 0).any()), "a clamped channel, an unused coefficient or a culled row gets exactly 0"
        if mode == 0 and c["deg"] >= 0:
            used = (c["deg"] + 1) ** 2 if c["deg"] < 4 or c["cams"][0].sh_band4 else 16
            assert float(got[:, used:].abs().max() if got.shape[1] > used else 0.0) == 0.0, "coefficients the polynomial does not use get exactly 0"
    if mode == 0 and out["g_mean2d"] is not None:
        want, _, live = ref["g_mean2d"]
        got = out["g_mean2d"].t.cpu()
        assert torch.equal(got[live], want.float()[live]), "g_mean2d is a copy of the record's mean gradient"
        assert bool((got[~live] == SENT).all()), "g_mean2d rows of culled Gaussians are left alone"
    if out["part"] is not None:
        n = 6 if mode == 0 else 12
        want, S = B.partial_rows64(*ref["pose_g"], n) if mode == 0 else B.partial_rows64(ref["pose_g"][0][:, :, :3].reshape(V, G, 12), ref["pose_g"][1][:, :, :3].reshape(V, G, 12), n)
        part = out["part"].t
        _close(part, want, S, B.PROJ_BOUND + 9 * U24, f"{name} pose partial rows")
        g_pose = _f((V, 6 if mode == 0 else 16))
        _ok("siu3r_raster_pose_reduce" if mode == 0 else "siu3r_raster_viewmat_reduce", V, part.shape[0], _p(part), _p(g_pose))
        assert g_pose.guards_intact()
        r_out, r_S, r_b = B.rows_reduce64(part.cpu(), 6 if mode == 0 else 16)
        _close(g_pose.t, r_out, r_S, r_b, f"{name} reduce of the partial rows")
        pv, pS = ref["pose"]
        _close(g_pose.t.reshape(pv.shape), pv, pS, B.PROJ_BOUND + 9 * U24 + r_b, f"{name} pose")
        if mode == 1:
            assert float(g_pose.t.reshape(V, 4, 4)[:, 3].abs().max()) == 0.0, "the fourth row of d loss / d viewmat is exactly 0"


@pytest.mark.parametrize("nrows", [1, 257, 1000])
def test_rows_reduce_on_synthetic_partial_rows(nrows):
    """rows_reduce_kernel's strided loop past 256 rows, without a scene of 65 537 Gaussians"""
    V = 3
    g = torch.Generator().manual_seed(nrows)
    for n, n_out, fn in ((6, 6, "siu3r_raster_pose_reduce"), (12, 16, "siu3r_raster_viewmat_reduce")):
        part = (torch.randn(nrows, V, n, generator=g) * torch.logspace(-3, 3, nrows)[:, None, None]).cuda()
        out = _f((V, n_out))
        _ok(fn, V, nrows, _p(part), _p(out))
        assert out.guards_intact()
        want, S, b = B.rows_reduce64(part.cpu(), n_out)
        _close(out.t, want, S, b, f"{fn} {nrows} rows")
        assert float(out.t[:, n:].abs().max() if n_out > n else 0.0) == 0.0


# ---- composite backward -----------------------------------------------------------------------------------------------------------------
def _composite_state(c):
    """device buffers of a composite case: camera blocks, records, bins (k2 / k3) or tile lists + quadrant workspace (feat)"""
    V, G, geo = c["V"], c["G"], c["geo"]
    arr, cams_dev = _cam_blocks(c["cams"])
    st = dict(arr=arr, cams_dev=cams_dev, rec=_dev(c["rec"]))
    if c["kind"] != "feat":
        E = [len(b[1]) for b in c["bins"]]
        cap_e = max(E) + 7
        bs = torch.stack([torch.from_numpy(b[0].astype(np.int32)) for b in c["bins"]]).cuda()
        ent = torch.full((V, cap_e, 2), SENT, dtype=torch.int32)
        for v, b in enumerate(c["bins"]):
            ent[v, :E[v]] = torch.from_numpy(b[1])
        st.update(bin_start=bs, entries=ent.cuda(), cap_e=cap_e)
    else:
        D = [len(l[1]) for l in c["lists"]]
        cap_d = max(D) + 5
        ts = torch.zeros((V, geo["T"] + 2), dtype=torch.int32)
        ids = torch.full((V, cap_d), SENT, dtype=torch.int32)
        for v, l in enumerate(c["lists"]):
            ts[v, :geo["T"] + 1] = torch.from_numpy(l[0].astype(np.int32))
            ts[v, geo["T"] + 1] = D[v]
            ids[v, :D[v]] = torch.from_numpy(l[1])
        st.update(tile_start=ts.cuda(), ids=ids.cuda(), cap_d=cap_d, feats=_dev(c["feats"]))
    return st


def _forward_totals(c, st):
    V, G, H, W, Cc = c["V"], c["G"], c["H"], c["W"], c["C"]
    f = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    if c["kind"] == "k2":
        image, depth, alpha = f(V, 3, H, W), f(V, H, W), f(V, H, W)
        _ok("siu3r_raster_composite_rgb", st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(image), _p(depth),
            _p(alpha), None)
        return image, depth, alpha
    if c["kind"] == "k3":
        image, alpha = f(V, H, W, 3), f(V, H, W)
        _ok("siu3r_raster_composite_rgb", st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(image), None,
            _p(alpha), None)
        return image, None, alpha
    out, alpha = f(V, H, W, Cc), f(V, H, W)
    _ok("siu3r_raster_composite_feat", st["arr"], V, _p(st["cams_dev"]), G, _p(st["tile_start"]), _p(st["ids"]), st["cap_d"], _p(st["rec"]), _p(st["feats"]), Cc, _p(out),
        _p(alpha))
    return out, None, alpha


COMP_RUNS = [(n, "all") for n in B.COMP_CASES] + [("k2_ragged", m) for m in B.COMP_MODES[1:]] + [("k3_full", "alpha_only"), ("k3_full", "one_colour"),
                                                                                               ("feat_full", "alpha_only")]


def _run_composite_bwd(kind, V, G, H, W, Cc, T, st, totals, ups):
    """the composite backward of `kind` on the device state st (camera blocks, records, bins or tile lists) -> grad, g_feats, qcnt"""
    from siu3r_amd import _lib

    out, depth, alpha = totals
    grad = _f((V, G, 10))
    g_out, g_alpha, g_depth = _dev(ups["g_out"]), _dev(ups["g_alpha"]), _dev(ups["g_depth"])
    g_feats = qcnt = None
    if kind == "k2":
        _ok("siu3r_raster_composite_rgb_bwd", st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(out),
            _p(depth), _p(alpha), _p(g_out), _p(g_depth), _p(g_alpha), _p(grad))
    elif kind == "k3":
        _ok("siu3r_raster_composite_rgb_bwd_k3", st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(out),
            _p(alpha), _p(g_out), _p(g_alpha), _p(grad))
    else:
        nbytes = int(_lib.lib().siu3r_raster_composite_feat_ws_bytes(W, H, V, st["cap_d"]))
        ws = _Guarded((nbytes // 4,))
        _ok("siu3r_raster_quad_lists", st["arr"], V, _p(st["cams_dev"]), G, _p(st["tile_start"]), _p(st["ids"]), st["cap_d"], _p(st["rec"]), _p(ws), nbytes)
        assert ws.guards_intact()
        qcnt = ws.t[V * 4 * st["cap_d"]:V * 4 * st["cap_d"] + V * T * 4].view(V, T, 4).cpu().numpy()
        g_feats = _f((G, Cc))
        _ok("siu3r_raster_composite_feat_bwd", st["arr"], V, _p(st["cams_dev"]), G, _p(st["tile_start"]), _p(ws), st["cap_d"], _p(st["rec"]), _p(st["feats"]), Cc,
            _p(out), _p(alpha), _p(g_out), _p(g_alpha), _p(grad), _p(g_feats))
        assert g_feats.guards_intact() and ws.guards_intact()
    assert grad.guards_intact()
    return grad, g_feats, qcnt


def _check_composite(name, kind, Cc, refs, low, totals, grad, g_feats, case):
    # the state is the one the reference walked: the forward's maps (the backward's saved totals), depth included, are held element by
    # element to the derived forward bound of tests/dense_raster_fwd64.py (a pixel below the margin may blend one entry more or less)
    out, depth, alpha = totals
    o = out.cpu().numpy()
    F.check_maps(f"{name} forward", kind, F.comp_fwd_ref(case, Cc if kind == "feat" else None), o.transpose(0, 2, 3, 1) if kind == "k2" else o, alpha.cpu().numpy(),
                 depth.cpu().numpy() if kind == "k2" else None)
    got = grad.t.cpu()
    for v, r in enumerate(refs):
        _close(got[v], r["grad"], r["S"], r["bound"], f"{name} view {v} grad", r["chain"])
        assert not bool((got[v][r["n_add"] == 0] != 0).any()), "a Gaussian that blends nowhere gets exactly 0"
    if g_feats is not None:
        ref_f, S_f, n_f = (sum(r[k] for r in refs) for k in ("g_feats", "S_feats", "n_add"))
        _close(g_feats.t, ref_f, S_f, B.comp_bound(n_f, Cc)[:, None], f"{name} g_feats", sum(r["chain_feats"] for r in refs))


@pytest.mark.parametrize("name,mode", COMP_RUNS)
def test_composite_backward(name, mode):
    c = B.comp_case(name)
    kind, V, G, H, W, Cc = c["kind"], c["V"], c["G"], c["H"], c["W"], c["C"]
    refs, ups = B.comp_ref(c, mode)
    low = c["margins"] < B.MARGIN
    assert low.reshape(V, -1).mean(1).max() <= B.ZERO_SHARE_CAP, "more than 1 % of a view's pixels are zeroed"
    st = _composite_state(c)
    with torch.no_grad():
        totals = _forward_totals(c, st)
    grad, g_feats, qcnt = _run_composite_bwd(kind, V, G, H, W, Cc, c["geo"]["T"], st, totals, ups)
    if name == "feat_qlen":  # the quadrant lists the case is for
        lens = set(qcnt.reshape(-1).tolist())
        assert {0, 1, 31, 32, 33}.issubset(lens) and max(lens) > 64, sorted(lens)
        ql = B.quadrant_lists_ref(c["cams"][0], c["rec"][0], c["lists"][0])
        assert qcnt[0, 3 * 6 + 3, 0] == len(ql[(3 * 6 + 3, 0)]) >= 40, "the slivers are not on the quadrant's list"
    _check_composite(f"{name} {mode}", kind, Cc, refs, low, totals, grad, g_feats, c)


@pytest.mark.parametrize("kind", ["k2", "k3", "feat"])
def test_composite_backward_on_the_state_of_a_real_forward(kind):
    """the crafted cases hand the composite stages records and lists made on the CPU; here the state is the forward's own: records as
    siu3r_raster_project wrote them, its sort, its bins (k2, k3) or its tile lists (feat), two views of 800 projected Gaussians"""
    import raster_stages_ref as RS
    from siu3r_amd import raster

    sc = B.forward_scene(kind)
    cams, V, G, H, W, Cc = sc["cams"], len(sc["cams"]), sc["means"].shape[0], sc["H"], sc["W"], sc["C"]
    m, cov, op, col = (_dev(sc[k]) for k in ("means", "cov6", "opac", "colors"))
    with torch.no_grad():
        if kind == "k2":
            o = raster.rasterize_views_k2(cams, m, cov, col, op)
            totals = (o["image"], o["depth"], o["opacity"])
        else:
            o = raster.rasterize_views_k3_rgb(cams, m, cov, op, col) if kind == "k3" else raster.rasterize_views_k3(cams, m, cov, op, col)
            totals = (o["colors"], None, o["alphas"])
    fs = o["state"]
    geo = RS.geometry_ref(W, H)
    st = dict(arr=fs["cams"], cams_dev=fs["cams_dev"], rec=fs["rec"])
    if kind == "feat":
        ts = fs["tile_start_all"].cpu().numpy()
        lists = [(ts[v, :geo["T"] + 1], fs["ids_all"][v, :ts[v, geo["T"] + 1]].cpu().numpy()) for v in range(V)]
        st.update(tile_start=fs["tile_start_all"], ids=fs["ids_all"], cap_d=fs["cap_d"], feats=col)
    else:
        E = fs.totals(2)
        lists = [RS.tile_lists_ref(geo, fs["bin_start"][v].cpu().numpy(), fs["entries"][v, :E[v]].cpu().numpy()) for v in range(V)]
        st.update(bin_start=fs["bin_start"], entries=fs["entries"], cap_e=fs["cap_e"])
    assert min(len(l[1]) for l in lists) > 1000 and int((fs["tiles_touched_all"] == 0).sum()) > 0, "the scene left the frame, or nothing was culled"
    g = np.random.default_rng(7)
    case = dict(kind=kind, V=V, H=H, W=W, cams=cams, rec=fs["rec"].cpu().numpy(), lists=lists, feats=sc["colors"].numpy() if kind == "feat" else None,
                walk_cache=[{} for _ in range(V)],
                ups=dict(g_out=g.normal(size=(V, 3, H, W) if kind == "k2" else (V, H, W, Cc)).astype(np.float32),
                         g_alpha=g.normal(size=(V, H, W)).astype(np.float32), g_depth=g.normal(size=(V, H, W)).astype(np.float32)))
    refs, ups = B.comp_ref(case)
    low = case["margins"] < B.MARGIN
    assert low.reshape(V, -1).mean(1).max() <= B.ZERO_SHARE_CAP, "more than 1 % of a view's pixels are zeroed"
    assert kind != "k2" or sum(r["counts"]["clamped"] for r in refs) > 0, "no alpha on the clamp"
    grad, g_feats, _ = _run_composite_bwd(kind, V, G, H, W, Cc, geo["T"], st, totals, ups)
    _check_composite(f"forward_{kind}", kind, Cc, refs, low, totals, grad, g_feats, case)


# ---- viewer helpers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 257])
def test_quat_scale_to_cov6_backward(G):
    g = torch.Generator().manual_seed(G)
    q = torch.randn(G, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * torch.logspace(-2, 2, G)[:, None] if G > 1 else q * 37.0
    q[::2, 0] = -q[::2, 0].abs()  # negative w
    s, g6 = torch.rand(G, 3, generator=g) * 2 + 0.05, torch.randn(G, 6, generator=g)
    gq, gs = _f((G, 4)), _f((G, 3))
    dq, ds, dg = _dev(q), _dev(s), _dev(g6)
    _ok("siu3r_quat_scale_to_cov6_bwd", _p(dq), _p(ds), _p(dg), _p(gq), _p(gs), G)
    assert gq.guards_intact() and gs.guards_intact()
    (rq, Sq), (rs, Ss) = B.quat_scale_cov6_bwd64(q, s, g6)
    _close(gq.t, rq, Sq, B.QUAT_BOUND, f"quat G={G} g_quats")
    _close(gs.t, rs, Ss, B.QUAT_BOUND, f"quat G={G} g_scales")


@pytest.mark.parametrize("degree,ncoef,G", [(0, 1, 1), (1, 4, 257), (2, 25, 700), (3, 16, 257), (4, 25, 700), (0, 25, 257)])
def test_sh_eval_backward(degree, ncoef, G):
    g = torch.Generator().manual_seed(10 * degree + ncoef)
    m, cp = torch.randn(G, 3, generator=g), torch.tensor([0.1, -0.2, 3.0])
    sh = torch.randn(G, ncoef, 3, generator=g) * 0.2
    ncl = torch.arange(G) % 4
    sh[:, 0, :] = torch.where(torch.arange(3)[None] < ncl[:, None], -6.0, 2.0)  # 0 .. 3 channels clamped at 0
    g3 = torch.randn(G, 3, generator=g)
    (rsh, Ssh), (rm, Sm), (rc, Sc), lin = B.sh_eval_bwd64(m, cp, sh, degree, g3)
    assert float(lin.abs().min()) > 1e-3 and (G < 4 or all(int(((lin < 0).sum(-1) == k).sum()) >= 1 for k in range(4)))
    gsh, gm, gc = _f((G, ncoef, 3)), _f((G, 3)), _f((3,))
    dm, dcp, dsh, dg3 = _dev(m), _dev(cp), _dev(sh), _dev(g3)
    _ok("siu3r_sh_eval_bwd", _p(dm), _p(dcp), _p(dsh), ncoef, degree, _p(dg3), _p(gsh), _p(gm), _p(gc), G)
    assert gsh.guards_intact() and gm.guards_intact() and gc.guards_intact()
    name = f"sh_eval degree {degree} ncoef {ncoef} G {G}"
    _close(gsh.t, rsh, Ssh, B.SH_BOUND, name + " g_sh")
    assert float(gsh.t[:, (degree + 1) ** 2:].abs().max() if ncoef > (degree + 1) ** 2 else 0.0) == 0.0, "coefficients past the degree get exactly 0"
    _close(gm.t, rm, Sm, B.SH_BOUND, name + " g_means")
    _close(gc.t, rc, Sc, B.SH_BOUND + (9 + -(-G // 256)) * U24, name + " g_campos")


# ---- error paths: refused in front of every launch, nothing written ---------------------------------------------------------------------
def _refused(name, match, *args, outs=()):
    from siu3r_amd import _lib

    assert _call(name, *args) != 0, f"{name} accepted a call it documents as an error"
    assert match in _lib.lib().siu3r_last_error().decode(), _lib.lib().siu3r_last_error().decode()
    for o in outs:
        assert o.untouched(), f"{name}: a refused call wrote its output"


def test_error_paths_of_the_projection_stages():
    c = B.proj_case("k2_deg2_wide")
    k3 = B.proj_case("k3_two")
    G = c["G"]
    arr, cd = _cam_blocks(c["cams"])
    arr3, cd3 = _cam_blocks(k3["cams"])
    m, cov, op, col, rect, grad = (_dev(c[k]) for k in ("means", "cov6", "opac", "colors", "rect", "grad"))
    o = [_f((G, 3)), _f((G, 6)), _f((G,)), _f((G, 16, 3))]
    P = lambda *a: [_p(x) for x in a]
    base = lambda **kw: [kw.get("arr", arr), kw.get("V", 1), _p(cd), kw.get("G", G), *P(m, cov), kw.get("stride", 6), *P(op, kw.get("col", col)), kw.get("ch", 16),
                         kw.get("planar", 0), *P(rect, grad), *P(*o), None, None]
    for match, kw in (("mode 0", dict(arr=arr3)), ("bad view array", dict(V=0)), ("out of range", dict(G=-1)), ("cov_stride", dict(stride=7)),
                      ("planar", dict(planar=1)), ("1 .. 25", dict(ch=26)), ("1 .. 25", dict(ch=0)), ("do not match sh_degree", dict(ch=4))):
        _refused("siu3r_raster_project_bwd", match, *base(**kw), outs=o)
    a = base()
    a[4] = None
    _refused("siu3r_raster_project_bwd", "null pointer", *a, outs=o)
    pre = B.proj_case("k2_precomputed")
    arrp, _ = _cam_blocks(pre["cams"][:1])
    _refused("siu3r_raster_project_bwd", "do not match sh_degree", *base(arr=arrp, ch=16), outs=o)
    b3 = lambda **kw: [kw.get("arr", arr3), kw.get("V", 1), _p(cd3), kw.get("G", G), *P(m, cov), kw.get("stride", 6), *P(rect, grad), *P(*o[:3]), None, None]
    for match, kw in (("mode 1", dict(arr=arr)), ("bad view array", dict(V=70000)), ("out of range", dict(G=1 << 31)), ("cov_stride", dict(stride=3))):
        _refused("siu3r_raster_project_bwd_k3", match, *b3(**kw), outs=o[:3])
    a = b3()
    a[7] = None
    _refused("siu3r_raster_project_bwd_k3", "null pointer", *a, outs=o[:3])
    part, gp = _dev(torch.zeros(2, 1, 12)), _f((16,))
    for fn in ("siu3r_raster_pose_reduce", "siu3r_raster_viewmat_reduce"):
        _refused(fn, "bad arguments", 0, 2, _p(part), _p(gp), outs=[gp])
        _refused(fn, "bad arguments", 1, 2, None, _p(gp), outs=[gp])
        _refused(fn, "bad arguments", 1, -1, _p(part), _p(gp), outs=[gp])
        _refused(fn, "bad arguments", 1, 2, _p(part), None)


def test_error_paths_of_the_composite_stages():
    from siu3r_amd import _lib

    c, f = B.comp_case("k2_ragged"), B.comp_case("feat_c5")
    st, sf = _composite_state(c), _composite_state(f)
    V, G, H, W = 1, c["G"], c["H"], c["W"]
    z = lambda *s: torch.zeros(s, device="cuda")
    img, dep, alp = z(V, 3, H, W), z(V, H, W), z(V, H, W)
    grad = _f((V, G, 10))
    arr3, _ = _cam_blocks(f["cams"])
    P = lambda *a: [_p(x) for x in a]
    k2 = lambda **kw: [kw.get("arr", st["arr"]), kw.get("V", 1), _p(st["cams_dev"]), kw.get("G", G), *P(st["bin_start"], st["entries"]), kw.get("cap_e", st["cap_e"]),
                       _p(st["rec"]), *P(img, kw.get("dep", dep), alp, img, dep, alp), _p(grad)]
    for match, kw in (("mode 0", dict(arr=arr3)), ("bad view array", dict(V=0)), ("bad sizes", dict(G=-1)), ("bad sizes", dict(cap_e=0)), ("null pointer", dict(dep=None))):
        _refused("siu3r_raster_composite_rgb_bwd", match, *k2(**kw), outs=[grad])
    k3 = lambda **kw: [kw.get("arr", arr3), 1, _p(st["cams_dev"]), G, *P(st["bin_start"], st["entries"]), kw.get("cap_e", st["cap_e"]), _p(st["rec"]),
                       *P(kw.get("img", img), alp, img, alp), _p(grad)]
    for match, kw in (("mode 1", dict(arr=st["arr"])), ("bad sizes", dict(cap_e=-3)), ("null pointer", dict(img=None))):
        _refused("siu3r_raster_composite_rgb_bwd_k3", match, *k3(**kw), outs=[grad])
    Gf, Cf = f["G"], f["C"]
    nbytes = int(_lib.lib().siu3r_raster_composite_feat_ws_bytes(f["W"], f["H"], 1, sf["cap_d"]))
    ws = _Guarded((nbytes // 4 + 1,))
    ql = lambda **kw: [kw.get("arr", arr3), 1, _p(sf["cams_dev"]), Gf, *P(sf["tile_start"], sf["ids"]), kw.get("cap_d", sf["cap_d"]), _p(sf["rec"]),
                       kw.get("ws", _p(ws)), kw.get("nbytes", nbytes)]
    for match, kw in (("mode 1", dict(arr=st["arr"])), ("workspace too small", dict(nbytes=64)), ("workspace too small", dict(cap_d=0)),
                      ("bad arguments", dict(ws=_p(ws) + 2)), ("bad arguments", dict(ws=None))):
        _refused("siu3r_raster_quad_lists", match, *ql(**kw), outs=[ws])
    gf, gr = _f((Gf, Cf)), _f((1, Gf, 10))
    out, oa = z(1, f["H"], f["W"], Cf), z(1, f["H"], f["W"])
    fb = lambda **kw: [kw.get("arr", arr3), 1, _p(sf["cams_dev"]), kw.get("G", Gf), _p(sf["tile_start"]), kw.get("ws", _p(ws)), kw.get("cap_d", sf["cap_d"]), _p(sf["rec"]),
                       _p(sf["feats"]), kw.get("C", Cf), *P(out, oa, out, oa), _p(gr), _p(gf)]
    for match, kw in (("mode 1", dict(arr=st["arr"])), ("null pointer", dict(ws=None)), ("bad sizes", dict(C=0)), ("bad sizes", dict(cap_d=0)), ("bad sizes", dict(G=-2))):
        _refused("siu3r_raster_composite_feat_bwd", match, *fb(**kw), outs=[gf, gr])


def test_error_paths_of_the_viewer_helpers():
    G = 8
    q, s, g6 = _dev(torch.randn(G + 1, 4)), _dev(torch.rand(G, 3)), _dev(torch.randn(G, 6))
    gq, gs = _f((G, 4)), _f((G, 3))
    _refused("siu3r_quat_scale_to_cov6_bwd", "16-byte aligned", q.data_ptr() + 4, _p(s), _p(g6), _p(gq), _p(gs), G, outs=[gq, gs])
    _refused("siu3r_quat_scale_to_cov6_bwd", "null pointer", _p(q), None, _p(g6), _p(gq), _p(gs), G, outs=[gq, gs])
    _refused("siu3r_quat_scale_to_cov6_bwd", "null pointer", _p(q), _p(s), _p(g6), _p(gq), _p(gs), -1, outs=[gq, gs])
    m, cp, sh, g3 = _dev(torch.randn(G, 3)), _dev(torch.zeros(3)), _dev(torch.randn(G, 9, 3)), _dev(torch.randn(G, 3))
    gsh, gm, gc = _f((G, 9, 3)), _f((G, 3)), _f((3,))
    outs = [gsh, gm, gc]
    _refused("siu3r_sh_eval_bwd", "needs", _p(m), _p(cp), _p(sh), 9, 3, _p(g3), _p(gsh), _p(gm), _p(gc), G, outs=outs)
    _refused("siu3r_sh_eval_bwd", "needs", _p(m), _p(cp), _p(sh), 9, 5, _p(g3), _p(gsh), _p(gm), _p(gc), G, outs=outs)
    _refused("siu3r_sh_eval_bwd", "needs", _p(m), _p(cp), _p(sh), 9, -1, _p(g3), _p(gsh), _p(gm), _p(gc), G, outs=outs)
    _refused("siu3r_sh_eval_bwd", "null pointer", _p(m), None, _p(sh), 9, 2, _p(g3), _p(gsh), _p(gm), _p(gc), G, outs=outs)
    _refused("siu3r_sh_eval_bwd", "null pointer", _p(m), _p(cp), _p(sh), 9, 2, _p(g3), _p(gsh), _p(gm), None, G, outs=outs)
    _refused("siu3r_sh_eval_bwd", "null pointer", _p(m), _p(cp), None, 9, 2, _p(g3), _p(gsh), _p(gm), _p(gc), G, outs=outs)
