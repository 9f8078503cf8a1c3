"""The photometric and depth loss kernels (siu3r_amd/csrc/photo_loss.hip, depth_loss.hip) called directly through the C ABI on the crafted
cases of tests/dense_photo64.py and tests/dense_depth64.py and held, element by element, to their float64 references:
|got - ref| <= bound * S + extra with the bounds and scales derived in those files' headers (and proved on the CPU by
tests/test_photo_loss_ref.py and tests/test_depth_loss_ref.py: the closed forms against float64 autograd, a float32 emulation of the
kernels inside the bound, the kernels with one line wrong outside it, every case's branch population).  Every output lies inside a
sentinel-filled parent (_Guarded of tests/test_raster_stages_gpu.py): the guards stay intact, the slack of sliced layouts keeps the
sentinel bits, a null grad_pred is never touched, every `partials` entry is compared on its own, counts are exact, a term that is
switched off is NaN, exact zeros are exact zeros, and a second call gives the same bits.  Every SIU3R_CHECK line returns its error
before anything is written.

Where a line is run (case names as in PHOTO_CASES / DEPTH_CASES):

  photo_ssim_kernel<true>
    centre index clamped (yc, xc)         tile_edge_32x33, offset_1e4_right_tile (xc = W - 1); no_window_tile_42x75 (yc = H - 1)
    staging: off the image = the shift    every case (the halo of tile row / column 0; the right and lower edge of partial tiles)
    NLD loads, i >= NP * NP               every case (52 * 52 = 2704 = 10 * 256 + 144)
    j0 + r < NW, i < NW                   every case (NW = 42 = 6 * 7: the last segment is full; threads 252 .. 255 idle)
    valid: wy <= H - 11, wx <= W - 11     one_window_11x12 (one row of two windows), sliver_33x43 / one_column_43x74 (one owned column),
                                          no_window_tile_42x75 / third_tile_74x42 (a tile that owns none and only receives)
    i >= WLO && vcol >= WLO (ownership)   every case of two or more tiles: halo windows are evaluated and not summed
    spp_raw > 0                           pred_flat, flat_equal (clamped, exactly 0); flat_off_centre, flat_across_seam, outlier_centre
                                          (noise of either sign: the undecided allowance); target_flat (stt clamped alone)
    transposed blur, tile pixels y < H    every partial tile; the corner pixel one window reaches: one_window_11x12, flat_off_centre
    do_l1 / d > 0, d < 0, d == 0          lambda 0.2 and 1 - 2^-24 (one_column_43x74); lambda 1: no_window_tile_42x75, pred_flat,
                                          outlier_centre, offset_1e4*; d == 0: flat_equal
    strided store                         nhwc (sliver_33x43, grey_target, range_255), window (no_window_tile_42x75), nhwc_spare
                                          (third_tile_74x42); target strides 0: one_target_for_all_views, grey_target
  photo_ssim_kernel<false>                one_window_12x11_nograd (lambda 0.2), third_tile_75x32_nograd (window / nhwc_spare), ssim_only_nograd
                                          (do_l1 false: the L1 loop is skipped, the partial is 0)
  photo_l1_kernel                         l1_only (grad, nhwc, four tiles), l1_only_equal (exactly 0), l1_only_nograd_small (grad null, 5 x 7)
  photo_finalize_kernel
    i < n strided adds                    n = 1 (one_window_11x12), 12 (one_target_for_all_views: V C = 6), 300 (many_planes_300: n > 256, not a multiple of it)
    do_l1 / do_ssim, NaN outputs          lambda 0, 1 and between
  depth_l1_kernel<true / false>
    vec && i0 + 4 <= P / scalar tail      p1, p4, p5_views3, p1025_views3 (views 1, 2 off 16 bytes: scalar throughout), p2049_l1_inverse (tail of 1)
    ok[k]                                 the threshold rows (on, one ulp below, one ulp above) of O, D, T, Wt; nonfinite_l1; fill past the plane
    e > 0, e < 0, e == 0                  every case; equal_pixels, equal_pixels_inverse
    inverse                               p4, p1025_l1_inverse_nograd (no maps), p2049_l1_inverse, equal_pixels_inverse
  depth_moments_kernel                    p3_views3, p1023_views3 (inverse), p1024 (no maps), p2049_views3, nonfinite, views_*, small_loss
    min / max of a view                   views_constant (constant x, constant y), views_none_one (no pixel: +-inf; one pixel)
  depth_finalize_kernel
    i < bpv strided adds                  1 record, 2 (p1025), 3 (p2049), 257 (two_chunks_of_records: a second round of the loop)
    counted, s[0] >= 2                    views_none_one (0 and 1 valid pixels), views_constant; NaN per_view, denom = 1 of 3
    s[0] > 0 (l1 per_view)                views_none_one_l1 (a view of nothing: NaN; a view of one pixel), every other l1 case
    stats *= inv                          every pearson case of three counted views (p3_views3, p1023_views3, p2049_views3, nonfinite)
  depth_pearson_grad_kernel
    counted (c_y, c_x != 0)               views_none_one, views_constant: the maps of an uncounted view are exactly 0
    scalar path / tail                    p3_views3, p1023_views3, p2049_views3, nonfinite (7 x 37 = 259)
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dense_depth64 as DD
import dense_photo64 as DP
import dense_raster_bwd64 as B
from test_raster_bwd_stages_gpu import _call, _ok
from test_raster_stages_gpu import SENT, _Guarded

pytestmark = pytest.mark.gpu


def _g(shape, dtype=torch.float32):
    return _Guarded(shape, dtype)


def _close(got, ref, S, bound, name, extra=None, kernel=""):
    """assert_elems_close; a NaN of the reference (a term that is switched off) must meet a NaN.  With SIU3R_LOSS_PARITY_LOG=file one JSON
    line per comparison: the worst element as a fraction of its tolerance, the tolerance as a multiple of the scale (median and
    largest element) and, at the median, as a multiple of |ref|; tools/loss_parity.py groups the lines into profiles/loss_parity.json"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN where a number belongs, or the reverse"
    got, ref = np.where(nan, 0.0, got), np.where(nan, 0.0, ref)
    w = B.assert_elems_close(got, ref, S, bound, name=name, extra=extra)
    if os.environ.get("SIU3R_LOSS_PARITY_LOG"):
        med, mx = B.effective_bound(ref, S, bound, extra)
        rel = B.effective_bound(ref, np.abs(ref), 0.0, B.tolerance(ref, S, bound, extra))[0]  # the tolerance against |ref| itself
        with open(os.environ["SIU3R_LOSS_PARITY_LOG"], "a") as f:
            f.write(json.dumps({"case": name, "kernel": kernel, "worst_ratio_to_bound": w, "bound_over_S_median": med, "bound_over_S_max": mx,
                                "bound_over_ref_median": rel}) + "\n")
    return w


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


# ---- photometric loss ---------------------------------------------------------------------------------------------------------------------
def _call_photo(c):
    """one siu3r_photo_loss call on the case's layouts -> the guarded buffers and what the kernel saw"""
    from siu3r_amd import _lib

    V, Cn, H, W = c["V"], c["C"], c["H"], c["W"]
    play, tlay = c["play"], c["tlay"]
    pp, tp = torch.from_numpy(play["parent"]).cuda(), torch.from_numpy(tlay["parent"]).cuda()
    n = int(_lib.lib().siu3r_photo_loss_partials(V, Cn, H, W))
    assert n == V * Cn * -(-H // 32) * -(-W // 32)
    b = dict(partials=_g((n, 2)), out=_g((3,)), grad=_g((play["parent"].size,)) if c["grad"] else None, pp=pp, tp=tp)
    ps, ts = (C.c_int64 * 4)(*play["strides"]), (C.c_int64 * 4)(*tlay["strides"])
    gp = b["grad"].t.data_ptr() + 4 * play["offset"] if c["grad"] else None
    _ok("siu3r_photo_loss", pp.data_ptr() + 4 * play["offset"], tp.data_ptr() + 4 * tlay["offset"], V, Cn, H, W, ps, ts, c["lam"], c["dr"], gp,
        b["partials"].t.data_ptr(), b["out"].t.data_ptr())
    return b


def _photo_outputs(c, b):
    got = dict(out=b["out"].t.cpu().numpy(), partials=b["partials"].t.cpu().numpy(), grad=None)
    if c["grad"]:
        got["grad"] = DP.logical(c["play"], b["grad"].t.cpu().numpy())
    return got


def _photo_kernel(c, what):
    if what == "out":
        return "photo_finalize_kernel"
    return "photo_l1_kernel" if c["lam"] == 0.0 else f"photo_ssim_kernel<{'true' if c['grad'] else 'false'}>"


@pytest.mark.parametrize("name", list(DP.PHOTO_CASES))
def test_photo_loss(name):
    c, ref = DP.photo_case(name), DP.photo_ref(name)
    b = _call_photo(c)
    for k in ("partials", "out", "grad"):
        assert b[k] is None or b[k].guards_intact(), f"{k}: written outside the buffer"
    # the inputs are read only, slack included
    assert torch.equal(_bits(b["pp"]), _bits(torch.from_numpy(c["play"]["parent"]))) and torch.equal(_bits(b["tp"]), _bits(torch.from_numpy(c["tlay"]["parent"])))
    if c["grad"]:  # pred's exact layout: every element the four strides do not address keeps the sentinel
        own = torch.from_numpy(DP.owned_mask(c["play"]))
        whole = b["grad"].t.cpu()
        assert bool((whole[~own] == SENT).all()), "grad_pred: a store into the slack of the layout"
        assert not bool((whole[own] == SENT).any()), "grad_pred: a pixel was not written"
    got = _photo_outputs(c, b)
    do_l1, do_ssim = c["lam"] != 1.0, c["lam"] != 0.0
    assert np.isnan(got["out"][1]) == (not do_l1) and np.isnan(got["out"][2]) == (not do_ssim)
    DP.photo_compare(got, ref, lambda g, r, S, bound, what, extra: _close(g, r, S, bound, f"photo/{name}/{what}", extra, _photo_kernel(c, what)))
    if not do_l1:
        assert not got["partials"][:, 0].any()
    if not do_ssim:
        assert not got["partials"][:, 1].any()
    if c["grad"] and not do_ssim:
        assert not got["grad"][c["P"] == c["T"]].any(), "pred == target: the L1 subgradient is exactly 0"
    # a second call gives the same bits
    b2 = _call_photo(c)
    for k in ("partials", "out", "grad"):
        assert b[k] is None or torch.equal(_bits(b[k].whole), _bits(b2[k].whole)), f"{k}: two calls differ"


# (error text, keyword overrides) for siu3r_photo_loss; null=x passes a null pointer for x
PHOTO_ERRORS = [("null pointer", dict(null="pred")), ("null pointer", dict(null="target")), ("null pointer", dict(null="partials")), ("null pointer", dict(null="out")),
                ("null pointer", dict(null="ps")), ("null pointer", dict(null="ts")), ("empty input", dict(V=0)), ("empty input", dict(C=0)),
                ("empty input", dict(H=0)), ("empty input", dict(W=-3)), ("outside [0, 1]", dict(lam=-0.125)), ("outside [0, 1]", dict(lam=1.5)),
                ("outside [0, 1]", dict(lam=float("nan"))), ("data_range", dict(dr=0.0)), ("data_range", dict(dr=-1.0)), ("data_range", dict(dr=float("nan"))),
                ("SSIM needs", dict(H=10)), ("SSIM needs", dict(W=10, lam=1.0)), ("exceed one launch", dict(V=32768, C=32768, H=1, W=1, lam=0.0)),
                ("negative strides", dict(ps=(16 * 16, 16 * 16, -16, 1))), ("negative strides", dict(ts=(16 * 16, 16 * 16, 16, -1)))]


@pytest.mark.parametrize("text,kw", PHOTO_ERRORS, ids=[f"{i}_{t.split()[0]}" for i, (t, _) in enumerate(PHOTO_ERRORS)])
def test_photo_loss_argument_errors_write_nothing(text, kw):
    from siu3r_amd import _lib

    a = dict(V=1, C=1, H=16, W=16, lam=0.2, dr=1.0, ps=(256, 256, 16, 1), ts=(256, 256, 16, 1), null=None)
    a.update(kw)
    img = torch.rand(16 * 16).cuda()
    bufs = dict(grad=_g((256,)), partials=_g((8, 2)), out=_g((3,)))
    ptr = dict(pred=img.data_ptr(), target=img.data_ptr(), partials=bufs["partials"].t.data_ptr(), out=bufs["out"].t.data_ptr(),
               ps=(C.c_int64 * 4)(*a["ps"]), ts=(C.c_int64 * 4)(*a["ts"]))
    if a["null"]:
        ptr[a["null"]] = None
    rc = _call("siu3r_photo_loss", ptr["pred"], ptr["target"], a["V"], a["C"], a["H"], a["W"], ptr["ps"], ptr["ts"], a["lam"], a["dr"], bufs["grad"].t.data_ptr(),
               ptr["partials"], ptr["out"])
    assert rc == 1 and text in _lib.lib().siu3r_last_error().decode()
    assert all(b.untouched() for b in bufs.values()), "an argument error wrote an output"


def test_photo_loss_accepts_small_images_without_ssim():
    """H, W below the window are an error only where SIU3R computes SSIM; the partials count of bad shapes is 0"""
    from siu3r_amd import _lib

    l = _lib.lib()
    assert l.siu3r_photo_loss_partials(0, 1, 16, 16) == 0 and l.siu3r_photo_loss_partials(1, 1, -1, 16) == 0 and l.siu3r_photo_loss_partials(2, 3, 33, 64) == 24
    c = DP.photo_case("l1_only_nograd_small")
    assert c["H"] < 11 and c["W"] < 11 and c["lam"] == 0.0
    b = _call_photo(c)
    assert abs(float(b["out"].t[0]) - DP.photo_ref("l1_only_nograd_small")["out"][0]) < 1e-6


def test_front_end_stride_zero_rule(monkeypatch):
    """losses.py: an expanded TARGET reaches the kernel as stored (view stride 0), an expanded differentiated PRED is made dense; both
    give the reference's gradient"""
    from siu3r_amd import losses

    seen, real = [], losses._launch
    monkeypatch.setattr(losses, "_launch", lambda p4, t4, *a: (seen.append((tuple(p4.stride()), tuple(t4.stride()))), real(p4, t4, *a))[1])
    name = "one_target_for_all_views"
    c, ref = DP.photo_case(name), DP.photo_ref(name)
    V, Cn, H, W = c["V"], c["C"], c["H"], c["W"]
    pred = torch.from_numpy(c["P"]).cuda().requires_grad_(True)
    t1 = torch.from_numpy(c["T"][:1]).cuda()
    loss = losses.photometric_loss(pred, t1.expand(V, -1, -1, -1), c["lam"], c["dr"])
    loss.backward()
    assert seen[-1] == ((Cn * H * W, H * W, W, 1), (0, H * W, W, 1)), seen[-1]
    _close(pred.grad.cpu().numpy(), ref["grad"], ref["S_grad"], DP.PHOTO_BOUND, f"photo/front_end_target_expanded/grad", ref["extra_grad"], "photo_ssim_kernel<true>")
    _close([float(loss.detach())], ref["out"][:1], ref["S_out"][:1], DP.PHOTO_BOUND, "photo/front_end_target_expanded/out", None, "photo_finalize_kernel")
    name = "one_pred_for_all_views"
    c, ref = DP.photo_case(name), DP.photo_ref(name)
    p1 = torch.from_numpy(c["P"][:1]).cuda().requires_grad_(True)
    pe = p1.expand(c["V"], -1, -1, -1)
    assert pe.stride(0) == 0
    losses.photometric_loss(pe, torch.from_numpy(c["T"]).cuda(), c["lam"], c["dr"]).backward()
    assert seen[-1][0] == (Cn * H * W, H * W, W, 1), "an expanded pred that receives a gradient must reach the kernel dense"
    # autograd adds the V views' gradients in float32: V more roundings on the sum of magnitudes
    want, S = ref["grad"].sum(0, keepdims=True), ref["S_grad"].sum(0, keepdims=True) + c["V"] * np.abs(ref["grad"]).sum(0, keepdims=True) / 2
    _close(p1.grad.cpu().numpy(), want, S, DP.PHOTO_BOUND, "photo/front_end_pred_expanded/grad", ref["extra_grad"].sum(0, keepdims=True), "photo_ssim_kernel<true>")


# ---- depth loss -----------------------------------------------------------------------------------------------------------------------------
def _in(a):
    """an input inside a guarded parent: the views' bases are 16-byte aligned exactly where v * H * W is a multiple of 4"""
    if a is None:
        return None
    g = _g(a.shape)
    g.t.copy_(torch.from_numpy(a))
    assert g.t.data_ptr() % 16 == 0
    return g


def _call_depth(c):
    from siu3r_amd import _lib

    V, H, W = c["V"], c["H"], c["W"]
    nbytes = int(_lib.lib().siu3r_depth_loss_ws(V, H, W))
    assert nbytes == (V * -(-H * W // 1024) * 11 + V * 4) * 8
    b = dict(D=_in(c["D"]), O=_in(c["O"]), T=_in(c["T"]), Wt=_in(c["Wt"]), ws=_g((nbytes // 8,), torch.float64), out=_g((4,)), per_view=_g((V,)),
             valid=_g((V,), torch.int32), g_depth=_g((V, H, W)) if c["grad"] else None, g_opacity=_g((V, H, W)) if c["grad"] else None)
    p = lambda k: None if b[k] is None else b[k].t.data_ptr()
    _ok("siu3r_depth_loss", p("D"), p("O"), p("T"), p("Wt"), V, H, W, {"l1": 0, "pearson": 1}[c["mode"]], {"depth": 0, "inverse": 1}[c["space"]], DD.MIN_OPACITY,
        p("g_depth"), p("g_opacity"), p("ws"), p("out"), p("per_view"), p("valid"))
    return b


def _depth_kernel(c, what):
    if what in ("g_depth", "g_opacity"):
        return "depth_pearson_grad_kernel" if c["mode"] == "pearson" else "depth_l1_kernel"
    return "depth_finalize_kernel" + (" (depth_moments_kernel)" if c["mode"] == "pearson" else " (depth_l1_kernel)")


@pytest.mark.parametrize("name", list(DD.DEPTH_CASES))
def test_depth_loss(name):
    c, ref = DD.depth_case(name), DD.depth_ref(name)
    b = _call_depth(c)
    for k, g in b.items():
        assert g is None or g.guards_intact(), f"{k}: written outside the buffer"
    for k in ("D", "O", "T", "Wt"):  # inputs are read only
        assert b[k] is None or torch.equal(_bits(b[k].t), _bits(torch.from_numpy(c[k])))
    assert b["valid"].t.cpu().tolist() == ref["valid"].tolist(), "the counts of valid pixels are exact"
    out = b["out"].t.cpu().numpy()
    assert out[3] == 0.0 and out[1] == np.float32(ref["out"][1]) and (c["mode"] == "l1" or out[2] == 1.0)
    outs = dict(out=out, per_view=b["per_view"].t.cpu().numpy())
    if c["grad"]:
        outs.update(g_depth=b["g_depth"].t.cpu().numpy(), g_opacity=b["g_opacity"].t.cpu().numpy())
    for k, got in outs.items():
        r = ref[k]
        extra = ref["tol_" + k] - DD.DEPTH_BOUND * np.abs(np.nan_to_num(r))
        _close(got, r, np.abs(np.nan_to_num(r)), DD.DEPTH_BOUND, f"depth/{name}/{k}", extra, _depth_kernel(c, k))
    if c["grad"]:
        for k in ("g_depth", "g_opacity"):
            assert not outs[k].view(np.int32)[~ref["ok"]].any(), f"{k}: an invalid pixel gets +0"
            # the exact zeros of the contract: l1, x == y bit for bit; pearson, every pixel of a view that is not counted
            zero = (ref[k] == 0) if c["mode"] == "l1" else np.broadcast_to(np.isnan(ref["per_view"])[:, None, None], ref[k].shape)
            assert not outs[k][zero].any(), f"{k}: an exact zero of the contract (x == y, an uncounted view) is not exact"
    b2 = _call_depth(c)
    for k in ("out", "per_view", "valid", "g_depth", "g_opacity"):
        assert b[k] is None or torch.equal(_bits(b[k].whole), _bits(b2[k].whole)), f"{k}: two calls differ"


DEPTH_ERRORS = [("null pointer", dict(null="D")), ("null pointer", dict(null="O")), ("null pointer", dict(null="T")), ("null pointer", dict(null="ws")),
                ("null pointer", dict(null="out")), ("null pointer", dict(null="per_view")), ("null pointer", dict(null="valid")), ("empty input", dict(V=0)),
                ("empty input", dict(H=0)), ("empty input", dict(W=-1)), ("32-bit indexing", dict(H=65536, W=32768)), ("exceed one launch", dict(V=65536)),
                ("mode", dict(mode=2)), ("mode", dict(mode=-1)), ("space", dict(space=2)), ("space", dict(space=-1)), ("min_opacity", dict(mo=-0.5)),
                ("min_opacity", dict(mo=float("inf"))), ("min_opacity", dict(mo=float("nan"))), ("come together", dict(null="g_depth")),
                ("come together", dict(null="g_opacity")), ("8-byte aligned", dict(ws_off=4))]


@pytest.mark.parametrize("text,kw", DEPTH_ERRORS, ids=[f"{i}_{t.split()[0]}" for i, (t, _) in enumerate(DEPTH_ERRORS)])
def test_depth_loss_argument_errors_write_nothing(text, kw):
    from siu3r_amd import _lib

    a = dict(V=2, H=4, W=8, mode=1, space=0, mo=0.5, null=None, ws_off=0)
    a.update(kw)
    x = (1.0 + torch.rand(2, 4, 8)).cuda()
    bufs = dict(ws=_g((64,), torch.float64), out=_g((4,)), per_view=_g((2,)), valid=_g((2,), torch.int32), g_depth=_g((2, 4, 8)), g_opacity=_g((2, 4, 8)))
    ptr = dict(D=x.data_ptr(), O=x.data_ptr(), T=x.data_ptr(), **{k: g.t.data_ptr() for k, g in bufs.items()})
    ptr["ws"] += a["ws_off"]
    if a["null"]:
        ptr[a["null"]] = None
    rc = _call("siu3r_depth_loss", ptr["D"], ptr["O"], ptr["T"], None, a["V"], a["H"], a["W"], a["mode"], a["space"], a["mo"], ptr["g_depth"], ptr["g_opacity"],
               ptr["ws"], ptr["out"], ptr["per_view"], ptr["valid"])
    assert rc == 1 and text in _lib.lib().siu3r_last_error().decode()
    assert all(b.untouched() for b in bufs.values()), "an argument error wrote an output"
    l = _lib.lib()
    assert l.siu3r_depth_loss_ws(1, 65536, 32768) == 0 and l.siu3r_depth_loss_ws(0, 4, 4) == 0
