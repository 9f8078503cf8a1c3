"""Every forward stage of the rasterizer that produces floating-point numbers (siu3r_amd/csrc/raster.hip: project_kernel with
cam_pose_kernel / cam_pose_c2w_kernel, composite_rgb_kernel, composite_feat_kernel, composite_feat5_kernel) called directly through the
C ABI on crafted cases and held, element by element, to its float64 reference with the bounds derived in the header of
tests/dense_raster_fwd64.py (and proved on the CPU by tests/test_raster_fwd_stages_ref.py: a float32 emulation of every stage within
the bound, one wrong answer per branch outside it, every case's branch population).  Integer outputs are exact on decided rows and
self-consistent on the others; every output lies inside a sentinel-filled parent (_Guarded) whose guards stay intact.

Where a line is run (projection cases: PROJ_CASES of dense_raster_bwd64 + PROJ_FWD_NEW; composite cases: COMP_CASES + FWD_COMP_CASES):

  project_kernel
    opacity_aware_extent                  k3_oae: opacities below, at and above alpha_min, the logarithmic extent smaller and larger than
                                          extent_sigma (2.0 there: at 3.33 it is the smaller one for every opacity <= 1)
    radius_clip                           k3_clip: radius_clip 2.0, radii 1 / 2 / 3 px in x and y separately (eps2d 0.01)
    PV = 16 view chunks, per-view stats   k2_v16, k2_v17, k2_v33 (G = 257): a block of Gaussians culled in every view of the even chunks, the
                                          rest in every view of the odd ones
    views of different sh_degree          k2_mixed, k2_mixed_planar: degrees 0, 3, 1, 4 + band 4 over 25 coefficients; a block culled in the
                                          degree-0 view, a block visible from the degree-4 view only
    scalar tail of the 16-byte SH loads   k2_deg0 (1 coefficient), k2_ch4, k2_ch9 (k2_one), k2_deg3 (16), k2_deg4_band4 (25)
    sh_planar against interleaved         k2_mixed_planar against k2_mixed (the same values: the same records bit for bit), k2_deg1_planar
    cov_stride 9, poisoned triangle       every stride-9 case (NaN in the entries the kernel must not read)
    tz <= k2_znear_cull, < near, > far    k2_depth, k3_depth: identity pose, rows on the threshold and one and two fp32 ulps either side
    K2 truncating / K3 floor-ceil rect    every case (decided rows exact); k2_edges, k3_edges: means off all four frame edges
    key clamp below 0xffffffff            cannot be reached by a valid row (dense_raster_fwd64, header); keys are culled exactly on empty rects
    NaN mean, Inf covariance              k2_nonfinite, k3_nonfinite: culled, key 0xffffffff, not counted
    K3 colours NULL / 3 / 5 channels      k3_nocolor, k3_rgb, k3_c5: rp[2] written, or left at the fill
  cam_pose_kernel / cam_pose_c2w_kernel   test_pose_dp, test_pose_c2w: V = 1, 3, 65 (two workgroups of 64 threads), off-centre non-square K, t_scale 10,
                                          one singular c2w among good ones; fields the kernels do not own keep the host's bytes
  composite_rgb_kernel
    refill slice that does not fit        k2_stage tile (0, 0): 250 + 250 + 100 coverers in the first three slices: slice 2 is read again
    STG_PULL                              k2_stage tile (1, 0): 188 staged after a full round (refill again), tile (2, 0): 196 (walk first)
    nq % 4 = 1, 2, 3, 0                   k2_pairs: quadrant lists of 0 .. 7 entries over two tiles, one empty quadrant between listed ones
    saturation on a pair's first entry    k2_satpair, k3_satpair: bands of pixels saturating on even and on odd list positions, entries behind
    n_touched, both nt_post_blend         every k2 case (post-blend); k2_nt_pre (pre-blend); NT = false once (k2_full, bit-identical maps)
    background where nothing blends       k2_pairs, k2_stage (most of the frame), the empty last tile of the full scenes
  composite_feat_kernel
    batches of 128                        feat_batch: tile lists of 127, 128, 129, 257 entries
    channel tails                         feat_batch at C = 1, 31, 32, 33; feat_c1 .. feat_c168
  composite_feat5_kernel
    1 - 4 chunks, ring wrap, prologue     feat_ring: quadrant lists of 0, 1, 7, 8, 9, 16, 17, 24, 25, 70 entries
    NP = 1 .. 6, shifted last window      feat_ring at C = 32, 33, 64, 65, 96, 97, 160, 161, 192, 193
    shifted-back second chunk, 3 chunks   feat_ring at C = 193 and 385; C = 193 with siu3r_raster_tune(1, n), n = 1 .. 5
    early exit with DMAs in flight        feat_sat_early: quadrant 0 saturates in its first chunk, 40 entries behind; quadrant 1 walks all
    ragged frame, two views               feat_ring_ragged (90 x 62, V = 2, C = 65)
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dense_raster_bwd64 as B
import dense_raster_fwd64 as F
from test_raster_bwd_stages_gpu import _cam_blocks, _composite_state, _dev, _f, _ok, _p, _refused
from test_raster_stages_gpu import SENT, _Guarded

pytestmark = pytest.mark.gpu
FILL = np.float32(SENT)


def _log(**kw):
    if os.environ.get("SIU3R_RASTER_FWD_PARITY_LOG"):
        with open(os.environ["SIU3R_RASTER_FWD_PARITY_LOG"], "a") as f:
            f.write(json.dumps(kw) + "\n")


def _log_maps(case, worst, med, mx, share):
    print(f"[fwd parity] {case}: worst element {worst:.3f} of its bound")
    _log(case=case, worst_ratio_to_bound=worst, bound_over_S_median=med, bound_over_S_max=mx, undecided_share=share)


def _log_proj(case, worst, share):
    print(f"[fwd parity] {case}: worst ratio per slot {worst}, undecided rows {share:.4f}")
    _log(case="proj " + case, worst_ratio_to_bound=max(worst.values()) if worst else 0.0, bound_over_S_median=F.PROJ_MEAN_BOUND, bound_over_S_max=F.SH_FWD_BOUND,
         undecided_share=share)


# ---- projection ---------------------------------------------------------------------------------------------------------------------------
def _project(c, cams=None, entry="siu3r_raster_project", pose=()):
    """runs the projection entry point on a case of dense_raster_fwd64 -> got (numpy, as check_projection takes it), the read-back blocks"""
    from siu3r_amd import _lib, raster

    cams = cams or c["cams"]
    mode, V, G = c["mode"], len(cams), c["G"]
    arr = raster._cam_array(cams)
    sz = C.sizeof(cams[0])
    cams_dev = _Guarded((V * sz // 4,))
    means, opac = _dev(c["means"]), _dev(c["opac"])
    if c["stride"] == 6:
        cov = _dev(c["cov6"])
    else:  # [G,3,3]: the entries the kernel must not read are NaN
        cov = torch.full((G, 9), float("nan"))
        cov[:, [0, 1, 2, 4, 5, 8]] = c["cov6"]
        cov = cov.cuda()
    col, channels = c["colors"], c["channels"]
    if col is not None and mode == 0 and c["planar"]:
        full = torch.zeros((G, 25, 3))
        full[:, :col.shape[1]] = col
        col = full.permute(0, 2, 1).contiguous()
    colors = None if col is None else col.contiguous().cuda()
    o = dict(rec=_f((V, G, 12)), radii=_Guarded((V, G, 2)), rect=_Guarded((V, G, 4)), tiles=_Guarded((V, G)), keys=_Guarded((V, G)), stats=_Guarded((V, 4), torch.int64))
    args = [arr, V, _p(cams_dev), *pose, G, _p(means), _p(cov), c["stride"], _p(opac), _p(colors), channels, int(bool(c["planar"]) and mode == 0),
            *[_p(o[k]) for k in ("rec", "radii", "rect", "tiles", "keys", "stats")]]
    _ok(entry, *args)
    for k, b in o.items():
        assert b.guards_intact(), f"{k}: written outside the buffer"
    assert cams_dev.guards_intact()
    got = {k: o[k].t.cpu().numpy() for k in ("rec", "radii", "rect", "tiles", "stats")}
    got["keys"] = o["keys"].t.cpu().numpy().view(np.uint32)
    got["fill"] = FILL
    blocks = (type(cams[0]) * V).from_buffer_copy(cams_dev.t.cpu().numpy().tobytes())
    return got, blocks, args, o


@pytest.mark.parametrize("name", F.PROJ_FWD_CASES)
def test_projection(name):
    c = F.proj_fwd_case(name)
    got, blocks, args, o = _project(c)
    assert bytes(blocks) == bytes(_cam_blocks(c["cams"])[0]), "siu3r_raster_project uploads the host blocks as they are"
    F.check_projection(c, F.proj_fwd_ref(name), got, log=_log_proj)
    if name == "k2_mixed_planar":  # the same values in the planar layout: the same records, bit for bit
        other, _, _, _ = _project(F.proj_fwd_case("k2_mixed"))
        for k in ("rec", "radii", "rect", "tiles", "keys"):
            assert np.array_equal(got[k].view(np.int32), other[k].view(np.int32)), f"planar and interleaved SH differ in {k}"
    if name == "k2_v33":  # one repeat launch: the outputs are deterministic
        again, _, _, _ = _project(c)
        for k in ("rec", "radii", "rect", "tiles", "keys", "stats"):
            assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k


def test_nonfinite_rows_are_culled():
    for name in ("k2_nonfinite", "k3_nonfinite"):
        c = F.proj_fwd_case(name)
        got, _, _, _ = _project(c)
        for g in (64, 65):  # the NaN mean, the Inf covariance
            assert got["keys"][0, g] == 0xFFFFFFFF and got["tiles"][0, g] == 0 and not got["rect"][0, g].any() and not got["radii"][0, g].any(), (name, g)
        assert int(got["stats"][0, 0]) == int((got["keys"][0] != 0xFFFFFFFF).sum()) <= 64


def _pose_case(mode, V):
    rng = np.random.default_rng(100 * mode + V)
    W, H, G = 96, 64, 64
    from siu3r_amd import raster

    c2w = torch.stack([B._c2w(rng) for _ in range(V)])
    c2w[:, :3, 3] *= 0.1  # (scaled by t_scale = 10 on the device)
    if V > 1:
        c2w[1, :3, :3] = 0.0  # a singular pose among good ones (its determinant is exactly 0)
    Kn = torch.tensor([[0.9, 0.0, 0.45], [0.0, 1.3, 0.55], [0.0, 0.0, 1.0]]).repeat(V, 1, 1)
    if mode == 0:
        cams = [raster.make_cam_k2(None, None, None, None, None, [0.1, 0.2, 0.3], W, H, sh_degree=1, near=0.2, far=1000.0) for _ in range(V)]
    else:
        cams = [raster.make_cam_k3(torch.eye(4), 1.0, 1.0, 0.0, 0.0, W, H) for _ in range(V)]
    good = c2w[0].double().clone()
    good[:3, 3] *= 10.0
    tz = rng.uniform(1.5, 4.0, G)
    pc = torch.from_numpy(np.stack([rng.uniform(-0.4, 0.4, G) * tz, rng.uniform(-0.3, 0.3, G) * tz, tz, np.ones(G)], -1))
    means = (pc @ good.T)[:, :3].float()
    colors = torch.from_numpy(rng.normal(size=(G, 4, 3)) * 0.2).float() if mode == 0 else torch.from_numpy(rng.uniform(0, 1, (G, 3))).float()
    c = dict(name=f"pose mode {mode} V {V}", mode=mode, V=V, G=G, cams=cams, means=means, cov6=F._covs(rng, G), opac=torch.from_numpy(rng.uniform(0.1, 0.9, G)).float(),
             colors=colors, channels=4 if mode == 0 else 3, planar=False, stride=6, exact_depth=False)
    return c, c2w.float(), Kn


OWNED_C2W = {0: ("w2c", "campos", "tanfovx", "tanfovy", "proj"), 1: ("w2c", "campos", "fx", "fy", "cx", "cy")}


def _same_but(blocks, cams, owned):
    """the fields the pose kernels do not own keep the host's bytes"""
    for b, h in zip(blocks, cams):
        for name, _ in type(h)._fields_:
            if name not in owned:
                x, y = getattr(b, name), getattr(h, name)
                assert (bytes(x) == bytes(y)) if hasattr(x, "_length_") else (x == y or (x != x and y != y)), name


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V", [1, 3, 65])
def test_pose_c2w(mode, V):
    c, c2w, Kn = _pose_case(mode, V)
    dc, dk = _dev(c2w), _dev(Kn)
    got, blocks, _, _ = _project(c, entry="siu3r_raster_project_c2w", pose=(_p(dc), _p(dk), 10.0))
    _same_but(blocks, c["cams"], OWNED_C2W[mode])
    cams = [blocks[v] for v in range(V)]
    for v in range(V):
        ref = F.pose_c2w64(c["cams"][v], c2w[v].numpy(), Kn[v].numpy(), 10.0)
        for k, (val, err) in ref.items():
            g = np.array(list(getattr(cams[v], k))) if hasattr(getattr(cams[v], k), "_length_") else np.array([getattr(cams[v], k)])
            if val is None:
                assert V > 1 and v == 1 and np.isnan(g).all(), "a singular pose poisons the view"
                continue
            assert float(np.max(err, initial=0.0)) < 1e-9, "the float64 evaluation error is orders below an fp32 ulp"
            assert F.pose_close(g, val, err), (c["name"], v, k, g, val)
    refs = F.proj_refs_for(dict(c, cams=cams))
    F.check_projection(dict(c, cams=cams), refs, got, log=_log_proj)
    if V > 1:
        assert int(got["stats"][1, 0]) == 0 and int(got["stats"][1, 1]) == 0 and (got["keys"][1] == 0xFFFFFFFF).all(), "the singular view projects nothing"
        assert int(got["stats"][0, 0]) > 32, "its neighbours are unaffected (check_projection holds each of them to its own reference)"


@pytest.mark.parametrize("V", [1, 3, 65])
def test_pose_dp(V):
    c, c2w, _ = _pose_case(1, V)
    c2w = c2w.double().clone()
    c2w[:, :3, 3] *= 10.0
    if V > 1:
        c2w[1] = c2w[0]
    vm = torch.linalg.inv(c2w).float()
    Ks = torch.tensor([[70.0, 0.0, 33.6], [0.0, 55.0, 38.4], [0.0, 0.0, 1.0]]).repeat(V, 1, 1)
    dv, dk = _dev(vm), _dev(Ks)
    got, blocks, _, _ = _project(c, entry="siu3r_raster_project_dp", pose=(_p(dv), _p(dk)))
    _same_but(blocks, c["cams"], ("w2c", "fx", "fy", "cx", "cy"))
    for v in range(V):  # plain copies: bit-equal
        assert np.array_equal(np.array(list(blocks[v].w2c), np.float32), vm[v].reshape(-1).numpy())
        assert (blocks[v].fx, blocks[v].fy, blocks[v].cx, blocks[v].cy) == (70.0, 55.0, float(np.float32(33.6)), float(np.float32(38.4)))
    cams = [blocks[v] for v in range(V)]
    F.check_projection(dict(c, cams=cams), F.proj_refs_for(dict(c, cams=cams)), got, log=_log_proj)


def test_pose_refusals():
    c, c2w, Kn = _pose_case(0, 1)
    c3, c2w3, Kn3 = _pose_case(1, 1)
    dc, dk = _dev(c2w), _dev(Kn)
    got, _, args, o = _project(c, entry="siu3r_raster_project_c2w", pose=(_p(dc), _p(dk), 1.0))
    outs = [_f((1, c["G"], 12))]

    def with_pose(a, pose, rec):
        a = list(a)
        a[3:6] = pose
        a[-6] = _p(rec)
        return a

    _refused("siu3r_raster_project_c2w", "null pose", *with_pose(args, (None, _p(dk), 1.0), outs[0]), outs=outs)
    _refused("siu3r_raster_project_c2w", "null pose", *with_pose(args, (_p(dc), None, 1.0), outs[0]), outs=outs)
    bad = [type(c["cams"][0]).from_buffer_copy(bytes(c["cams"][0]))]
    bad[0].k2_near = bad[0].k2_far
    from siu3r_amd import raster

    a = with_pose(args, (_p(dc), _p(dk), 1.0), outs[0])
    a[0] = raster._cam_array(bad)
    _refused("siu3r_raster_project_c2w", "k2_near < k2_far", *a, outs=outs)
    a = with_pose(args, (_p(dc), _p(dk), 1.0), outs[0])
    a = a[:5] + a[6:]  # the _dp signature: no t_scale
    _refused("siu3r_raster_project_dp", "mode 1", *a, outs=outs)
    a[3] = None
    _refused("siu3r_raster_project_dp", "null pose", *a, outs=outs)


# ---- composites -----------------------------------------------------------------------------------------------------------------------------
def _rgb(c, st, nt=True):
    V, G, H, W = c["V"], c["G"], c["H"], c["W"]
    k3 = c["kind"] == "k3"
    image = _f((V, H, W, 3) if k3 else (V, 3, H, W))
    depth, alpha = (None if k3 else _f((V, H, W))), _f((V, H, W))
    n_touched = _Guarded((V, G)) if (nt and not k3) else None
    _ok("siu3r_raster_composite_rgb", st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(image), _p(depth),
        _p(alpha), _p(n_touched))
    for b in (image, depth, alpha, n_touched):
        assert b is None or b.guards_intact(), "a composite wrote outside its map (pixels off a ragged frame lie in the guard bands)"
    return image, depth, alpha, n_touched


def _feat(c, st, feats, Cc, ws_form):
    """composite_feat, or composite_feat_ws with a workspace -> out, alpha (guarded)"""
    from siu3r_amd import _lib

    V, G, H, W = c["V"], c["G"], c["H"], c["W"]
    out, alpha = _f((V, H, W, Cc)), _f((V, H, W))
    base = [st["arr"], V, _p(st["cams_dev"]), G, _p(st["tile_start"]), _p(st["ids"]), st["cap_d"], _p(st["rec"]), _p(feats), Cc, _p(out), _p(alpha)]
    if not ws_form:
        _ok("siu3r_raster_composite_feat", *base)
    else:
        nbytes = int(_lib.lib().siu3r_raster_composite_feat_ws_bytes(W, H, V, st["cap_d"]))
        ws = _Guarded((nbytes // 4,))
        takes = int(_lib.lib().siu3r_raster_composite_feat_ws_lists(W, H, V, G, _p(feats), Cc, _p(ws), nbytes, st["cap_d"]))
        assert takes == (1 if Cc >= 32 else 0), "the matrix-core form serves 32 channels and more"
        _ok("siu3r_raster_composite_feat_ws", *base, _p(ws), nbytes)
        assert ws.guards_intact()
    assert out.guards_intact() and alpha.guards_intact()
    return out, alpha


def _np(t):
    return t.t.cpu().numpy() if isinstance(t, _Guarded) else t.cpu().numpy()


def _check_feat(name, c, st, Cc):
    feats = _dev(F.case_feats(c, Cc))
    refs = F.comp_fwd_ref(c, Cc)
    out, alpha = _feat(c, st, feats, Cc, False)
    F.check_maps(f"{name} C={Cc} feat", "feat", refs, _np(out), _np(alpha), log=_log_maps)
    out_ws, alpha_ws = _feat(c, st, feats, Cc, True)
    F.check_maps(f"{name} C={Cc} feat_ws", "feat", refs, _np(out_ws), _np(alpha_ws), log=_log_maps)
    assert torch.equal(out.t, out_ws.t) and torch.equal(alpha.t, alpha_ws.t), f"{name} C={Cc}: composite_feat_ws must equal composite_feat bit for bit"


FEAT_RUNS = [(n, B.COMP_CASES[n][5]) for n in B.COMP_CASES if B.COMP_CASES[n][0] == "feat"] + [("feat_ring", Cc) for Cc in F.RING_CHANNELS] + \
    [("feat_batch", Cc) for Cc in F.BATCH_CHANNELS] + [("feat_ring_ragged", 65), ("feat_sat_early", 65), ("feat_sat_early", 33)]
RGB_RUNS = [n for n in list(B.COMP_CASES) + list(F.FWD_COMP_CASES) if (B.COMP_CASES.get(n) or F.FWD_COMP_CASES[n])[0] != "feat"]


@pytest.mark.parametrize("name", RGB_RUNS)
def test_composite_rgb(name):
    c = F.fwd_comp_case(name)
    st = _composite_state(c)
    refs = F.comp_fwd_ref(c)
    k2 = c["kind"] == "k2"
    image, depth, alpha, nt = _rgb(c, st)
    out = _np(image).transpose(0, 2, 3, 1) if k2 else _np(image)
    F.check_maps(name, c["kind"], refs, out, _np(alpha), _np(depth) if k2 else None, _np(nt) if k2 else None, log=_log_maps)
    if name in ("k2_full", "k2_stage"):  # the NT = false instantiation (and with it one repeat launch): bit-identical maps
        image2, depth2, alpha2, _ = _rgb(c, st, nt=False)
        assert torch.equal(image.t, image2.t) and torch.equal(depth.t, depth2.t) and torch.equal(alpha.t, alpha2.t)
    if name == "k3_satpair":
        image2, _, alpha2, _ = _rgb(c, st)
        assert torch.equal(image.t, image2.t) and torch.equal(alpha.t, alpha2.t)


@pytest.mark.parametrize("name,Cc", FEAT_RUNS)
def test_composite_feat(name, Cc):
    c = F.fwd_comp_case(name)
    _check_feat(name, c, _composite_state(dict(c, feats=F.case_feats(c, Cc))), Cc)


@pytest.fixture
def feat_np():
    from siu3r_amd import _lib

    yield lambda n: _lib.check(_lib.lib().siu3r_raster_tune(1, n), "siu3r_raster_tune")
    _lib.lib().siu3r_raster_tune(1, 6)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_composite_feat_ring_with_fewer_accumulator_blocks(n, feat_np):
    c = F.fwd_comp_case("feat_ring")
    feat_np(n)
    _check_feat(f"feat_ring np={n}", c, _composite_state(dict(c, feats=F.case_feats(c, 193))), 193)


@pytest.mark.parametrize("kind", ["k2", "k3", "feat"])
def test_forward_on_the_state_of_a_real_projection(kind):
    """project -> sort -> bin (-> tile lists) of the front-end, then the maps against the float64 walk of the records the device wrote"""
    import raster_stages_ref as RS
    from siu3r_amd import raster

    sc = B.forward_scene(kind)
    cams, V, G, H, W, Cc = sc["cams"], len(sc["cams"]), sc["means"].shape[0], sc["H"], sc["W"], sc["C"]
    m, cov, op, col = (_dev(sc[k]) for k in ("means", "cov6", "opac", "colors"))
    with torch.no_grad():
        if kind == "k2":
            o = raster.rasterize_views_k2(cams, m, cov, col, op)
            out, alpha, depth = o["image"].cpu().numpy().transpose(0, 2, 3, 1), o["opacity"].cpu().numpy(), o["depth"].cpu().numpy()
        else:
            o = raster.rasterize_views_k3_rgb(cams, m, cov, op, col) if kind == "k3" else raster.rasterize_views_k3(cams, m, cov, op, col)
            out, alpha, depth = o["colors"].cpu().numpy(), o["alphas"].cpu().numpy(), None
    fs = o["state"]
    geo = RS.geometry_ref(W, H)
    if kind == "feat":
        ts = fs["tile_start_all"].cpu().numpy()
        lists = [(ts[v, :geo["T"] + 1], fs["ids_all"][v, :ts[v, geo["T"] + 1]].cpu().numpy()) for v in range(V)]
    else:
        E = fs.totals(2)
        lists = [RS.tile_lists_ref(geo, fs["bin_start"][v].cpu().numpy(), fs["entries"][v, :E[v]].cpu().numpy()) for v in range(V)]
    case = dict(kind=kind, V=V, H=H, W=W, C=Cc, cams=cams, rec=fs["rec"].cpu().numpy(), lists=lists, feats=sc["colors"].numpy() if kind == "feat" else None,
                walk_cache=[{} for _ in range(V)])
    assert min(len(l[1]) for l in lists) > 1000
    F.check_maps(f"forward_{kind}", kind, F.comp_fwd_ref(case), out, alpha, depth, log=_log_maps)


def test_composite_refusals():
    c = F.fwd_comp_case("k3_satpair")
    st = _composite_state(c)
    V, G, H, W = 1, c["G"], c["H"], c["W"]
    image, alpha, nt = _f((V, H, W, 3)), _f((V, H, W)), _Guarded((V, G))
    a = [st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(image), None, _p(alpha), _p(nt)]
    _refused("siu3r_raster_composite_rgb", "n_touched belongs", *a, outs=[image, alpha, nt])
    a[-1], a[8] = None, None
    _refused("siu3r_raster_composite_rgb", "null pointer", *a, outs=[image, alpha])
