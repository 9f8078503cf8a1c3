"""CPU proofs of tests/dense_raster_fwd64.py, the float64 references and bounds that tests/test_raster_fwd_stages_gpu.py holds the
rasterizer's forward stages to:

  (a) a float32 emulation of every stage, in the kernels' expression order (project_kernel: numpy float32; the composites: the float32
      walk of dense_raster_bwd64 with the sums as fused multiply-adds), stays within the derived bound on every case, and its integer
      outputs equal the reference's on every decided row.  The worst ratios are printed; no bound is tuned to them;
  (b) every wrong answer of the list below exceeds the bound, or breaks an exactness rule, on at least one case;
  (c) every case populates the branches it is for, and the undecided rows / margin pixels stay under ZERO_SHARE_CAP (1 %).

Two wrong answers of the issue's list cannot be told from the right one by any input and are not in (b): "K2 rect by floor for truncation"
on the LOWER edges (after the clamp to [0, gw] both give 0 for every negative quotient; the upper edges, where K2's trunc((x + 15) / 16)
and K3's ceil(x / 16) differ, are swapped instead) and "a key not clamped" (no valid row has a depth whose bits reach 0xffffffff)."""
import copy

import numpy as np
import pytest

import dense_raster_bwd64 as B
import dense_raster_fwd64 as F

FILL = np.float32(-7.25)
ALL_COMP = list(F.FWD_COMP_CASES) + list(B.COMP_CASES)


# ---- projection ---------------------------------------------------------------------------------------------------------------------------
def _emulate(c, mutate=None, nf_loaded=None):
    """project_emul32 over the views of a case, in the layout check_projection takes"""
    nf = F.nf_chunk(c["cams"]) if nf_loaded is None else nf_loaded
    col = None if c["colors"] is None else c["colors"].numpy()
    outs = [F.project_emul32(c["mode"], cam, c["means"].numpy(), c["cov6"].numpy(), c["opac"].numpy(), col, c["planar"], nf, c["channels"], mutate)
            for cam in c["cams"]]
    rec = np.stack([o["rec"] for o in outs])
    rec = np.where(np.isnan(rec) & (np.arange(12) >= 8), FILL, rec).astype(np.float32)  # what rp[2] keeps where it is not written
    return dict(rec=rec, radii=np.stack([o["radii"] for o in outs]), rect=np.stack([o["rect"] for o in outs]), tiles=np.stack([o["tiles"] for o in outs]),
                keys=np.stack([o["keys"] for o in outs]), stats=[(int(o["valid"].sum()), int(o["tiles"].sum())) for o in outs], fill=FILL)


@pytest.mark.parametrize("name", F.PROJ_FWD_CASES)
def test_projection_emulation_within_bound(name):
    c = F.proj_fwd_case(name)
    worst, share = F.check_projection(c, F.proj_fwd_ref(name), _emulate(c))
    print(f"[fwd emulation] {name}: worst ratio to the bound per slot {({k: round(v, 3) for k, v in worst.items()})}, undecided rows {share:.4f}")


def _rejected(c, refs, got):
    try:
        F.check_projection(c, refs, got)
    except AssertionError:
        return True
    return False


PROJ_WRONG = {
    "tz < k2_znear_cull for <=": (dict(znear_lt=True), ["k2_depth"]),
    "limx / limy swapped": (dict(swap_lim=True), ["k2_deg0", "k3_rgb"]),
    "SH band 1 sign": (dict(sh_sign=1), ["k2_ch4"]),
    "SH band 2 sign": (dict(sh_sign=2), ["k2_ch9"]),
    "SH band 3 sign": (dict(sh_sign=3), ["k2_deg3"]),
    "SH band 4 sign": (dict(sh_sign=4), ["k2_deg4_band4"]),
    "planar read as interleaved": (dict(planar_as_interleaved=True), ["k2_mixed_planar", "k2_deg1_planar"]),
    "SH block loaded for the first view's degree only": (dict(sh_first_view_only=True), ["k2_mixed"]),
    "opacity-aware extent without the fminf": (dict(oae_no_min=True), ["k3_oae"]),
    "radius_clip compared with <": (dict(clip_lt=True), ["k3_clip"]),
    "K2 upper rect edge by ceil(x / 16)": (dict(k2_upper_ceil=True), ["k2_v33", "k2_ch9", "k2_edges"]),
    "K3 upper rect edge by trunc((x + 15) / 16)": (dict(k3_upper_trunc=True), ["k3_edges", "k3_oae", "k3_views"]),
    "a NaN mean / Inf covariance left valid": (dict(nonfinite_valid=True), ["k2_nonfinite", "k3_nonfinite"]),
}


@pytest.mark.parametrize("what", list(PROJ_WRONG))
def test_projection_wrong_answers_are_rejected(what):
    mutate, cases = PROJ_WRONG[what]
    hit = []
    for name in cases:
        c = F.proj_fwd_case(name)
        nf = 3 if "first view" in what else None  # (the degree-0 view's block: one coefficient)
        assert not _rejected(c, F.proj_fwd_ref(name), _emulate(c)), "the right answer must pass"
        if _rejected(c, F.proj_fwd_ref(name), _emulate(c, mutate, nf)):
            hit.append(name)
    assert hit, f"{what}: accepted on {cases}"
    if "NaN" in what:
        assert len(hit) == 2


def test_projection_case_populations():
    why = lambda name: np.stack([r["ints"]["why"] for r in F.proj_fwd_ref(name)])
    for name in ("k2_v16", "k2_v17", "k2_v33"):  # chunks of 16 views; the block behind is culled in a whole even chunk, the rest in a whole odd one
        w = why(name)
        V = w.shape[0]
        front = (w[:16] == 0).any(0)
        assert int(((w[:16] != 0).all(0)).sum()) >= 60, name
        if V > 16:
            assert int((front & (w[16:min(32, V)] != 0).all(0)).sum()) >= 100 and int(((w[16:min(32, V)] == 0).any(0) & ~front).sum()) >= 40, name
        assert all(int((w[v] == 0).sum()) >= 20 for v in range(V)), f"{name}: every view counts something (per-view stats)"
    w = why("k2_mixed")
    assert int(((w[0] != 0) & (w[1] == 0)).sum()) >= 40, "a block culled in the degree-0 view and seen by the degree-3 view"
    assert int(((w[:3] != 0).all(0) & (w[3] == 0)).sum()) >= 40, "a block visible from the degree-4 view only"
    assert int(((w[0] == 0) & (w[1] == 0)).sum()) >= 40, "rows first seen by the degree-0 view and read again at degree 3"
    c = F.proj_fwd_case("k3_oae")
    w, op, amin = why("k3_oae"), c["opac"].numpy().astype(np.float64), float(np.float32(c["cams"][0].alpha_min))
    lext = np.sqrt(2 * np.log(np.maximum(op / amin, 1.0)))
    assert int((w[0] == 3).sum()) >= 25 and int((op == amin).sum()) >= 3 and int(((w[0] == 0) & (lext < 2.0)).sum()) >= 20 and int(((w[0] == 0) & (lext > 2.0)).sum()) >= 100
    r = F.proj_fwd_ref("k3_clip")[0]["ints"]
    combos = {(int(a), int(b)) for a, b in r["radii"][r["valid"]]} | {(int(a), int(b)) for a, b in zip(*[np.ceil(x) for x in _clip_radii()])}
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (3, 3)} <= combos and int((r["why"] == 4).sum()) >= 30 and int(r["valid"].sum()) >= 40
    for name in ("k2_edges", "k3_edges"):
        c, r = F.proj_fwd_case(name), F.proj_fwd_ref(name)[0]
        mx, my, out = r["rec"][:, B.MX], r["rec"][:, B.MY], r["ints"]["why"] >= 5
        assert all(int((out & m).sum()) >= 8 for m in (mx < 0, mx > c["cams"][0].width, my < 0, my > c["cams"][0].height)), f"{name}: means off all four edges"
    for name, n in (("k2_depth", 6), ("k3_depth", 10)):
        r = F.proj_fwd_ref(name)[0]["ints"]
        assert int((r["why"] == 1).sum()) == n and r["decided"].all(), f"{name}: the exact depth rows decide with no margin"
    for name in ("k2_nonfinite", "k3_nonfinite"):
        assert (F.proj_fwd_ref(name)[0]["ints"]["why"][64:] == 2).all()


def _clip_radii():
    c = F.proj_fwd_case("k3_clip")
    r = F.proj_fwd_ref("k3_clip")[0]
    det = r["aux"]["det"].numpy()
    return 3.33 * np.sqrt(r["rec"][:, B.CC] * det), 3.33 * np.sqrt(r["rec"][:, B.CA] * det)


def test_pose_reference():
    """the adjugate inverse against numpy's, its stated evaluation error orders below an fp32 ulp, the singular pose, the fp32 t_scale product"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        E = B._c2w(rng).numpy()
        E[:3, 3] *= 10.0
        W, err = F.pose_inverse64(E)
        assert np.abs(W - np.linalg.inv(E)).max() <= 1e-13 and err.max() < 1e-13 < 0.5 * 2.0 ** -24 * 1e-4
    Z = np.eye(4)
    Z[:3, :3] = 0.0
    assert F.pose_inverse64(Z)[0] is None
    from siu3r_amd import raster

    cam = raster.make_cam_k2(None, None, None, None, None, [0, 0, 0], 96, 64, near=0.2, far=1000.0)
    c2w = B._c2w(rng).float().numpy()
    c2w[:3, 3] = [0.1, 0.2, 0.3]
    ref = F.pose_c2w64(cam, c2w, np.array([[0.9, 0, 0.45], [0, 1.3, 0.55], [0, 0, 1]], np.float32), 10.0)
    assert ref["campos"][0].tolist() == [float(np.float32(np.float32(x) * np.float32(10.0))) for x in (0.1, 0.2, 0.3)]
    # the lens: tan of half the angle between the K^-1 rays of the two edge midpoints, here by atan2(|a x b|, a . b) instead of acos
    fx, fy, cx, cy = (float(np.float32(x)) for x in (0.9, 1.3, 0.45, 0.55))
    ang = lambda a_, b_: np.arctan2(np.linalg.norm(np.cross(a_, b_)), a_ @ b_)
    ray = lambda x, y: np.array([(x - cx) / fx, (y - cy) / fy, 1.0])
    assert abs(ref["tanfovx"][0][0] - np.tan(0.5 * ang(ray(0, 0.5), ray(1, 0.5)))) < 1e-12 and abs(ref["tanfovy"][0][0] - np.tan(0.5 * ang(ray(0.5, 0), ray(0.5, 1)))) < 1e-12
    assert F.pose_close(np.float32(ref["w2c"][0]), ref["w2c"][0], ref["w2c"][1]) and not F.pose_close(np.nextafter(np.nextafter(np.float32(ref["w2c"][0]), np.float32(9)), np.float32(9)), ref["w2c"][0], ref["w2c"][1])


# ---- composites ---------------------------------------------------------------------------------------------------------------------------
def _emul_maps(c, C=None, mutate=None, ring_np=None):
    kind = c["kind"]
    feats = F.case_feats(c, C or c["C"]) if kind == "feat" else None
    outs = [F.composite_emul32(kind, c["cams"][v], c["rec"][v], c["lists"][v], feats, bool(c["cams"][v].nt_post_blend), mutate, ring_np) for v in range(c["V"])]
    k2 = kind == "k2"
    return ([o["out"] for o in outs], [o["alpha"] for o in outs], [o["depth"] for o in outs] if k2 else None, [o["n_touched"] for o in outs] if k2 else None)


@pytest.mark.parametrize("name", ALL_COMP)
def test_composite_emulation_within_bound(name):
    c = F.fwd_comp_case(name)
    w = F.check_maps(name, c["kind"], F.comp_fwd_ref(c), *_emul_maps(c))
    print(f"[fwd emulation] {name}: worst element {w:.3f} of its bound")


def _maps_rejected(c, C, mutate, ring_np=None):
    try:
        F.check_maps(c["name"], c["kind"], F.comp_fwd_ref(c, C), *_emul_maps(c, C, mutate, ring_np))
    except AssertionError:
        return True
    return False


COMP_WRONG = {
    "K3 pixel centres without the + 0.5": (dict(no_half=True), [("k3_satpair", None), ("feat_ring", 33)]),
    "the alpha_max clamp dropped": (dict(no_alpha_max=True), [("k2_small", None), ("k3_small", None)]),
    "background weighted by the transmittance before the last blend": (dict(bg_before_last=True), [("k2_pairs", None)]),
    "the dead second entry of a pair blended": (dict(dead_pair=True), [("k2_pairs", None)]),
    "a saturated pixel still blends the pair's second entry": (dict(sat_pair=True), [("k2_satpair", None), ("k3_satpair", None)]),
    "feature rows of chunk k from chunk k - 3's ring slot": (dict(ring_slot=True), [("feat_ring", 33)]),
    "the last channel window of a chunk not shifted": (dict(window_unshifted=True), [("feat_ring", 33), ("feat_ring", 65), ("feat_ring", 161)]),
    "the last chunk not shifted back": (dict(chunk_unshifted=True), [("feat_ring", 193), ("feat_ring", 385)]),
    "alpha written by a chunk other than 0": (dict(alpha_other_chunk=True), [("feat_c1", 1), ("feat_batch", 31)]),
}


@pytest.mark.parametrize("what", list(COMP_WRONG))
def test_composite_wrong_answers_are_rejected(what):
    mutate, runs = COMP_WRONG[what]
    hits = []
    for name, C in runs:
        c = F.fwd_comp_case(name)
        assert not _maps_rejected(c, C, None, 6), "the right answer must pass"
        hits.append(_maps_rejected(c, C, mutate, 6))
    assert all(hits) if "window" in what or "chunk not" in what else any(hits), (what, runs, hits)


@pytest.mark.parametrize("kind", ["k2", "k3"])
def test_the_other_saturation_comparison_is_rejected(kind):
    """< for <= at t_min and the reverse: as in test_raster_bwd_stages_ref.py, exact equality is the only place where they differ, and such a
    pixel has margin 0 in any real case; shown on a two-splat scene with thresholds that are binary fractions"""
    c = B.comp_case("k2_full" if kind == "k2" else "k3_full")
    cam = copy.copy(c["cams"][0])
    cam.alpha_max, cam.t_min = 1.0, 0.25
    off = 0.5 if kind == "k3" else 0.0
    rec = np.zeros((2, 12), np.float32)
    rec[:, 0], rec[:, 1] = 20.0 + off, 20.0 + off
    rec[:, 4], rec[:, 6], rec[:, 2], rec[:, 7], rec[:, 8:11] = 0.02, 0.02, (1.0, 2.0), (0.75, 0.5), 0.7
    T = (-(-cam.width // 16)) * (-(-cam.height // 16))
    lists = (np.arange(T + 1) * 2, np.tile(np.array([0, 1], np.int32), T))
    ref = F.composite_fwd64(kind, cam, rec, lists)
    right, wrong = (F.composite_emul32(kind, cam, rec, lists, mutate=m) for m in (None, dict(flip_sat=True)))
    assert ref["margin"][20, 20] == 0.0
    d = lambda o: abs(float(o["alpha"][20, 20]) - ref["alpha"][20, 20])
    assert d(right) <= ref["tol_alpha"][20, 20] < d(wrong)


def _quadrant_counts(c, v, tile):
    ts, ids = c["lists"][v]
    t_ids = np.asarray(ids[ts[tile]:ts[tile + 1]], np.int64)
    mk = F.quadrant_lists_k2(c["cams"][v], c["rec"][v], t_ids, tile, c["kind"] != "k2")
    return [int(((mk >> q) & 1).sum()) for q in range(4)], t_ids, mk


def test_composite_case_populations():
    gw = 6
    # k2_stage: the refill loop's counters, restated (no pixel of the three tiles stops the walk: checked below)
    c = F.fwd_comp_case("k2_stage")
    bs, ent = c["bins"][0]
    e0 = np.asarray(ent[bs[0]:bs[1]], np.int64)
    assert e0.shape[0] == 1104
    covers = lambda tx: np.array([((p & 31) <= tx < ((p >> 10) & 31)) and (((p >> 5) & 31) <= 0 < ((p >> 15) & 31)) for p in e0[:, 1]])
    r0, _ = F.refill_rounds(covers(0))
    assert int(covers(0).sum()) == 700 and int((~covers(0)).sum()) >= 300
    assert any(kk < F.FK and base < 1104 for _, kk, _, base in r0), "a refill commits fewer than FK slices and reads the rest again"
    r1, _ = F.refill_rounds(covers(1))
    assert any(F.STG_PULL - 8 <= s0 < F.STG_PULL for s0, _, _, _ in r1), "a refill round starts with staged just below STG_PULL"
    r2, w2 = F.refill_rounds(covers(2))
    assert any(F.STG_PULL <= st < F.STG_PULL + 8 and base < 1104 for _, _, st, base in r2) and w2 == 2, "the loop leaves with staged just above STG_PULL"
    ref = F.comp_fwd_ref(c)[0]
    for t in (0, 1, 2):
        w = ref["walks"][t]
        assert not (w["saturated"] | ~np.ones(256, bool)).all(), "the tile is never saturated as a whole: the restated counters are the kernel's"
    # k2_pairs: per-wave list lengths 0 .. 7
    c = F.fwd_comp_case("k2_pairs")
    for (tx, ty), want in F.PAIR_COUNTS.items():
        got, t_ids, mk = _quadrant_counts(c, 0, ty * gw + tx)
        assert tuple(got) == want, (tx, ty, got)
    assert F.comp_fwd_ref(c)[0]["blends"].mean() < 0.2, "most of the frame is background"
    # satpair: bands saturating on an even and on an odd list position, with static entries behind
    for name in ("k2_satpair", "k3_satpair"):
        c = F.fwd_comp_case(name)
        ref = F.comp_fwd_ref(c)[0]
        even = odd = behind = 0
        for tile, w in ref["walks"].items():
            got, t_ids, mk = _quadrant_counts(c, 0, tile)
            px, py, inside, _ = B._tile_pixels(c["cams"][0], tile, c["kind"] != "k2")
            sat_j = np.argmax(w["reached"] & w["static"] & ~w["bl"], 0)
            for q in range(4):
                pm = w["saturated"] & ((px % 16 >= 8) == bool(q & 1)) & ((py % 16 >= 8) == bool(q >> 1)) & (ref["margin"][np.minimum(py, 63), np.minimum(px, 95)] >= F.MARGIN)
                pos = np.cumsum((mk >> q) & 1) - 1  # position in the quadrant's list
                even += int((pos[sat_j[pm]] % 2 == 0).sum())
                odd += int((pos[sat_j[pm]] % 2 == 1).sum())
                behind += int((w["static"][np.minimum(sat_j[pm] + 1, len(t_ids) - 1), np.flatnonzero(pm)]).sum())
        assert even >= 30 and odd >= 30 and behind >= 60, (name, even, odd, behind)
    # feat_ring: the quadrant lists' lengths
    for name in ("feat_ring", "feat_ring_ragged"):
        c = F.fwd_comp_case(name)
        for v in range(c["V"]):
            ql = B.quadrant_lists_ref(c["cams"][v], c["rec"][v], c["lists"][v])
            g6 = -(-c["W"] // 16)
            assert [len(ql[(ty * g6 + tx, 0)]) for tx, ty in F.RING_TILES] == list(F.RING_LENGTHS), name
            assert any(len(x) == 0 for x in ql.values())
    c = F.fwd_comp_case("feat_batch")
    ts = c["lists"][0][0]
    assert [int(ts[ty * gw + tx + 1] - ts[ty * gw + tx]) for tx, ty in F.BATCH_TILES] == list(F.BATCH_LENGTHS)
    # feat_sat_early: quadrant 0 of tile (2, 1) is saturated inside its first chunk of 8, with 40 listed entries behind; quadrant 1 never is
    c = F.fwd_comp_case("feat_sat_early")
    tile = 1 * gw + 2
    ql = B.quadrant_lists_ref(c["cams"][0], c["rec"][0], c["lists"][0])
    w = F.comp_fwd_ref(c)[0]["walks"][tile]
    px, py, _, _ = B._tile_pixels(c["cams"][0], tile, True)
    q0, q1 = (px % 16 < 8) & (py % 16 < 8), (px % 16 >= 8) & (py % 16 < 8)
    assert len(ql[(tile, 0)]) == 48 and list(ql[(tile, 0)][:8]) == list(c["lists"][0][1][c["lists"][0][0][tile]:][:8]) and len(ql[(tile, 1)]) == 48
    assert w["saturated"][q0].all() and (np.argmax(w["reached"] & w["static"] & ~w["bl"], 0)[q0] < 8).all() and not w["saturated"][q1].all()
    # n_touched: both thresholds are populated, and the pre-blend form differs from the post-blend one
    post, pre = F.comp_fwd_ref(F.fwd_comp_case("k2_full"))[0], F.comp_fwd_ref(F.fwd_comp_case("k2_nt_pre"))[0]
    assert post["counts"]["nt_flip"] > 1000 and int((pre["nt_lo"] != post["nt_lo"]).sum()) > 50 and int((post["nt_lo"] > 200).sum()) >= 20
