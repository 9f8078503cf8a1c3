"""Every kernel of siu3r_amd/csrc/postprocess.hip called through the C ABI (siu3r_panoptic_stage1, siu3r_panoptic_qcl, siu3r_lift_ids) on
the crafted cases of tests/dense_panoptic64.py; every intermediate buffer is read back and each stage is held to its reference, fed
with the DEVICE's upstream buffers, under the bounds and decision rules derived in that file's header (proved on the CPU by
tests/test_panoptic_stages_ref.py).  Every output lies inside a sentinel-filled parent (_Guarded): the guards stay intact, and what the
kernels must leave unwritten (planes behind n_keep, kept_idx / acc_list tails, table rows of rejected slots, the label map of an empty
item) still holds the sentinel.

Where a line is run:

  pp_class_kernel
    Q walked by 64 threads               q1_c2 (1), q63_c2_b3 (63), q64_c33 (64), q65_c64 (65), net256 (100), tiled128 (128)
    C                                    2 (q1_c2, q63_c2_b3), 21, 33 (q64_c33), 64 (q65_c64); softmax at +-80 (q63_c2_b3, q64_c33, identity16)
    score == thr is not kept             q63_c2_b3 item 0 query 1: two equal logits at C = 2, score exactly 0.5, label 0 (the first)
    equal top logits, non-void           q64_c33 query 7 (classes 3 and 9: label 3)
    void / low score / keeps nothing     q63_c2_b3 item 1 (all void), identity16 query 5 (label 7, score far below thr), keeps all: item 2
    compaction, B = 3                    q63_c2_b3: n_keep = 22, 0, 63
    area / orig cleared                  test_second_call_on_the_same_buffers (nothing else clears them)
  pp_mask256_kernel
    pix >= OS * OS tail                  q63_c2_b3 (24^2 = 576), q64_c33 (40^2 = 1600)
    k >= n_keep[b] early return          every case with a dropped query; per item in q63_c2_b3; planes behind n_keep keep the sentinel
    (IH, IW)                             (1,1) q1_c2, (7,9) q63_c2_b3, (24,40) q64_c33, (32,32) net256 / q65_c64 [identity], (300,260) -> 256 down256
    T                                    1 (q1_c2, q65_c64, ...), 2 (q63_c2_b3, tiled128, net256), 3 (q64_c33)
  pp_argmax_kernel / pp_write_kernel
    pix < npix tail                      (1,1) q1_c2, (37,53) x 2 q63_c2_b3, (50,70) x 3 q64_c33, (300,40) q65_c64
    identity target                      tiled128, identity16, accept32, accept256, down256 (256 x 256)
    up in y, down in x                   q65_c64: 32 -> (300, 40)
    s_area / s_orig [128]                n_keep = 1, 64, 65, 128; tiled128: every one of the 128 counters ends at 16
    first maximum wins                   identity16 queries 0 / 1 and 3 / 4: bit-identical planes and class rows
    wv == mask_thr counts (>=)           identity16 query 0: sigmoid(0) x 1.0 on 128 pixels
    nk == 0                              q63_c2_b3 item 1, between two non-empty items: label map unwritten, maps zero
  pp_accept_kernel                       accept32, accept256: ratio 4 / 5 and 400 / 500 (== fp32(0.8): accepted, as the reference's double
                                         comparison does), 3 / 5, 1; area > 0 with orig == 0; orig > 0 with area == 0; two stuff-0 queries with
                                         a thing between; a stuff-0 query rejected before an accepted one; fused and unfused ids interleaved;
                                         cls >= 32 (q65_c64: never fused, never in the stuff memory, fuse bit 31 set beside it)
  pp_qcl_kernel
    min(256, npairs - pair0) tail        nq = 1, 2, 3, 7 at T H W = 2 x 37 x 53, 3 x 50 x 70, 300 x 40, 1
    C not dividing 256 pairs' run        C = 2, 21, 33, 64; b > 0: q63_c2_b3 item 2
  lift_pixel / lift_label / lift_fuse / fill_i32
    q C (lanes per pixel)                2 (62 lanes idle), 63, 64, 65, 126, 2100, 6400
    V H W (waves, partial last wave)     1, 63, 64, 65, 480, 4097; a query whose only pixel is the last one; a query that owns nothing
    ties                                 across queries, across classes, void against a class (void wins); values on a coarse grid everywhere
    threshold                            maximum == thr (kept), one ulp below (void)
    stuff bits                           sem 1 and 32 (bit 31) fuse, 33 cannot (qc6400_p65)

Worst element as a fraction of its bound on one MI355X (profiles/panoptic_parity.json, from one run of this file with
SIU3R_PANOPTIC_PARITY_LOG set; the bounds do not come from it): class 0.89 (q65_c64; 0.12 - 0.68 elsewhere), mask256 0.49 (q65_c64; 0.14 -
0.45 elsewhere), qcl 0.38 where the sample is interpolated (q64_c33) and 0.66 - 0.999 at identity sizes (accept32 / accept256 0.66,
tiled128 and identity16 0.96, down256 0.999), where the bound is the rounding of the one product; argmax, accept, write and lift are
integer stages, exact.  Undecided share: 1 pixel of 682 500 in q64_c33, none elsewhere (cap 0.005).  On the parent's kernels (float32
overlap comparison) test_stages[accept32], test_stages[accept256] and test_wrappers_accept_the_ratio_four_fifths fail, nothing else."""
import json
import os

import numpy as np
import pytest
import torch

import dense_panoptic64 as P
from test_raster_bwd_stages_gpu import _dev, _f, _ok, _p, _refused
from test_raster_stages_gpu import SENT, _Guarded

pytestmark = pytest.mark.gpu
assert SENT == P.SENT

_OUT = ("probs", "scores", "labels", "kept_idx", "n_keep", "p256", "lab_map", "area", "orig", "seg_id", "seg_label", "seg_fused", "seg_score",
        "acc_list", "n_acc", "seg", "sem", "ins")


def _log(**kw):
    if os.environ.get("SIU3R_PANOPTIC_PARITY_LOG"):
        with open(os.environ["SIU3R_PANOPTIC_PARITY_LOG"], "a") as f:
            f.write(json.dumps(kw) + "\n")


def _buffers(c):
    B, Q, C = c["cls"].shape
    T, MS, H, W = c["mcl"].shape[1], c["MS"], c["H"], c["W"]
    i, f = _Guarded, _f
    return dict(probs=f((B, Q, C)), scores=f((B, Q)), labels=i((B, Q)), kept_idx=i((B, Q)), n_keep=i((B,)), p256=f((B, T, Q, MS, MS)),
                lab_map=i((B, T, H, W)), area=i((B, Q)), orig=i((B, Q)), seg_id=i((B, Q)), seg_label=i((B, Q)), seg_fused=i((B, Q)),
                seg_score=f((B, Q)), acc_list=i((B, Q)), n_acc=i((B,)), seg=i((B, T, H, W)), sem=i((B, T, H, W)), ins=i((B, T, H, W)))


def _stage1_args(c, bufs, cls, mcl, **over):
    B, Q, C = c["cls"].shape
    T, IH, IW = c["mcl"].shape[1:4]
    fuse_mask = sum(1 << s for s in c["fuse"])
    dims = dict(B=B, T=T, Q=Q, C=C, IH=IH, IW=IW, H=c["H"], W=c["W"], MS=c["MS"])
    dims.update(over)
    return [_p(cls), _p(mcl), *[_p(bufs[k]) for k in _OUT], *[dims[k] for k in ("B", "T", "Q", "C", "IH", "IW", "H", "W", "MS")],
            c["thr"], c["mask_thr"], c["overlap"], fuse_mask]


def _stage1(c, bufs=None):
    """one call of siu3r_panoptic_stage1 -> the read-back buffers (numpy), the device buffers"""
    bufs = bufs or _buffers(c)
    cls, mcl = _dev(c["cls"]), _dev(c["mcl"])
    _ok("siu3r_panoptic_stage1", *_stage1_args(c, bufs, cls, mcl))
    for k, b in bufs.items():
        assert b.guards_intact(), f"{k}: written outside the buffer"
    return {k: b.t.cpu().numpy() for k, b in bufs.items()}, bufs


def _check_stages(c, o, bufs, fresh=True):
    for stage, check in P.STAGE_CHECKS:
        worst, und, tot = check(c, o, fresh=fresh)
        share = und / max(tot, 1)
        print(f"[panoptic parity] {c['name']} {stage}: worst element {worst:.3f} of its bound, undecided share {share:.5f}")
        _log(case=c["name"], stage=stage, worst_ratio_to_bound=worst, undecided_share=share)
        assert share <= P.UNDECIDED_CAP
    B, Q, C = c["cls"].shape
    T, H, W = c["mcl"].shape[1], c["H"], c["W"]
    for b, nq in P.qcl_runs(c, o):
        out = _f((T * H * W, nq, C))
        _ok("siu3r_panoptic_qcl", _p(bufs["p256"]), _p(bufs["probs"]), _p(bufs["kept_idx"]), _p(bufs["acc_list"]), nq, _p(out), b, T, H, W, c["MS"], Q, C)
        assert out.guards_intact(), f"qcl item {b} nq {nq}: written outside the buffer"
        worst, _, _ = P.check_qcl(c, o, nq, b, out.t.cpu().numpy())
        print(f"[panoptic parity] {c['name']} qcl item {b} nq {nq}: worst element {worst:.3f} of its bound")
        _log(case=c["name"], stage=f"qcl b{b} nq{nq}", worst_ratio_to_bound=worst, undecided_share=0.0)


@pytest.mark.parametrize("name", P.STAGE1_CASES)
def test_stages(name):
    c = P.stage1_case(name)
    o, bufs = _stage1(c)
    _check_stages(c, o, bufs)
    if name.startswith("accept"):  # the table the case is built for: 4 / 5 and 400 / 500 accepted
        acc = o["acc_list"][0, :o["n_acc"][0]].tolist()
        assert [(k, int(o["seg_id"][0, k]), int(o["seg_label"][0, k]), int(o["seg_fused"][0, k])) for k in acc] == P.ACCEPT_EXPECT
        assert (int(o["area"][0, 1]), int(o["orig"][0, 1]), int(o["area"][0, 2]), int(o["orig"][0, 2])) == (4, 5, 400, 500)
    if name == "tiled128":
        assert (o["area"][0] == 16).all() and (o["orig"][0] == 16).all() and o["n_acc"][0] == 128


def test_second_call_on_the_same_buffers():
    """pp_class clears area / orig and nothing else does: a second call with other inputs on the same buffers gives the second input's
    answer (items rolled: the empty item moves, every n_keep changes)"""
    c = P.stage1_case("q63_c2_b3")
    o, bufs = _stage1(c)
    P.check_argmax(c, o)
    c2 = P.rolled(c)
    o2, _ = _stage1(c2, bufs)
    assert o2["n_keep"].tolist() == np.roll(o["n_keep"], 1).tolist() != o["n_keep"].tolist()
    for stage, check in P.STAGE_CHECKS:
        check(c2, o2, fresh=False)
    for k in ("area", "orig", "seg", "sem", "ins", "seg_id", "n_acc"):
        assert np.array_equal(o2[k], np.roll(o[k], 1, 0)), k


@pytest.mark.parametrize("name", list(P.LIFT_CASES))
def test_lift(name):
    c = P.lift_case(name)
    V, H, W, q, C = c["V"], c["H"], c["W"], c["q"], c["C"]
    qc = _dev(c["qc"])
    sem, ins = _Guarded((V, H, W), torch.int64), _Guarded((V, H, W), torch.int64)
    first, qlab = _Guarded((q,)), _Guarded((q,))
    _ok("siu3r_lift_ids", _p(qc), V, H, W, q, C, c["thr"], c["num_queries"], c["stuff_mask"], _p(sem), _p(ins), _p(first), _p(qlab))
    for k, b in dict(sem=sem, ins=ins, first=first, qlab=qlab).items():
        assert b.guards_intact(), f"{k}: written outside the buffer"
    P.check_lift(c, *[b.t.cpu().numpy() for b in (sem, ins, first, qlab)])
    _log(case=name, stage="lift", worst_ratio_to_bound=0.0, undecided_share=0.0)


def test_refusals():
    """Q = 129, C = 65, a null pointer; nq == 0; q == 0, C == 1: an error string, and nothing is launched (every output keeps the sentinel)"""
    c = P.stage1_case("q1_c2")
    bufs = _buffers(c)
    cls, mcl = _dev(c["cls"]), _dev(c["mcl"])
    outs = list(bufs.values())
    _refused("siu3r_panoptic_stage1", "up to 128 queries", *_stage1_args(c, bufs, cls, mcl, Q=129), outs=outs)
    _refused("siu3r_panoptic_stage1", "up to 128 queries", *_stage1_args(c, bufs, cls, mcl, C=65), outs=outs)
    args = _stage1_args(c, bufs, cls, mcl)
    _refused("siu3r_panoptic_stage1", "null pointer", None, *args[1:], outs=outs)
    _refused("siu3r_panoptic_stage1", "null pointer", *args[:7], None, *args[8:], outs=outs)  # p256
    out = _f((1, 1, 2))
    q = [_p(bufs["p256"]), _p(bufs["probs"]), _p(bufs["kept_idx"]), _p(bufs["acc_list"])]
    _refused("siu3r_panoptic_qcl", "bad arguments", *q, 0, _p(out), 0, 1, 1, 1, 16, 1, 2, outs=[out])
    _refused("siu3r_panoptic_qcl", "bad arguments", *q, 1, None, 0, 1, 1, 1, 16, 1, 2, outs=[out])
    l = P.lift_case("qc2_p1")
    qc = _dev(l["qc"])
    sem, ins, first, qlab = _Guarded((1,), torch.int64), _Guarded((1,), torch.int64), _Guarded((1,)), _Guarded((1,))
    tail = [0.3, 100, 0, _p(sem), _p(ins), _p(first), _p(qlab)]
    _refused("siu3r_lift_ids", "bad arguments", _p(qc), 1, 1, 1, 0, 2, *tail, outs=[sem, ins, first, qlab])
    _refused("siu3r_lift_ids", "bad arguments", _p(qc), 1, 1, 1, 1, 1, *tail, outs=[sem, ins, first, qlab])
    _refused("siu3r_lift_ids", "bad arguments", None, 1, 1, 1, 1, 2, *tail, outs=[sem, ins, first, qlab])


# ---- the same through the Python wrappers ----------------------------------------------------------------------------------------------------
def _through_the_wrappers(cls, msk, target, fuse):
    """post_process_panoptic_segmentation and lift_query_class_logits against the oracle on the same logits, as
    tests/test_postprocess_gpu.py compares them"""
    from oracle import siu3r_oracle as O
    from siu3r_amd.gaussian_renderer import lift_query_class_logits
    from siu3r_amd.postprocess import VideoMask2FormerImageProcessor

    ref = O.panoptic_postprocess(cls, msk, target, fuse=tuple(fuse))
    out = dict(class_queries_logits=cls.cuda(), masks_queries_logits=msk.cuda())
    res = VideoMask2FormerImageProcessor().post_process_panoptic_segmentation(out, threshold=0.5, target_sizes=[target] * cls.shape[0], label_ids_to_fuse=set(fuse))
    assert len(res) == len(ref)
    strip = lambda segs: [(s_["id"], s_["label_id"], s_["was_fused"]) for s_ in segs]
    for b, (r, m) in enumerate(zip(ref, res)):
        assert m["segmentation"].dtype == r["segmentation"].dtype and torch.equal(m["segmentation"].cpu(), r["segmentation"]), f"segmentation differs for item {b}"
        assert strip(m["segments_info"]) == strip(r["segments_info"]), (b, m["segments_info"], r["segments_info"])
        assert all(abs(x["score"] - y["score"]) <= 2e-6 for x, y in zip(m["segments_info"], r["segments_info"]))
        assert tuple(m["query_class_logits"].shape) == tuple(r["query_class_logits"].shape), (b, m["query_class_logits"].shape, r["query_class_logits"].shape)
        assert float((m["query_class_logits"].cpu() - r["query_class_logits"]).abs().max()) <= 2e-6
        # lifting of the device's own volume (a stand-in for the rendered one) against the oracle on the same numbers
        qc = m["query_class_logits"]
        sem, ins, infos = lift_query_class_logits([qc], [m["query_scores"]], num_queries=100, label_ids_to_fuse=tuple(fuse))
        sem_o, ins_o, info_o = O.lift_ids(qc.cpu(), m["query_scores"], 100, tuple(fuse), 0.3)
        assert torch.equal(sem[0].cpu(), sem_o) and torch.equal(ins[0].cpu(), ins_o) and infos[0] == info_o, b
    return ref, res


def test_wrappers_accept_the_ratio_four_fifths():
    c = P.stage1_case("accept256")
    ref, res = _through_the_wrappers(torch.from_numpy(c["cls"]), torch.from_numpy(c["msk"]), (256, 256), c["fuse"])
    assert [(s_["id"], s_["label_id"]) for s_ in res[0]["segments_info"]] == [(e[1], e[2]) for e in P.ACCEPT_EXPECT]


def test_wrappers_at_a_ragged_size_with_three_views():
    """target (37, 53), T = 3, an empty item in front of the kept-but-none-accepted one: the reference's stale (height, width) quirk at a
    ragged size"""
    from crafted import crafted_panoptic_inputs, permuted

    cls, msk = permuted(*crafted_panoptic_inputs(T=3), [1, 2, 0, 3])
    ref, res = _through_the_wrappers(cls, msk, (37, 53), (0, 1))
    assert ref[0]["segments_info"] == [] and ref[1]["segments_info"] == [] and tuple(ref[1]["query_class_logits"].shape[-2:]) == (37, 53)
    assert len(ref[2]["segments_info"]) >= 3
