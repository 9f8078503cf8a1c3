"""CPU proof of tests/dense_panoptic64.py, the yardstick of tests/test_panoptic_stages_gpu.py: the stage references agree with the pinned
restatement (oracle/siu3r_oracle.py: panoptic_postprocess, scatter_labels, lift_ids) on every case, from the same float32 inputs; a
float32 emulation of every stage in the kernels' operation order lies inside the derived bounds; one deliberately wrong answer per stage
falls outside; the undecided share of every case is at most UNDECIDED_CAP; and every case populates the branch it is listed for."""
import functools

import numpy as np
import pytest
import torch

import dense_panoptic64 as P

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _emulated(name):
    c = P.stage1_case(name)
    return c, P.emulate_stage1(c)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import siu3r_oracle as O

    c = P.stage1_case(name)
    return O.panoptic_postprocess(torch.from_numpy(c["cls"]), torch.from_numpy(c["msk"]), (c["H"], c["W"]), c["thr"], c["mask_thr"], c["overlap"],
                                  c["fuse"], mask_size=c["MS"])


@pytest.mark.parametrize("name", P.STAGE1_CASES)
def test_references_agree_with_the_oracle(name):
    """segment tables, id maps (on decided pixels), label scatter and the query x class volume of the stage references, fed with the
    float32 emulation's upstream buffers, against the oracle on the same logits: integers exact, floats within float32 rounding"""
    from oracle import siu3r_oracle as O

    c, o = _emulated(name)
    res = _oracle(name)
    B, Q, C = c["cls"].shape
    T, H, W = c["mcl"].shape[1], c["H"], c["W"]
    sem_o, ins_o = O.scatter_labels(res, B, T, H, W)
    r_cls = P.class_ref(c["cls"], c["thr"])
    assert r_cls["keep_decided"].all() and r_cls["label_decided"].all(), "the cases leave no class decision open"
    for b, r in enumerate(res):
        keep = np.flatnonzero(r_cls["keep"][b])
        assert int(o["n_keep"][b]) == len(keep) and np.array_equal(o["kept_idx"][b, :len(keep)], keep)
        if len(keep) == 0:
            assert r["segments_info"] == [] and bool((r["segmentation"] == -1).all())
            continue
        am = P.argmax_ref(o["p256"], o["scores"], o["kept_idx"], o["n_keep"], b, H, W, c["mask_thr"])
        if am["decided"].all() and am["undecided_pairs"] == 0:  # the counters are then those of the reference alone
            area, orig = np.zeros((B, Q), np.int32), np.zeros((B, Q), np.int32)
            area[b, :len(keep)], orig[b, :len(keep)] = am["area_lo"], am["orig_lo"]
        else:
            area, orig = o["area"], o["orig"]
        seg_id, rows, acc = P.accept_ref(area, orig, o["kept_idx"], o["n_keep"], r_cls["label"], r_cls["score"].astype(F32), b, c["overlap"], c["fuse"])
        got = [dict(id=int(seg_id[k]), label_id=rows[k][0], was_fused=bool(rows[k][1])) for k in acc]
        assert got == [{k: v for k, v in s.items() if k != "score"} for s in r["segments_info"]], (b, got, r["segments_info"])
        assert all(abs(float(rows[k][2]) - s["score"]) <= 5e-7 + 4 * P.U for k, s in zip(acc, r["segments_info"]))  # (rounded to 6 decimals by the reference)
        seg_label = np.zeros((B, Q), np.int32)
        for k in acc:
            seg_label[b, k] = rows[k][0]
        tab = np.zeros((B, Q), np.int32)
        tab[b] = seg_id
        seg, sem, ins = P.write_ref(am["best"][None].repeat(B, 0), tab, seg_label, o["n_keep"], b)
        d = am["decided"]
        assert np.array_equal(seg[d], r["segmentation"].numpy()[d]), f"item {b}: segmentation differs on decided pixels"
        assert np.array_equal(sem.reshape(-1)[d.reshape(-1)], sem_o[b].numpy()[d.reshape(-1)]) and np.array_equal(ins.reshape(-1)[d.reshape(-1)], ins_o[b].numpy()[d.reshape(-1)])
        if acc:
            nq = min(len(acc), 7)
            accl = np.zeros((B, Q), np.int32)
            accl[b, :len(acc)] = acc
            ref, bound = P.qcl_ref(o["p256"], o["probs"], o["kept_idx"], accl, nq, b, H, W)
            want = r["query_class_logits"][:, :nq].permute(0, 3, 4, 1, 2).reshape(-1, nq, C).numpy()
            assert (np.abs(ref - want) <= 2e-6 + 2 * bound).all(), float(np.abs(ref - want).max())


@functools.lru_cache(maxsize=None)
def _checked(name):
    c, o = _emulated(name)
    out = {stage: f(c, o) for stage, f in P.STAGE_CHECKS}
    for b, nq in P.qcl_runs(c, o):
        out[f"qcl b{b} nq{nq}"] = P.check_qcl(c, o, nq, b, P.emulate_qcl(c, o, nq, b))
    return out


@pytest.mark.parametrize("name", P.STAGE1_CASES)
def test_float32_emulation_lies_inside_the_bounds(name):
    for stage, (worst, und, tot) in _checked(name).items():
        print(f"[panoptic emulation] {name} {stage}: worst element {worst:.3f} of its bound, undecided {und} of {tot}")
        assert worst <= 1.0


@pytest.mark.parametrize("name", P.STAGE1_CASES)
def test_undecided_share_is_capped(name):
    for stage, (_, und, tot) in _checked(name).items():
        assert und <= P.UNDECIDED_CAP * tot, (stage, und, tot)


@pytest.mark.parametrize("variant, case, stage", [("noclamp", "q63_c2_b3", "mask256"), ("align", "q63_c2_b3", "mask256"), ("lastmax", "identity16", "argmax"),
                                                  ("gt", "identity16", "argmax"), ("f32overlap", "accept32", "accept")])
def test_a_wrong_stage_falls_outside(variant, case, stage):
    """src_idx without the clamp at 0, align_corners=True sampling, last-maximum argmax, > for >= at the mask threshold, a float32
    overlap comparison: the stage's check refuses each (and the stages in front of it still pass)"""
    c = P.stage1_case(case)
    o = P.emulate_stage1(c, variant)
    for name, f in P.STAGE_CHECKS:
        if name == stage:
            with pytest.raises(AssertionError):
                f(c, o)
            return
        f(c, o)


def _lift_emulated(c, variant=None):
    return P.lift_ref(c["qc"], c["q"], c["C"], c["thr"], c["num_queries"], c["stuff_mask"], variant)


@pytest.mark.parametrize("variant", ["unrolled", "lastquery"])
def test_a_wrong_lift_falls_outside(variant):
    c = P.lift_case("qc126_p480")
    with pytest.raises(AssertionError):
        P.check_lift(c, *_lift_emulated(c, variant))
    P.check_lift(c, *_lift_emulated(c))


@pytest.mark.parametrize("name", list(P.LIFT_CASES))
def test_lift_reference_agrees_with_the_oracle(name):
    from oracle import siu3r_oracle as O

    c = P.lift_case(name)
    q, C, V, H, W = c["q"], c["C"], c["V"], c["H"], c["W"]
    sem, ins, first, qlab = _lift_emulated(c)
    fuse = tuple(s for s in range(32) if (c["stuff_mask"] >> s) & 1)
    qc = torch.from_numpy(c["qc"]).view(V, H, W, q, C).permute(0, 3, 4, 1, 2)
    scores = [0.5 + 0.001 * i for i in range(q)]
    sem_o, ins_o, info_o = O.lift_ids(qc, scores, c["num_queries"], fuse, c["thr"])
    assert np.array_equal(sem, sem_o.numpy().reshape(-1)) and np.array_equal(ins, ins_o.numpy().reshape(-1))
    info = []  # (as siu3r_amd.gaussian_renderer.lift_query_class_logits builds it from q_label)
    for i in range(q):
        if qlab[i] >= 0:
            fused = (qlab[i] - 1) in fuse
            info.append({"id": c["num_queries"] + int(qlab[i]) if fused else i + 1, "label_id": int(qlab[i]), "was_fused": fused, "score": scores[i]})
    assert info == info_o


def test_every_stage1_case_populates_its_branch():
    U = {n: _emulated(n) for n in P.STAGE1_CASES}
    nk = {n: o["n_keep"].tolist() for n, (c, o) in U.items()}
    assert nk["q1_c2"] == [1] and nk["q63_c2_b3"] == [22, 0, 63] and nk["q64_c33"] == [64] and nk["q65_c64"] == [65] and nk["tiled128"] == [128]
    assert {c["cls"].shape[1] for c, _ in U.values()} >= {1, 63, 64, 65, 100, 128} and {c["cls"].shape[2] for c, _ in U.values()} >= {2, 21, 33, 64}
    assert {c["mcl"].shape[1] for c, _ in U.values()} == {1, 2, 3}
    assert {c["mcl"].shape[2:4] for c, _ in U.values()} >= {(1, 1), (7, 9), (24, 40), (32, 32), (300, 260)}
    assert {(c["H"], c["W"]) for c, _ in U.values()} >= {(1, 1), (16, 16), (37, 53), (50, 70), (64, 64), (300, 40), (256, 256), (32, 32)}
    assert {c["MS"] for c, _ in U.values()} >= {16, 24, 32, 40, 256} and (24 * 24) % 256 and (40 * 40) % 256
    for n in ("q63_c2_b3", "q64_c33", "q65_c64"):  # tails of pp_argmax / pp_write, and of pp_qcl for every nq
        c, o = U[n]
        npix = c["mcl"].shape[1] * c["H"] * c["W"]
        assert npix % 256 and all((npix * nq) % 256 for nq in c["nqs"]) and {nq for _, nq in P.qcl_runs(c, o)} == {1, 2, 3, 7}
    assert any(b > 0 for b, _ in P.qcl_runs(*U["q63_c2_b3"]))
    # class edges
    c, o = U["q63_c2_b3"]
    r = P.class_ref(c["cls"], c["thr"])
    assert r["exact"][0, 1] and o["scores"][0, 1] == F32(0.5) and o["labels"][0, 1] == 0 and 1 not in o["kept_idx"][0, :22]
    assert o["scores"][0, 2] == F32(1.0) and 2 in o["kept_idx"][0, :22] and o["labels"][0, 4] == 1
    c, o = U["q64_c33"]
    assert o["labels"][0, 7] == 3 and c["cls"][0, 7, 3] == c["cls"][0, 7, 9] and o["scores"][0, 5] == F32(1.0)
    c, o = U["q65_c64"]
    acc = o["acc_list"][0, :o["n_acc"][0]]
    lab = o["seg_label"][0, acc]
    assert (lab >= 32).any() and not o["seg_fused"][0, acc][lab >= 32].any() and o["seg_fused"][0, acc][lab < 32].any()
    assert len(set(o["seg_id"][0, acc][lab >= 32].tolist())) == int((lab >= 32).sum()), "a class >= 32 never shares an id"
    c, o = U["tiled128"]
    assert (o["area"][0] == 16).all() and (o["orig"][0] == 16).all() and o["n_acc"][0] == 128
    c, o = U["down256"]
    assert c["mcl"].shape[2] > c["MS"] and c["mcl"].shape[3] > c["MS"]
    c, o = U["net256"]
    assert o["n_keep"][0] == 14 and o["n_acc"][0] >= 5 and o["seg_fused"][0, o["acc_list"][0, :o["n_acc"][0]]].any()
    c, o = U["identity16"]
    wv = o["p256"][0, 0, 0] * o["scores"][0, 0]
    assert (wv == F32(0.5)).sum() == 128 and o["orig"][0, 0] == 128 and o["area"][0, 0] == 128 and o["area"][0, 1] == 0 and o["orig"][0, 1] == 128
    assert o["area"][0, 4] == 0 and o["area"][0, 3] == 64 and o["labels"][0, 5] == 7 and o["scores"][0, 5] < 0.5 and o["n_keep"][0] == 5


@pytest.mark.parametrize("name", ["accept32", "accept256"])
def test_accept_cases_hold_the_counts_they_are_built_for(name):
    c, o = _emulated(name)
    for k, (a, orig) in P.ACCEPT_COUNTS.items():
        assert (int(o["area"][0, k]), int(o["orig"][0, k])) == (a, orig), k
    assert o["area"][0, 0] > 0 and o["orig"][0, 0] == 0 and o["area"][0, 5] == c["H"] * c["W"] // 4 and o["orig"][0, 5] == 0
    acc = o["acc_list"][0, :o["n_acc"][0]].tolist()
    assert [(k, int(o["seg_id"][0, k]), int(o["seg_label"][0, k]), int(o["seg_fused"][0, k])) for k in acc] == P.ACCEPT_EXPECT
    # at least one segment accepted at ratio == fp32(0.8): the double comparison accepts it, a float32 one does not
    assert F32(4) / F32(5) == F32(0.8) == F32(400) / F32(500) and float(F32(4) / F32(5)) > 0.8 and not F32(4) / F32(5) > F32(0.8)
    assert [s["id"] for s in _oracle(name)[0]["segments_info"]] == [e[1] for e in P.ACCEPT_EXPECT]


def test_every_lift_case_populates_its_branch():
    assert sorted(c[0] * c[1] for c in P.LIFT_CASES.values()) == [2, 63, 64, 65, 126, 2100, 6400]
    assert sorted(c[2] * c[3] * c[4] for c in P.LIFT_CASES.values()) == [1, 63, 64, 65, 65, 480, 4097]
    for name in P.LIFT_CASES:
        c = P.lift_case(name)
        sem, ins, first, qlab = _lift_emulated(c)
        q, npix, cr = c["q"], c["qc"].shape[0], c["crafted"]
        if cr:
            cq = min(2, c["C"] - 2)
            assert (sem[cr["void_tie"]], ins[cr["void_tie"]]) == (0, 0)
            assert sem[cr["query_tie"]] == cq + 1 and (ins[cr["query_tie"]] == 1 or (c["stuff_mask"] >> cq) & 1)
            assert sem[cr["class_tie"]] == cq + 1 and (c["C"] <= 3 or ins[cr["class_tie"]] == q)
            assert sem[cr["at_thr"]] == cq + 1 and sem[cr["below_thr"]] == 0 and ins[cr["below_thr"]] == 0
        if c["owner"] is not None:
            assert first[c["owner"]] == npix - 1 and npix % 64 and qlab[c["owner"]] == 1 and qlab[q - 3] == -1 and first[q - 3] == 0x7fffffff
        if "stuff32" in cr:
            assert (sem[cr["stuff1"]], ins[cr["stuff1"]]) == (1, 101) and (sem[cr["stuff32"]], ins[cr["stuff32"]]) == (32, 132)
            assert (sem[cr["unfusable33"]], ins[cr["unfusable33"]]) == (33, 6)
