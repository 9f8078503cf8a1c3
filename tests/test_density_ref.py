"""Adaptive density control without a GPU: the schedule (DensityControl.events), the scene extent, the float64 restatement's own hand cases
(tests/dense_density64.py: every threshold hit exactly) and the C ABI's new declarations."""
import math
import os
import re

import pytest
import torch

import dense_density64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_schedule_is_one_event_at_100_and_no_reset():
    from siu3r_amd.density import DensityControl

    assert DensityControl().events(200) == ([100], [])


def test_schedule_edges():
    from siu3r_amd.density import DensityControl as C

    assert C().events(99) == ([], []) and C().events(100) == ([], [])  # iters <= start: nothing (iteration 100 does not exist in 100 iterations)
    assert C(start=50).events(49) == ([], [])
    assert C(start=10, every=10).events(30) == ([10, 20], [])  # stop = None -> iters - every: the last event leaves `every` steps
    assert C(start=10, every=10, stop=10).events(100) == ([10], [])  # stop is inclusive
    assert C(start=10, every=10, stop=9).events(100) == ([], [])
    assert C(start=10, every=10, stop=1000).events(35) == ([10, 20, 30], [])  # never past the run
    assert C(start=10, every=7, stop=30).events(100) == ([10, 17, 24], [])
    assert C(start=0, every=10, stop=20).events(100) == ([10, 20], [])  # iteration 0 has no statistics
    assert C(start=10, every=1, stop=12).events(100) == ([10, 11, 12], [])
    assert C(start=10, every=10, stop=40, reset_every=15).events(100) == ([10, 20, 30, 40], [15, 30])  # resets up to stop
    assert C(start=10, every=10, stop=40, reset_every=40).events(100) == ([10, 20, 30, 40], [40])
    assert C(start=10, every=10, stop=40, reset_every=41).events(100)[1] == []
    with pytest.raises(ValueError):
        C(every=0).events(100)


def test_scene_extent_hand_case():
    from siu3r_amd.density import DensityControl, scene_extent

    c2w = torch.eye(4)[None].repeat(3, 1, 1)
    c2w[0, :3, 3] = torch.tensor([0.0, 0.0, 0.0])
    c2w[1, :3, 3] = torch.tensor([3.0, 0.0, 0.0])
    c2w[2, :3, 3] = torch.tensor([0.0, 6.0, 0.0])
    # mean (1, 2, 0); distances sqrt(5), sqrt(8), sqrt(17)
    assert scene_extent(c2w) == pytest.approx(1.1 * math.sqrt(17.0), rel=1e-12)
    with pytest.raises(ValueError, match="scene_extent"):
        scene_extent(c2w[:1])
    with pytest.raises(ValueError, match="scene_extent"):
        scene_extent(c2w[:1].repeat(4, 1, 1))
    bad = c2w.clone()
    bad[1, 0, 3] = float("nan")
    with pytest.raises(ValueError):
        scene_extent(bad)
    for e in (0.0, float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError):
            DensityControl().thresholds(e)


def test_thresholds_are_float32_numbers():
    from siu3r_amd.density import DensityControl

    t = DensityControl(max_world_scale_frac=0.1, max_screen_radius=20).thresholds(3.0)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float64).float())
    assert t["grad_threshold"] == f32(2e-4) and t["log_dense_scale"] == f32(math.log(0.03)) and t["logit_min_opacity"] == f32(math.log(0.005 / 0.995))
    assert t["log_max_world_scale"] == f32(math.log(0.3)) and t["max_screen_radius"] == 20
    assert DensityControl().thresholds(3.0)["log_max_world_scale"] == math.inf


THR = dict(grad_threshold=0.25, log_dense_scale=-2.0, logit_min_opacity=-5.0)


def _plan(rows, **kw):
    """rows of (grad_accum, seen, max_radius, top log-scale, logit opacity)"""
    t = torch.tensor(rows, dtype=torch.float64)
    ls = torch.stack((t[:, 3] - 1.0, t[:, 3], t[:, 3] - 0.5), -1).float()
    return D.plan(t[:, 0].float(), t[:, 1].int(), t[:, 2].int(), ls, t[:, 4].float(), **dict(THR, **kw))


def test_reference_thresholds_are_hit_exactly():
    # avg = 0.5 / 2 = the threshold exactly: >= densifies; one ulp less does not
    below = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
    a, _, _ = _plan([(0.5, 2, 0, -3.0, 0.0), (below, 2, 0, -3.0, 0.0)])
    assert a.tolist() == [D.CLONE, D.KEEP]
    # top log-scale exactly on the dense scale: > is needed for a split, so it clones; one ulp above splits
    above = float(torch.nextafter(torch.tensor(-2.0), torch.tensor(0.0)))
    a, _, _ = _plan([(1.0, 1, 0, -2.0, 0.0), (1.0, 1, 0, above, 0.0)])
    assert a.tolist() == [D.CLONE, D.SPLIT]
    # logit opacity exactly on the threshold: < prunes, so it stays; one ulp below goes
    under = float(torch.nextafter(torch.tensor(-5.0), torch.tensor(-10.0)))
    a, _, _ = _plan([(0.0, 1, 0, -3.0, -5.0), (0.0, 1, 0, -3.0, under)])
    assert a.tolist() == [D.KEEP, D.PRUNE]
    # the two optional prune rules: strictly above
    a, _, _ = _plan([(0.0, 1, 20, -3.0, 0.0), (0.0, 1, 21, -3.0, 0.0)], max_screen_radius=20)
    assert a.tolist() == [D.KEEP, D.PRUNE]
    a, _, _ = _plan([(0.0, 1, 21, -3.0, 0.0)])  # off by default
    assert a.tolist() == [D.KEEP]
    a, _, _ = _plan([(0.0, 1, 0, -1.0, 0.0), (0.0, 1, 0, -0.5, 0.0)], log_max_world_scale=-1.0)
    assert a.tolist() == [D.KEEP, D.PRUNE]


def test_reference_precedence_and_counts():
    rows = [(9.0, 0, 0, 0.0, 0.0),     # never seen: no average, never densifies
            (9.0, 3, 0, 0.0, -9.0),    # hot and big and transparent: the prune wins over the split
            (9.0, 3, 0, -3.0, -9.0),   # ... and over the clone
            (9.0, 3, 0, 0.0, 0.0),     # split
            (9.0, 3, 0, -3.0, 0.0),    # clone
            (0.1, 3, 0, 0.0, 0.0),     # cold
            (9.0, 3, 0, -3.0, 0.0)]    # clone
    a, off, tot = _plan(rows)
    assert a.tolist() == [D.KEEP, D.PRUNE, D.PRUNE, D.SPLIT, D.CLONE, D.KEEP, D.CLONE]
    assert off.tolist() == [0, 1, 1, 1, 3, 5, 6]  # the exclusive scan of (1, 0, 0, 2, 2, 1, 2)
    rows_out, pruned, cloned, split = tot
    kept = int((a == D.KEEP).sum())
    assert (rows_out, pruned, cloned, split) == (8, 2, 2, 1) and rows_out == kept + 2 * cloned + 2 * split
    a0, off0, tot0 = _plan(rows, grow=False)  # growth off: clone and split become keep, prunes stay
    assert a0.tolist() == [D.KEEP, D.PRUNE, D.PRUNE, D.KEEP, D.KEEP, D.KEEP, D.KEEP] and off0.tolist() == [0, 1, 1, 1, 2, 3, 4] and tot0 == (5, 2, 0, 0)
    g = torch.Generator().manual_seed(0)
    G = 5000
    a, off, tot = D.plan(torch.rand(G, generator=g), torch.randint(0, 4, (G,), generator=g).int(), torch.zeros(G).int(), torch.randn(G, 3, generator=g) - 2.0,
                         torch.randn(G, generator=g) * 4, **THR)
    cnt = a.clamp(max=2)
    assert torch.equal(off, torch.cumsum(cnt, 0) - cnt) and tot[0] == int((a == D.KEEP).sum()) + 2 * tot[2] + 2 * tot[3] and min(tot[1:]) > 0


def test_reference_accumulate_and_apply_hand_case():
    nan = float("nan")
    g2d = torch.tensor([[[3.0, 4.0], [nan, nan], [1.0, 0.0]], [[0.0, 0.0], [6.0, 8.0], [nan, 5.0]]])
    radii = torch.tensor([[[2, 1], [0, 0], [0, 7]], [[1, 1], [4, 0], [0, 0]]], dtype=torch.int32)
    acc, n, rmax = D.accumulate(g2d, radii, 1.0, 0.5, torch.tensor([1.0, 0.0, 0.0]), torch.tensor([1, 0, 0]).int(), torch.tensor([9, 0, 0]).int())
    assert acc.tolist() == pytest.approx([1.0 + math.hypot(3.0, 2.0), math.hypot(6.0, 4.0), 1.0], rel=1e-14) and n.tolist() == [3, 1, 1] and rmax.tolist() == [9, 4, 7]
    # apply: a split along the x axis of an axis-aligned Gaussian, a clone, a prune and a keep
    p = dict(means=torch.tensor([[0.0, 0, 0], [1.0, 1, 1], [2.0, 2, 2], [3.0, 3, 3]]), scales=torch.log(torch.tensor([[2.0, 1, 1]] * 4)),
             rotations=torch.tensor([[0.0, 0, 0, 3.0]] * 4), opacities=torch.tensor([0.1, 0.2, 0.3, 0.4]))
    m = dict(means=(torch.ones(4, 3), 2 * torch.ones(4, 3)))
    noise = torch.zeros(4, 2, 3)
    noise[0, 0, 0], noise[0, 1, 0] = 1.0, -0.5
    action, offset = torch.tensor([D.SPLIT, D.CLONE, D.PRUNE, D.KEEP]), torch.tensor([0, 2, 4, 4])
    q, qm = D.apply(p, m, action, offset, 5, noise)
    # (the inputs are float32: log(2) carries that rounding)
    assert torch.allclose(q["means"], torch.tensor([[2.0, 0, 0], [-1.0, 0, 0], [1.0, 1, 1], [1.0, 1, 1], [3.0, 3, 3]], dtype=torch.float64), rtol=0, atol=1e-6)
    assert torch.equal(q["means"][2:], p["means"][[1, 1, 3]].double())
    assert torch.allclose(q["scales"].exp(), torch.tensor([[1.25, 0.625, 0.625]] * 2 + [[2.0, 1, 1]] * 3, dtype=torch.float64), rtol=1e-6)
    assert q["opacities"].tolist() == pytest.approx([0.1, 0.1, 0.2, 0.2, 0.4], rel=1e-7)
    assert qm["means"][0][:, 0].tolist() == [0, 0, 1, 0, 1] and qm["means"][1][:, 0].tolist() == [0, 0, 2, 0, 2]
    # a quarter turn about z carries the x axis onto y
    s = math.sqrt(0.5)
    R = D.rotation(torch.tensor([[0.0, 0.0, 5 * s, 5 * s]], dtype=torch.float64))[0]
    assert torch.allclose(R @ torch.tensor([1.0, 0, 0], dtype=torch.float64), torch.tensor([0.0, 1, 0], dtype=torch.float64), atol=1e-15)


def test_header_and_ctypes_declare_the_density_entry_points():
    from siu3r_amd import _lib

    text = open(os.path.join(ROOT, "include", "siu3r_hip.h")).read()
    for s in ("siu3r_density_accumulate", "siu3r_density_plan_ws", "siu3r_density_plan", "siu3r_density_apply"):
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert s in _lib.SIGNATURES and hasattr(_lib.lib(), s)
    assert re.search(r"#define\s+SIU3R_ABI_VERSION\s+13\b", text) and _lib.ABI_VERSION == 13
    assert int(_lib.lib().siu3r_density_plan_ws(100003)) >= (100003 + 255) // 256
