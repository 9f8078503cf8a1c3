"""CPU tests of the float64 restatement of the depth smoothness (tests/dense_smooth64.py), the reference of tests/test_depth_smooth_gpu.py:
its closed-form gradients (the formulas csrc/depth_smooth.hip implements) against autograd through the same value, autograd against central
differences, the active-term rule of order 1 against an independent torch.diff formulation of the training objective's two-step mask, and
the shapes without a term position."""
import math

import pytest
import torch

import dense_smooth64 as S

ORDERS, SPACES = (1, 2), ("render", "expected")


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_closed_form_matches_autograd(kind, order, space):
    for segments in (True, False):
        D, O, seg = S.make_inputs(kind, 3, 37, 67, seed=7, segments=segments)
        a = S.loss_and_grad(D, O, seg, order, space, route="autograd")
        c = S.loss_and_grad(D, O, seg, order, space, route="closed")
        assert a["loss"] == c["loss"] and a["loss"] > 0 and int(a["active"].sum()) > 100
        for k in ("g_depth", "g_opacity"):
            gmax = float(a[k].abs().max())
            assert gmax > 0 or (space == "render" and k == "g_opacity")
            assert float((a[k] - c[k]).abs().max()) <= 1e-12 * gmax, (kind, order, space, k)
        dead = ~S.usable_mask(D.double(), O.double(), space, 0.5) | ((seg < 0) if seg is not None else torch.zeros_like(D, dtype=torch.bool))
        assert not bool(c["g_depth"][dead].any()) and not bool(c["g_opacity"][dead].any())


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("order", ORDERS)
def test_autograd_matches_central_differences(order, space):
    D, O, seg = S.make_inputs("noise", 2, 9, 11, seed=3, segments=True)
    D, O = D.double(), O.double()
    (tx, ty), _, _ = S.term_values(D, O, seg, order, space)
    assert all(float(t[act].abs().min()) > 1e-6 for t, act in (tx, ty)), "a term within 1e-6 of zero: the difference quotient would straddle the kink"
    ref = S.loss_and_grad(D, O, seg, order, space, route="autograd")
    f = lambda d, o: float(S.terms(d, o, seg, order, space)[0])
    h = 1e-7
    g = torch.Generator().manual_seed(1)
    for idx in torch.randperm(D.numel(), generator=g)[:40].tolist():
        for which, key in ((0, "g_depth"), (1, "g_opacity")):
            # a step must not carry the pixel across the usability threshold
            if space == "expected" and abs(float(O.view(-1)[idx]) - 0.5) < 1e-5:
                continue
            lo, hi = [D.clone(), O.clone()], [D.clone(), O.clone()]
            lo[which].view(-1)[idx] -= h
            hi[which].view(-1)[idx] += h
            fd = (f(*hi) - f(*lo)) / (2 * h)
            assert abs(fd - float(ref[key].view(-1)[idx])) <= 1e-6 * max(1.0, float(ref[key].abs().max())), (order, space, key, idx, fd)


def test_order_one_rule_is_the_two_step_mask():
    """equal ids, then the right / lower pixel not void -- formulated with torch.diff on random maps with void pixels; exact"""
    g = torch.Generator().manual_seed(5)
    for _ in range(4):
        seg = torch.randint(-1, 3, (3, 23, 31), generator=g, dtype=torch.int32)
        D = torch.rand(3, 23, 31, generator=g) + 0.5
        (tx, ty), x, _ = S.term_values(D.double(), torch.ones_like(D).double(), seg, 1, "render")
        same_x = seg.diff(dim=-1) == 0
        same_x &= seg[:, :, 1:] != -1
        same_y = seg.diff(dim=-2) == 0
        same_y &= seg[:, 1:, :] != -1
        assert torch.equal(tx[1], same_x) and torch.equal(ty[1], same_y)
        want = (D.double().diff(dim=-1) * same_x).abs().mean() + (D.double().diff(dim=-2) * same_y).abs().mean()
        got = S.loss_and_grad(D, None, seg, 1, "render")
        assert abs(got["loss"] - float(want)) <= 1e-15 * float(want)
        assert torch.equal(got["active"], torch.stack([same_x.flatten(1).sum(1), same_y.flatten(1).sum(1)], dim=1))


@pytest.mark.parametrize("space", SPACES)
def test_axes_without_a_position_give_zero(space):
    one = lambda *s: (torch.full(s, 2.0), torch.full(s, 1.0))
    for order, shape, positions in ((1, (1, 1, 1), (0, 0)), (2, (1, 2, 2), (0, 0)), (2, (1, 1, 2), (0, 0)), (1, (1, 1, 2), (1, 0)), (1, (1, 2, 1), (0, 1)),
                                    (2, (1, 3, 3), (3, 3))):
        D, O = one(*shape)
        D.view(-1)[0] = 3.0
        for route in ("autograd", "closed"):
            r = S.loss_and_grad(D, O, None, order, space, route=route)
            assert math.isfinite(r["loss"]) and bool(torch.isfinite(r["per_view"]).all()) and bool(torch.isfinite(r["g_depth"]).all())
            assert r["active"].tolist() == [list(positions)], (order, shape, r["active"])
            assert (r["loss"] == 0.0) == (sum(positions) == 0)
            assert (r["parts"][0] == 0.0) == (positions[0] == 0) and (r["parts"][1] == 0.0) == (positions[1] == 0)
