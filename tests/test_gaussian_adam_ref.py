"""CPU tests of the fused Adam's reference and host side: tests/dense_adam64.py against torch.optim.Adam, the visibility and head / tail
rules, optim.means_lr_schedule, refine_gaussians' keyword validation (which comes before any device work) and the compiled kernel's
resources."""
import math

import pytest
import torch

import dense_adam64 as A


def _carried(shape, steps, lr, lr_tail=None, head_period=0, kind="noise", seed=0):
    """`steps` carried steps of the float64 restatement on fresh state, with a new seeded gradient each step -> (params, grads)"""
    p, _, m, v, _ = A.make_field(kind, shape, seed)
    p, m, v = p.double(), m.double(), v.double()
    ps, gs = [p], []
    for t in range(1, steps + 1):
        g = A.make_field(kind, shape, seed + 100 * t)[1].double()
        p, m, v = A.step(p, g, m, v, t, lr, lr_tail, head_period)
        ps.append(p)
        gs.append(g)
    return ps, gs


def test_float64_restatement_is_torch_adam():
    shape, lr = (50, 3, 4), 2.5e-3
    ps, gs = _carried(shape, 5, lr)
    x = ps[0].clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr, eps=1e-15)
    worst = 0.0
    for t in range(5):
        x.grad = gs[t].clone()
        opt.step()
        worst = max(worst, float((x.detach() - ps[t + 1]).abs().max()))
    print(f"\nfloat64 restatement vs torch.optim.Adam over 5 carried steps: max |d| {worst:.3e}")
    assert worst <= 1e-12
    assert float((ps[5] - ps[0]).abs().max()) > 1e-3


def test_head_period_and_tail_rate_are_two_parameter_groups():
    shape, lr, tail = (40, 3, 4), 2.5e-3, 2.5e-3 * 0.05
    ps, gs = _carried(shape, 5, lr, tail, head_period=4, kind="render", seed=3)
    dc = ps[0][:, :, :1].clone().requires_grad_(True)
    rest = ps[0][:, :, 1:].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [dc], "lr": lr}, {"params": [rest], "lr": tail}], eps=1e-15)
    for t in range(5):
        dc.grad, rest.grad = gs[t][:, :, :1].clone(), gs[t][:, :, 1:].clone()
        opt.step()
    got = torch.cat((dc.detach(), rest.detach()), dim=-1)
    assert float((got - ps[5]).abs().max()) <= 1e-12
    # head_period 0: every element at lr; a period that does not divide the width restarts with every row
    p, g, m, v, t = A.make_field("noise", (9, 5), 1, "t2")
    a = A.step(p, g, m, v, t, 1e-2, 0.0, head_period=0)[0]
    assert bool((a != p.double()).flatten(1).any(1)[torch.arange(9) % 7 != 3].all())
    b = A.step(p, g, m, v, t, 1e-2, 0.0, head_period=2)[0]
    moved = b != p.double()
    assert not bool(moved[:, [1, 3]].any()) and bool(moved[:, [0, 2, 4]].any(1).all())


@pytest.mark.parametrize("form", ["radii", "mask"])
def test_skipped_rows_keep_their_bits(form):
    G = 30
    p, g, m, v, t = A.make_field("noise", (G, 3), 2, "t1000")
    radii, vis = A.make_radii(G, 3, seed=5)
    assert 0 < int(vis.sum()) < G
    g[~vis] = float("nan")
    visible = radii if form == "radii" else vis.to(torch.uint8)
    for dtype in (torch.float64, torch.float32):
        pn, mn, vn = A.step(p, g, m, v, t, 1e-3, visible=visible, dtype=dtype)
        for new, old in ((pn, p), (mn, m), (vn, v)):
            assert torch.equal(new[~vis], old[~vis].to(dtype)) and bool(torch.isfinite(new).all())
        dense = A.step(p, torch.nan_to_num(g), m, v, t, 1e-3, dtype=dtype)
        assert torch.equal(pn[vis], dense[0][vis]) and torch.equal(mn[vis], dense[1][vis]) and torch.equal(vn[vis], dense[2][vis])
        assert not torch.equal(mn[vis], m[vis].to(dtype))


def test_input_maker():
    for kind in ("noise", "render"):
        for state, t_want in (("fresh", 1), ("t2", 2), ("t1000", 1000)):
            p, g, m, v, t = A.make_field(kind, (700, 3, 4), 11, state)
            assert t == t_want and all(x.dtype == torch.float32 and x.shape == (700, 3, 4) for x in (p, g, m, v))
            zero_rows = ~g.flatten(1).any(1)
            assert bool(zero_rows[torch.arange(700) % 7 == 3].all()) and int(zero_rows.sum()) <= 110
            mag = g.abs().flatten(1).max(1).values[~zero_rows]
            assert float(mag.min()) < 1e-6 and float(mag.max()) > 0.1
            assert bool((v >= 0).all()) and (state != "fresh" or not bool(m.any() or v.any()))


def test_means_lr_schedule():
    from siu3r_amd.optim import means_lr_schedule

    s = means_lr_schedule(1.6e-4, 1.6e-6, 30)
    assert len(s) == 30 and s[0] == 1.6e-4 and s[-1] == 1.6e-6
    assert all(a > b for a, b in zip(s, s[1:]))
    ratios = [b / a for a, b in zip(s, s[1:])]
    assert max(ratios) / min(ratios) < 1 + 1e-9  # log-linear
    up = means_lr_schedule(1e-5, 1e-3, 7)
    assert up[0] == 1e-5 and up[-1] == 1e-3 and all(a < b for a, b in zip(up, up[1:]))
    assert means_lr_schedule(2e-4, 2e-4, 4) == [2e-4] * 4
    assert means_lr_schedule(3e-4, 1e-6, 1) == [3e-4] and means_lr_schedule(3e-4, 1e-6, 2) == [3e-4, 1e-6] and means_lr_schedule(3e-4, 1e-6, 0) == []
    for bad in ((0.0, 1e-3), (1e-3, 0.0), (-1e-3, 1e-3), (1e-3, math.inf), (math.nan, 1e-3)):
        with pytest.raises(ValueError, match="positive and finite"):
            means_lr_schedule(*bad, 10)


def test_refine_keywords_are_validated_before_device_work():
    """CPU tensors throughout: a call that got past the validation would fail in the render with another error"""
    from siu3r_amd.refine import refine_gaussians

    G = 8
    fields = (torch.zeros(G, 3), torch.ones(G, 3), torch.ones(G, 4), torch.full((G,), 0.5), torch.zeros(G, 3, 4))
    call = lambda **kw: refine_gaussians(*fields, torch.zeros(2, 3, 16, 16), torch.eye(4)[None].repeat(2, 1, 1), torch.eye(3), 0.5, 100.0, (0, 0, 0), iters=3, **kw)
    with pytest.raises(ValueError, match="optimizer"):
        call(optimizer="adamw")
    for kw in (dict(sparse=True), dict(means_lr_final=1e-6), dict(means_lr_extent_scale=True), dict(sh_rest_lr_scale=0.05)):
        with pytest.raises(ValueError, match=f'{next(iter(kw))}.*optimizer="hip"'):
            call(**kw)
        with pytest.raises(ValueError, match="optimizer"):
            call(optimizer="torch", **kw)
    for kw in (dict(means_lr_final=0.0), dict(means_lr_final=-1e-4), dict(means_lr_final=math.inf), dict(sh_rest_lr_scale=-0.1), dict(sh_rest_lr_scale=math.nan)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            call(optimizer="hip", **kw)


def test_cpu_tensors_are_refused():
    from siu3r_amd.optim import GaussianAdam

    with pytest.raises(RuntimeError, match="GPU"):
        GaussianAdam({"means": torch.zeros(4, 3, requires_grad=True)}, {"means": 1e-3})


def test_kernel_has_no_scratch_and_no_spills():
    from siu3r_amd import build as B

    B.build()
    res = B.kernel_resources("gaussian_adam.hip")
    names = sorted(res)
    assert len(names) == 2 and any("gaussian_adam_kernel" in n for n in names) and any("adam_visible_kernel" in n for n in names), names
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] == 0 and r["Occupancy [waves/SIMD]"] >= 4, (name, r)


def test_entry_point_validates_before_any_launch():
    """siu3r_gaussian_adam checks its arguments on the host and returns an error string: no GPU is needed to see it (the pointers below are
    never dereferenced)"""
    from siu3r_amd import _lib

    lib = _lib.lib()
    assert lib.siu3r_gaussian_adam_ws(1000) >= 1000 and lib.siu3r_gaussian_adam_ws(0) == 0

    def call(n=2, G=100, radii=None, mask=None, ws=64, **edit):
        table = (_lib.AdamField * 9)()
        for i in range(9):
            table[i] = _lib.AdamField(64, 64, 64, 64, 3, 0, 1e-3, 1e-3)
        for k, v in edit.items():
            setattr(table[1], k, v)
        _lib.check(lib.siu3r_gaussian_adam(table, n, G, 0.9, 0.999, 1e-15, 0.1, 0.001, radii, 2, 2, mask, ws, None))

    for match, kw in (("null pointer", dict(param=None)), ("null pointer", dict(grad=None)), ("null pointer", dict(exp_avg=None)),
                      ("null pointer", dict(exp_avg_sq=None)), ("width 0", dict(width=0)), ("width -3", dict(width=-3)), ("9 fields", dict(n=9)),
                      ("0 fields", dict(n=0)), ("learning rate", dict(lr=-1e-3)), ("learning rate", dict(lr_tail=-1e-3)),
                      ("learning rate", dict(lr=math.nan)), ("head_period", dict(head_period=-1)), ("at most one", dict(radii=64, mask=64)),
                      ("workspace", dict(radii=64, ws=None)), ("rows", dict(G=0))):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    with pytest.raises(RuntimeError, match="null field table"):
        _lib.check(lib.siu3r_gaussian_adam(None, 1, 100, 0.9, 0.999, 1e-15, 0.1, 0.001, None, 0, 0, None, None, None))
