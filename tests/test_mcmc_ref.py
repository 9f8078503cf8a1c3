"""MCMC densification without a GPU: the restatement's own properties (tests/dense_mcmc64.py: the relocation update, the integer sampler),
the schedule and the validation of mcmc.MCMCControl, the growth arithmetic, and every ValueError refine_gaussians raises for the control
before any device work."""
import math

import pytest
import torch

import dense_mcmc64 as M


# ---- the relocation update ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [-5.2, -1.0, 0.0, 2.5, 13.0])
def test_a_row_that_is_not_split_keeps_its_opacity_and_scale(a):
    """N = 1 (count = 0): o_new = o, the denominator is o, the scale factor 1.  In float64 the logit of the sigmoid comes back with the
    rounding of o and 1 - o (half a unit of 2^-52 each) divided by o (1 - o) = 1 / (2 + e^a + e^-a); in float32, the stored type, the
    row is unchanged to the bit."""
    s = [-3.0, -1.5, 0.25]
    na, ns = M.relocated_row(a, s, 0, 1e-9)
    assert abs(na - a) <= 2.0 ** -52 * (2.0 + math.exp(a) + math.exp(-a))
    assert ns == pytest.approx(s, rel=1e-15, abs=1e-15)
    assert float(torch.tensor(na).float()) == float(torch.tensor(a).float()) and torch.equal(torch.tensor(ns).float(), torch.tensor(s).float())


@pytest.mark.parametrize("o", [0.005, 0.5, 0.99, 1 - 1e-6])
def test_double_sum_equals_the_hockey_stick_form(o):
    worst = 0.0
    for N in range(1, M.N_MAX + 1):
        o_new = 1.0 - (1.0 - o) ** (1.0 / N)
        a, b = M.denominator(o_new, N), M.denominator_hockey_stick(o_new, N)
        worst = max(worst, abs(a - b) / abs(a))
        assert a > 0 and abs(a - b) <= 1e-12 * abs(a), (N, o, a, b)
    print(f"\no = {o}: double sum against hockey stick, largest relative difference over N <= {M.N_MAX}: {worst:.2e}")


def test_relocation_hand_case_and_count_clamp():
    """N = 2, o = 0.75: o_new = 1 - sqrt(0.25) = 0.5; the double sum is o_new + (o_new - o_new^2 / sqrt 2); a count above 50 is N = 51"""
    a = math.log(0.75 / 0.25)
    na, ns = M.relocated_row(a, [0.0, 1.0, 2.0], 1, 0.005)
    denom = 0.5 + (0.5 - 0.25 / math.sqrt(2.0))
    assert na == pytest.approx(0.0, abs=1e-14)
    assert ns == pytest.approx([v + math.log(0.75 / denom) for v in (0.0, 1.0, 2.0)], rel=1e-14)
    assert M.relocated_row(a, [0.0] * 3, 50, 0.005) == M.relocated_row(a, [0.0] * 3, 500, 0.005)
    assert M.relocated_row(a, [0.0] * 3, 49, 0.005) != M.relocated_row(a, [0.0] * 3, 50, 0.005)
    # the clamp works on the opacity only, after the denominator
    lo, s_lo = M.relocated_row(-4.0, [0.0] * 3, 50, 0.005)
    free, s_free = M.relocated_row(-4.0, [0.0] * 3, 50, 1e-12)
    assert lo == pytest.approx(math.log(0.005 / 0.995), rel=1e-14) and free < lo and s_lo == s_free


# ---- the integer sampler --------------------------------------------------------------------------------------------------------------
def test_sampler_frequencies_and_zero_weights():
    """8 weights, three of them zero (first, middle, last), 200,000 seeded draws: every frequency within 5 binomial standard deviations
    of w / total (five rows: a false alarm has a chance of about 5 x 5.7e-7, and the words are seeded), a zero weight is never drawn"""
    w = [0, 3_000_000, 16_777_216, 0, 1, 524_288, 9_999_999, 0]
    n = 200_000
    rbits = torch.randint(0, 1 << 32, (n,), generator=torch.Generator().manual_seed(2024), dtype=torch.int64).tolist()
    sampled, count = M.multinomial(w, rbits)
    total = sum(w)
    assert sum(count) == n and len(sampled) == n
    worst = 0.0
    for g, c in enumerate(count):
        p = w[g] / total
        if w[g] == 0:
            assert c == 0
            continue
        sd = math.sqrt(n * p * (1 - p))
        worst = max(worst, abs(c - n * p) / sd)
        assert abs(c - n * p) <= 5.0 * sd, (g, c, n * p, sd)
    print(f"\n{n} draws over {w}: counts {count}, largest deviation {worst:.2f} standard deviations")


def test_sampler_edges():
    w = [0, 0, 5, 0, 0, 7, 0]
    top = (1 << 32) - 1
    sampled, count = M.multinomial(w, [0, top, 1 << 31])
    # t = 0 -> the first row with a weight; t = (top * 12) >> 32 = 11 -> the last one; t = 6 -> cum 5 < 7 <= 12
    assert sampled == [2, 5, 5] and count == [0, 0, 1, 0, 0, 2, 0]
    assert M.multinomial([0, 0, 0], [0, top]) == ([0, 0], [2, 0, 0])  # no weight anywhere: row 0
    # exact where a float product is not: a total of 2^53 + 1 and the largest word
    big = [1 << 52, 1, 1 << 52]
    t = (top * sum(big)) >> 32
    assert M.multinomial(big, [top])[0] == [2] and t > (1 << 52)
    assert M.dead_list(torch.tensor([True, False, False, True, True])) == [0, 3, 4]
    assert M.scan(torch.tensor([1 << 24] * 3)).tolist() == [1 << 24, 2 << 24, 3 << 24]


def test_weights_restatement():
    thr = M.f32(math.log(0.005 / 0.995))
    a = torch.tensor([thr, float(torch.nextafter(torch.tensor(thr), torch.tensor(0.0))), float(torch.nextafter(torch.tensor(thr), torch.tensor(-10.0))),
                      0.0, 30.0, -30.0])
    w, dead = M.weights(a, thr, relocate=False)
    assert dead.tolist() == [True, False, True, False, False, True]  # <=: a row exactly at the threshold is dead
    assert w.tolist()[3:] == [1 << 23, 1 << 24, 0] and w[0] == round(M.W_ONE / (1 + math.exp(-thr)))
    w2, _ = M.weights(a, thr, relocate=True)
    assert w2.tolist() == [0, int(w[1]), 0, 1 << 23, 1 << 24, 0]


# ---- the control ----------------------------------------------------------------------------------------------------------------------
def test_schedule():
    from siu3r_amd.mcmc import MCMCControl as C

    c = lambda **kw: C(cap_max=10, **kw)
    assert c().events(200) == [100]
    assert c().events(99) == [] and c().events(100) == []
    assert c(start=10, every=10).events(30) == [10, 20]  # stop = None -> iters - every
    assert c(start=10, every=10, stop=10).events(100) == [10]  # stop is inclusive
    assert c(start=10, every=10, stop=9).events(100) == []
    assert c(start=10, every=10, stop=1000).events(35) == [10, 20, 30]  # never past the run
    assert c(start=0, every=10, stop=20).events(100) == [10, 20]  # never iteration 0
    assert c(start=10, every=7, stop=30).events(100) == [10, 17, 24]
    with pytest.raises(ValueError):
        c(every=0).events(100)


def test_defaults_are_gsplats():
    from siu3r_amd.mcmc import GATE_OPACITY, MCMCControl

    c = MCMCControl(cap_max=1000)
    assert (c.grow_factor, c.min_opacity, c.noise_lr, c.opacity_reg, c.scale_reg, c.start, c.every, c.stop, c.seed) == (1.05, 0.005, 5e5, 0.01, 0.01, 100, 100, None, 0)
    assert GATE_OPACITY == M.GATE_OPACITY == 0.005
    assert c.logit_min_opacity == M.f32(math.log(0.005 / 0.995))
    with pytest.raises(TypeError):
        MCMCControl()  # cap_max is required


def test_growth_arithmetic():
    from siu3r_amd.mcmc import MCMCControl as C

    assert C(cap_max=1000).n_new(1000) == 0  # G = cap_max
    assert C(cap_max=1000).n_new(999) == 1  # cap_max - 1: int(1.05 * 999) = 1048, capped
    assert C(cap_max=10**9).n_new(19) == 0 and int(1.05 * 19) == 19  # int(1.05 G) == G: nothing to add
    assert C(cap_max=10**9).n_new(20) == 1 and C(cap_max=10**9).n_new(4000) == 200
    assert C(cap_max=4100).n_new(4000) == 100 and C(cap_max=3000).n_new(4000) == 0  # (a cap below G never removes rows)
    assert C(cap_max=10**9, grow_factor=1.0).n_new(4000) == 0
    assert C(cap_max=10**9, grow_factor=2.0).n_new(7) == 7


BAD = [dict(cap_max=0), dict(cap_max=-5), dict(cap_max=10.5), dict(cap_max=True), dict(grow_factor=0.9), dict(grow_factor=float("nan")),
       dict(grow_factor=float("inf")), dict(min_opacity=0.0), dict(min_opacity=1.0), dict(min_opacity=-0.1), dict(min_opacity=float("nan")),
       dict(noise_lr=-1.0), dict(noise_lr=float("inf")), dict(opacity_reg=-0.01), dict(opacity_reg=float("nan")), dict(scale_reg=-0.01),
       dict(scale_reg=float("inf")), dict(every=0), dict(every=-3), dict(start=-1), dict(stop=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_validation(bad):
    from siu3r_amd.mcmc import MCMCControl

    with pytest.raises(ValueError, match=next(iter(bad))):
        MCMCControl(**{"cap_max": 100, **bad}).validate()
    MCMCControl(cap_max=100).validate(100)
    with pytest.raises(ValueError, match="cap_max"):
        MCMCControl(cap_max=100).validate(101)


def _cpu_call(control, G=8, **kw):
    """refine_gaussians on CPU tensors: a control that is rejected must be rejected before anything touches the device"""
    from siu3r_amd.refine import refine_gaussians

    z = torch.zeros
    return refine_gaussians(z(G, 3), torch.ones(G, 3), torch.ones(G, 4), torch.full((G,), 0.5), z(G, 3, 1), z(2, 3, 16, 16), torch.eye(4)[None].repeat(2, 1, 1),
                            torch.eye(3), 0.5, 100.0, (0.0, 0.0, 0.0), iters=5, density=control, **kw)


@pytest.mark.parametrize("bad", [dict(cap_max=7), dict(every=0), dict(noise_lr=float("nan")), dict(opacity_reg=-1.0), dict(scale_reg=float("inf")),
                                 dict(min_opacity=2.0), dict(grow_factor=-1.05)], ids=lambda d: next(iter(d)))
def test_refine_rejects_a_bad_control_before_any_device_work(bad):
    from siu3r_amd.mcmc import MCMCControl

    with pytest.raises(ValueError, match=next(iter(bad))):
        _cpu_call(MCMCControl(**{"cap_max": 8, **bad}))
    with pytest.raises(ValueError, match=next(iter(bad))):
        _cpu_call(MCMCControl(**{"cap_max": 8, **bad}), optimizer="hip", sparse=True)


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    """no CPU fallback: the kernels' wrappers raise on host tensors"""
    from siu3r_amd import mcmc

    a, s = torch.zeros(4), torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        mcmc.weights(a, -5.0, True)
    with pytest.raises(RuntimeError):
        mcmc.inject_noise(s.clone(), s, torch.ones(4, 4), a, 1.0, s)
    with pytest.raises(RuntimeError):
        mcmc.regularize(a, s, 0.01, 0.01)
    with pytest.raises(RuntimeError):
        mcmc.relocate(dict(means=s, scales=s, rotations=torch.ones(4, 4), opacities=a, harmonics=torch.zeros(4, 3, 1)), {}, mcmc.MCMCControl(cap_max=4))
