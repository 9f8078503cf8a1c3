"""csrc/mcmc.hip on the GPU against tests/dense_mcmc64.py (float64 and Python integers, written from the rules): weights, scan, draws, the
dead list, the relocation update, the row copy, noise and regulariser.

Integers (draws, counts, the dead list, copied rows) are compared bit for bit; the weights to one unit; the relocation update (fp64 in
the kernel) to one float32 ulp of the float64 restatement.  Float32 bar (noise, regulariser), the one of tests/test_density_gpu.py: the
float64 restatement is evaluated on the SAME float32 inputs upcast; the same restatement in float32 runs on the CPU; the kernel's error
against float64 may be at most 2 x that float32 error (another operation order), with a floor of 1e-6."""
import math

import pytest
import torch

import dense_mcmc64 as M

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 257, 10007]
THR = M.f32(math.log(0.005 / 0.995))  # logit(min_opacity) as the kernel compares it
TOP = (1 << 32) - 1


def _logits(G, seed):
    """logit opacities around and far from the threshold: runs of dead rows at the start, in the middle and at the end (G >= 63), rows
    exactly at the threshold and one float32 step either side of it"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(G, generator=g) * 3
    if G >= 63:
        a[:9] = -9.0 - torch.rand(9, generator=g)
        a[G // 2:G // 2 + 17] = -7.0
        a[-5:] = -20.0
        t = torch.tensor(THR)
        a[11], a[12], a[13] = t, torch.nextafter(t, torch.tensor(0.0)), torch.nextafter(t, torch.tensor(-10.0))
        a[20], a[21] = 25.0, -25.0
    return a


def _draws(n, seed):
    r = torch.randint(0, 1 << 32, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    r[0] = 0
    r[-1] = TOP
    if n > 2:
        r[1] = TOP
        r[2] = 1 << 31
    return r


# ---- (a) weights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("relocate", [True, False])
def test_weights(G, relocate):
    from siu3r_amd import mcmc

    a = _logits(G, seed=G)
    ref_w, ref_dead = M.weights(a, THR, relocate)
    outs = [mcmc.weights(a.cuda(), THR, relocate) for _ in range(2)]
    w, dead = outs[0]
    assert w.dtype == torch.int32 and dead.dtype == torch.bool
    assert torch.equal(dead.cpu(), ref_dead), "the dead mask"
    off = (w.cpu().long() - ref_w).abs()
    print(f"\nweights G={G} relocate={relocate}: {int(ref_dead.sum())} dead, largest difference to the float64 restatement {int(off.max())} unit(s)")
    assert int(off.max()) <= 1
    assert int(w.min()) >= 0 and int(w.max()) <= M.W_ONE
    if relocate:
        assert not bool(w[dead].any())
    elif G >= 63:
        assert bool(w.cpu()[ref_dead].any())  # growth draws from every row
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- (b), (c) scan, draws, dead list --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("n_kind", ["1", "300", "3G"])
def test_draws_are_the_integer_restatement(G, n_kind):
    from siu3r_amd import mcmc

    n = {"1": 1, "300": 300, "3G": 3 * G}[n_kind]
    a = _logits(G, seed=G + 1)
    w, dead = mcmc.weights(a.cuda(), THR, True)  # the kernel's own weights: zero runs at the start, in the middle, at the end
    rbits = _draws(n, seed=G + n)
    outs = []
    for _ in range(2):
        cum, dead_idx, n_dead = mcmc.scan(w, dead)
        sampled, count = mcmc.sample(cum, rbits.cuda())
        outs.append((cum, dead_idx[:int(n_dead)], n_dead, sampled, count))
    cum, dead_idx, n_dead, sampled, count = outs[0]
    ref_sampled, ref_count = M.multinomial(w.tolist(), rbits.tolist())
    ref_dead = M.dead_list(dead.cpu())
    assert torch.equal(cum.cpu(), M.scan(w.cpu())), "the scan"
    assert int(n_dead) == len(ref_dead) and dead_idx.tolist() == ref_dead, "the dead list"
    assert sampled.dtype == torch.int32 and count.dtype == torch.int32
    assert sampled.tolist() == ref_sampled, "the draws"
    assert count.tolist() == ref_count and int(count.sum()) == n, "the counts"
    assert not bool(count[dead].any()), "a dead row was drawn"
    live = torch.nonzero(w).flatten()
    if n > 1:
        assert int(sampled[0]) == int(live[0])  # word 0 -> the first row with a weight, behind the dead run at the start
    if G >= 63:
        assert int(live[0]) >= 9 and int(live[-1]) <= G - 6 and int(sampled.max()) <= G - 6
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)


def test_no_weight_anywhere_draws_row_zero():
    from siu3r_amd import mcmc

    G = 300
    w, dead = mcmc.weights(torch.full((G,), -12.0).cuda(), THR, True)
    cum, dead_idx, n_dead = mcmc.scan(w, dead)
    sampled, count = mcmc.sample(cum, _draws(50, 1).cuda())
    assert int(n_dead) == G and dead_idx.tolist() == list(range(G)) and int(cum[-1]) == 0
    assert sampled.tolist() == [0] * 50 and count.tolist() == [50] + [0] * (G - 1)
    assert (sampled.tolist(), count.tolist()) == M.multinomial([0] * G, _draws(50, 1).tolist())


@pytest.mark.parametrize("G", [256 * 1024, 256 * 1024 + 1, 300001])
def test_scan_across_the_second_level_carry(G):
    """workgroups of 256 rows, their sums scanned 1024 at a time: 262,145 rows are the first count at which the second level takes a
    second chunk and its carry.  Full 24-bit weights: the total passes 2^32"""
    from siu3r_amd import mcmc

    g = torch.Generator().manual_seed(G)
    w = torch.randint(0, M.W_ONE + 1, (G,), generator=g, dtype=torch.int32)
    w[1000:3000] = 0
    dead = torch.rand(G, generator=g) < 0.3
    outs = [mcmc.scan(w.cuda(), dead.cuda()) for _ in range(2)]
    cum, dead_idx, n_dead = outs[0]
    ref = M.scan(w)
    assert int(ref[-1]) > (1 << 40)
    assert torch.equal(cum.cpu(), ref)
    want = torch.nonzero(dead).flatten()
    assert int(n_dead) == want.numel() and torch.equal(dead_idx[:int(n_dead)].cpu().long(), want)
    only, none_idx, none_n = mcmc.scan(w.cuda())
    assert torch.equal(only, cum) and none_idx is None and none_n is None
    # draws at both ends of every chunk boundary's neighbourhood are found by the bisection
    rbits = _draws(300, G)
    sampled, count = mcmc.sample(cum, rbits.cuda())
    t = torch.tensor([(int(r) * int(ref[-1])) >> 32 for r in rbits.tolist()])
    assert torch.equal(sampled.cpu().long(), torch.searchsorted(ref, t, right=True))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1][:int(n_dead)], outs[1][1][:int(n_dead)])


# ---- (d) relocation update ------------------------------------------------------------------------------------------------------------
def test_relocation_update_within_one_float32_ulp():
    from siu3r_amd import mcmc

    counts = [0, 1, 2, 7, 50, 51, 500]
    per = 90
    G = per * len(counts)
    g = torch.Generator().manual_seed(5)
    lo, hi = math.log(0.0051 / (1 - 0.0051)), math.log((1 - 1e-6) / 1e-6)
    a = (lo + (hi - lo) * torch.linspace(0, 1, per, dtype=torch.float64)).float().repeat(len(counts))  # o from 0.0051 to 1 - 1e-6 for every count
    s = torch.log(0.01 + 0.3 * torch.rand(G, 3, generator=g))
    count = torch.tensor(counts, dtype=torch.int32).repeat_interleave(per)
    perm = torch.randperm(G, generator=g)
    a, s, count = a[perm].contiguous(), s[perm].contiguous(), count[perm].contiguous()
    ref_a, ref_s = M.relocation(a, s, count, 0.005)
    outs = []
    for _ in range(2):
        xa, xs = a.cuda(), s.cuda()
        mcmc.relocation_update(xs, xa, count.cuda(), 0.005)
        outs.append((xa.cpu(), xs.cpu()))
    xa, xs = outs[0]
    still = count == 0
    assert torch.equal(xa[still], a[still]) and torch.equal(xs[still], s[still]), "rows that were not drawn keep their bits"
    assert not bool((xa[~still] == a[~still]).any()) and not bool((xs[~still] == s[~still]).any())
    inf = torch.tensor(float("inf"))
    for name, x, ref in (("logit opacity", xa, ref_a), ("log-scales", xs, ref_s)):
        r32 = ref.float()
        ok = (x >= torch.nextafter(r32, -inf)) & (x <= torch.nextafter(r32, inf))
        exact = float((x == r32).float().mean())
        print(f"\nrelocation {name}: {exact:.4f} of the outputs are the float32-rounded float64 restatement, largest difference "
              f"{float((x.double() - ref).abs().max()):.3e}")
        assert bool(ok.all()), name
    # a count above 50 is the update of 50; no opacity falls below the floor
    big = torch.full((4,), 0.3).logit()
    outs2 = []
    for c in (50, 51, 500):
        xa2, xs2 = big.cuda(), torch.zeros(4, 3).cuda()
        mcmc.relocation_update(xs2, xa2, torch.full((4,), c, dtype=torch.int32).cuda(), 0.005)
        outs2.append((xa2, xs2))
    assert all(torch.equal(outs2[0][i], outs2[1][i]) and torch.equal(outs2[0][i], outs2[2][i]) for i in range(2))
    assert float(xa.min()) >= THR
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- (e) row copy ---------------------------------------------------------------------------------------------------------------------
WIDTHS = {"1": (), "3": (3,), "4": (4,), "3x1": (3, 1), "3x4": (3, 4), "3x16": (3, 16)}


@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("width", list(WIDTHS))
def test_copy_rows_is_bit_exact(G, width):
    from siu3r_amd import mcmc

    g = torch.Generator().manual_seed(G + len(width))
    tail = WIDTHS[width]
    for n in (1, 300, 3 * G):
        for given in (True, False):
            if given:  # destinations inside the field: n distinct rows, the sources drawn (with repeats) from the others
                n_ = min(n, G // 2)
                if n_ == 0:
                    continue
                perm = torch.randperm(G, generator=g)
                dst = perm[:n_].to(torch.int32)
                src = perm[n_:][torch.randint(0, G - n_, (n_,), generator=g)].to(torch.int32)
                rows, G0 = G, 0
            else:  # growth: n new rows behind the first G
                n_, dst, rows, G0 = n, None, G + n, G
                src = torch.randint(0, G, (n_,), generator=g, dtype=torch.int32)
            field = torch.randn(rows, *tail, generator=g)
            for with_moments in (True, False):
                moments = (torch.randn(rows, *tail, generator=g), torch.rand(rows, *tail, generator=g) + 0.1) if with_moments else None
                ref_f, ref_m = M.copy_rows(field, moments, src, dst, G0)
                outs = []
                for _ in range(2):
                    f = field.cuda()
                    m = tuple(x.cuda() for x in moments) if with_moments else None
                    mcmc.copy_rows(f, m, src.cuda(), None if dst is None else dst.cuda(), G0)
                    outs.append((f, m))
                f, m = outs[0]
                what = f"G={G} width={width} n={n_} dst={'given' if given else 'NULL'} moments={with_moments}"
                assert torch.equal(f.cpu(), ref_f), what
                touched = torch.zeros(rows, dtype=torch.bool)
                touched[src.long()] = True
                touched[(G0 + torch.arange(n_)) if dst is None else dst.long()] = True
                if with_moments:
                    for j in range(2):
                        assert torch.equal(m[j].cpu(), ref_m[j]), what
                        assert torch.equal(m[j].cpu()[~touched], moments[j][~touched]) and not bool(m[j].cpu()[touched].any()), what
                        assert torch.equal(outs[1][1][j], m[j])
                assert torch.equal(f.cpu()[src.long()], field[src.long()]), what  # the sources keep their bits
                assert torch.equal(outs[1][0], f)


def test_copy_rows_rejects_what_it_cannot_do():
    from siu3r_amd import _lib, mcmc

    f = torch.zeros(10, 3).cuda()
    src = torch.zeros(4, dtype=torch.int32).cuda()
    with pytest.raises(ValueError):
        mcmc.copy_rows(f, None, src, None, G0=7)  # rows 7 .. 11 of 10
    with pytest.raises(ValueError):
        mcmc.copy_rows(f, (f.clone(), f.clone()[:5]), src, None, G0=0)
    lib = _lib.lib()
    assert lib.siu3r_mcmc_copy_rows(f.data_ptr(), None, None, 3, 10, src.data_ptr(), None, 0, -1, None) != 0 and b"negative" in lib.siu3r_last_error()
    assert lib.siu3r_mcmc_copy_rows(None, None, None, 3, 10, src.data_ptr(), None, 0, 4, None) != 0 and b"null" in lib.siu3r_last_error()
    assert lib.siu3r_mcmc_copy_rows(f.data_ptr(), f.data_ptr(), None, 3, 10, src.data_ptr(), None, 0, 4, None) != 0
    # an index outside the field is skipped, not followed
    bad = torch.tensor([0, 99, -3, 1], dtype=torch.int32).cuda()
    dst = torch.tensor([5, 6, 7, 1000], dtype=torch.int32).cuda()
    x = torch.arange(30, dtype=torch.float32).view(10, 3).cuda()
    keep = x.clone()
    mcmc.copy_rows(x, None, bad, dst)
    keep[5] = keep[0]
    assert torch.equal(x, keep)


# ---- (f) noise ------------------------------------------------------------------------------------------------------------------------
def _bar(e_hip, e_32):
    return e_hip <= max(2.0 * e_32, 1e-6)


@pytest.mark.parametrize("G", SIZES)
def test_noise_against_float64(G):
    from siu3r_amd import mcmc

    g = torch.Generator().manual_seed(G + 7)
    means = torch.randn(G, 3, generator=g) * 2
    s = torch.log(0.01 + 0.3 * torch.rand(G, 3, generator=g))
    q = torch.randn(G, 4, generator=g) * (0.2 + 3 * torch.rand(G, 1, generator=g))  # not normalised
    # opacities on both sides of the gate at 0.005: far below (gate ~ 1), around it, far above (gate ~ 0)
    o = torch.tensor([1e-4, 1e-3, 0.004, 0.005, 0.006, 0.01, 0.03, 0.1, 0.5, 0.99], dtype=torch.float64)[torch.randint(0, 10, (G,), generator=g)]
    a = torch.logit(o).float()
    z = torch.randn(G, 3, generator=g)
    scaler = M.f32(5e5 * 1.6e-4)
    ref, delta = M.noise(means, s, q, a, z, scaler, M.f32(M.GATE_OPACITY))
    c32, _ = M.noise(means, s, q, a, z, scaler, M.f32(M.GATE_OPACITY), dtype=torch.float32)
    outs = []
    for _ in range(2):
        x = means.cuda()
        mcmc.inject_noise(x, s.cuda(), q.cuda(), a.cuda(), scaler, z.cuda())
        outs.append(x.cpu())
    x = outs[0]
    unit = (means.double().abs().amax(-1) + delta.abs().amax(-1))[:, None]  # a row's error in units of its mean and its displacement
    err = lambda y: float(((y.double() - ref).abs() / unit).max())
    e_hip, e_32 = err(x), err(c32)
    opaque, clear = o >= 0.5, o <= 1e-3  # gate <= exp(-49) against gate >= 0.98
    print(f"\nnoise G={G}: float32 restatement (CPU) {e_32:.2e}, hip {e_hip:.2e}; {int(clear.sum())} rows with gate ~ 1 moved by up to "
          f"{float(delta[clear].abs().max()) if bool(clear.any()) else 0.0:.3e}, {int(opaque.sum())} rows with gate ~ 0")
    assert bool(torch.isfinite(x).all())
    assert _bar(e_hip, e_32)
    assert torch.equal(x[opaque], means[opaque]), "an opaque Gaussian moved"
    if bool(clear.any()):
        assert bool((x[clear] != means[clear]).any(-1).all()), "a transparent Gaussian stayed"
    assert torch.equal(outs[0], outs[1])


# ---- (g) regulariser ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("frozen", ["none", "scales", "both"])
def test_regularize_against_float64(G, frozen):
    from siu3r_amd import mcmc

    g = torch.Generator().manual_seed(G + 11)
    a = torch.randn(G, generator=g) * 3
    s = torch.log(0.01 + 0.3 * torch.rand(G, 3, generator=g))
    ga0 = None if frozen == "both" else torch.randn(G, generator=g) * 1e-5
    gs0 = None if frozen != "none" else torch.randn(G, 3, generator=g) * 1e-5
    lam_o, lam_s = M.f32(0.01), M.f32(0.02)
    ref = M.regularize(a, s, lam_o, lam_s, ga0, gs0)
    c32 = M.regularize(a, s, lam_o, lam_s, ga0, gs0, dtype=torch.float32)
    outs = []
    for _ in range(2):
        ga = None if ga0 is None else ga0.cuda()
        gs = None if gs0 is None else gs0.cuda()
        outs.append((ga, gs, mcmc.regularize(a.cuda(), s.cuda(), lam_o, lam_s, ga, gs)))
    for i, (name, before) in enumerate((("opacity gradient", ga0), ("scale gradient", gs0))):
        if before is None:
            assert ref[i] is None
            continue
        unit = before.double().abs() + (ref[i] - before.double()).abs()  # an element's error in units of what was added to what
        err = lambda y: float(((y.double().cpu() - ref[i]).abs() / unit).max())
        e_hip, e_32 = err(outs[0][i]), err(c32[i])
        print(f"\nregularize G={G} ({frozen} frozen) {name}: float32 restatement (CPU) {e_32:.2e}, hip {e_hip:.2e}")
        assert _bar(e_hip, e_32) and not torch.equal(outs[0][i].cpu(), before)
    rel = lambda y: float(((y.double().cpu() - ref[2]).abs() / ref[2].abs()).max())
    e_hip, e_32 = rel(outs[0][2]), rel(c32[2])
    print(f"\nregularize G={G} ({frozen} frozen) values {outs[0][2].tolist()}: float32 restatement (CPU) {e_32:.2e}, hip {e_hip:.2e}")
    assert _bar(e_hip, e_32)
    for x, y in zip(outs[0], outs[1]):
        assert (x is None and y is None) or torch.equal(x, y)


# ---- relocate and grow, the two halves of an event -------------------------------------------------------------------------------------
def _fields(G, seed, dead_rows=()):
    g = torch.Generator().manual_seed(seed)
    p = dict(means=torch.randn(G, 3, generator=g), scales=torch.log(0.01 + 0.3 * torch.rand(G, 3, generator=g)), rotations=torch.randn(G, 4, generator=g),
             opacities=torch.logit(0.05 + 0.9 * torch.rand(G, generator=g)), harmonics=torch.randn(G, 3, 4, generator=g))
    p["opacities"][list(dead_rows)] = -9.0
    m = {k: (torch.randn(p[k].shape, generator=g), torch.rand(p[k].shape, generator=g) + 0.1) for k in ("means", "scales", "opacities", "harmonics")}
    return p, m


def _cuda(d):
    return {k: (tuple(x.cuda() for x in v) if isinstance(v, tuple) else v.cuda()) for k, v in d.items()}


def test_relocate_composes_the_kernels():
    from siu3r_amd import mcmc

    G = 2000
    dead_rows = list(range(0, G, 13))
    p, m = _fields(G, 3, dead_rows)
    control = mcmc.MCMCControl(cap_max=G, seed=4)
    rbits = _draws(len(dead_rows) + 10, 8)  # (more words than needed: the first n_dead are used)
    gp, gm = _cuda(p), _cuda(m)
    info = mcmc.relocate(gp, gm, control, rbits=rbits.cuda())
    assert info == dict(rows_in=G, rows_out=G, relocated=len(dead_rows))
    w, _ = mcmc.weights(p["opacities"].cuda(), THR, True)
    sampled, count = M.multinomial(w.tolist(), rbits[:len(dead_rows)].tolist())
    count = torch.tensor(count, dtype=torch.int32)
    ua, us = p["opacities"].cuda(), p["scales"].cuda()
    mcmc.relocation_update(us, ua, count.cuda(), 0.005)
    want = dict(p, opacities=ua.cpu(), scales=us.cpu())
    for k in want:
        ref_f, ref_m = M.copy_rows(want[k], m.get(k), sampled, dead_rows)
        assert torch.equal(gp[k].cpu(), ref_f), k
        if k in m:
            assert torch.equal(gm[k][0].cpu(), ref_m[0]) and torch.equal(gm[k][1].cpu(), ref_m[1]), k
    assert not bool((gp["opacities"] <= THR).any())
    # seeded words: two calls agree, another seed differs; nothing dead: nothing happens; everything dead: an error
    runs = []
    for seed in (4, 4, 5):
        q = _cuda(p)
        mcmc.relocate(q, {}, mcmc.MCMCControl(cap_max=G, seed=seed))
        runs.append(q["means"])
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    again = {k: v.clone() for k, v in gp.items()}
    assert mcmc.relocate(gp, gm, control)["relocated"] == 0 and all(torch.equal(gp[k], again[k]) for k in gp)
    allp, _ = _fields(50, 1, range(50))
    with pytest.raises(RuntimeError, match="dead"):
        mcmc.relocate(_cuda(allp), {}, mcmc.MCMCControl(cap_max=50))


def test_grow_adds_corrected_copies_with_zero_moments():
    from siu3r_amd import mcmc

    G = 2000
    p, m = _fields(G, 6)
    control = mcmc.MCMCControl(cap_max=2060)
    n = control.n_new(G)
    assert n == 60
    rbits = _draws(n, 9)
    gp, gm = _cuda(p), _cuda(m)
    new_p, new_m, info = mcmc.grow(gp, gm, control, rbits=rbits.cuda())
    assert info == dict(rows_in=G, rows_out=G + n, added=n)
    w, _ = mcmc.weights(p["opacities"].cuda(), THR, False)
    sampled, count = M.multinomial(w.tolist(), rbits.tolist())
    src = torch.tensor(sampled)
    drawn = torch.tensor(count) > 0
    for k in p:
        x = new_p[k].cpu()
        assert x.shape == (G + n, *p[k].shape[1:])
        assert torch.equal(x[G:], x[src]), f"{k}: a new row is a copy of its source"
        assert torch.equal(x[:G][~drawn], p[k][~drawn]), f"{k}: rows that were not drawn"
        if k in ("scales", "opacities"):
            assert not bool((x[:G][drawn] == p[k][drawn]).any()), f"{k}: the drawn rows are corrected"
        else:
            assert torch.equal(x[:G], p[k])
        if k in m:
            for j in range(2):
                y = new_m[k][j].cpu()
                assert not bool(y[G:].any()) and not bool(y[:G][drawn].any()) and torch.equal(y[:G][~drawn], m[k][j][~drawn]), k
    assert "rotations" not in new_m
    # at the cap nothing is added and the inputs come back
    full = mcmc.MCMCControl(cap_max=G)
    same_p, same_m, info = mcmc.grow(gp, gm, full)
    assert same_p is gp and same_m is gm and info == dict(rows_in=G, rows_out=G, added=0)
