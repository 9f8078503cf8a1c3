"""CPU checks of tests/dense_gemm64.py: the float64 reference against float64 torch at every case shape; a faithful float32 emulation of
the kernels' arithmetic (hi / lo split, three products, fp32 accumulation step by step and slice by slice, the fp32 epilogue) that must
sit at or below HALF the bound at every case; and the wrong answers a GEMM kernel can give, each of which must exceed the bound at every
case it applies to.  Also: the plan siu3r_gemm_plan gives every case (a host function: no GPU), the closure of the hand-written kernel
lists, the error paths the GPU test shares, and the constant of the GELU polynomial."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_gemm64 as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# reference vs float64 torch
# ------------------------------------------------------------------------------------------------
def torch_composition(c, inp):
    """the case's operation built from torch.nn.functional in float64 (and the oracle's rope2d): [Z, M, N], or None when the reference's
    operand is not what the torch form would normalise (a folded LayerNorm over rounded rows: checked through its statistics instead)"""
    from oracle import siu3r_oracle as O

    W = G.weights(c, inp)  # [Z, N, K]
    Z = c.Z
    if c.a_mode == 0:
        A = G.gather_rows(c, inp)
        lin = torch.stack([F.linear(A[z], W[z]) for z in range(Z)])
        if c.shuffle:
            up, co = c.shuffle
            B, ih, iw = c.smap
            x = A[0].view(B, ih, iw, c.k).permute(0, 3, 1, 2)
            wt = W[0].view(up, up, co, c.k).permute(3, 2, 0, 1)
            y = F.conv_transpose2d(x, wt, inp["bias"][0].double() if c.bias else None, stride=up).permute(0, 2, 3, 1)
            assert torch.allclose(G.shuffle_out(c, lin + (inp["bias"][0].double()[torch.arange(c.n) % co] if c.bias else 0)), y, rtol=1e-12, atol=1e-12)
    elif c.a_mode == 1:
        cv = c.conv
        x = inp["img"].double()
        x = G.rne_bf16(x).double() if c.mode == "f32" else x
        x = x.clamp_min(0) if c.relu_in else x
        wt = W[0].view(c.n, cv.kh, cv.kw, cv.cin).permute(0, 3, 1, 2)
        lin = F.conv2d(x.permute(0, 3, 1, 2), wt, None, stride=cv.stride, padding=cv.pad).permute(0, 2, 3, 1).reshape(1, c.m, c.n)
    else:
        x = inp["img"].double()
        x = G.rne_bf16(x).double() if c.mode == "f32" else x
        lin = F.conv2d(x, W[0].view(c.n, 3, 16, 16), None, stride=16).permute(0, 2, 3, 1).reshape(1, c.m, c.n)
    bi = [c.bias_index(z) for z in range(Z)]
    if c.ln:
        return None
    v = lin
    if c.bias:
        b = inp["bias"].double()[bi]
        v = v + (b[:, torch.arange(c.n) % c.shuffle[1]] if c.shuffle else b)[:, None, :]
    if c.rope:
        nc = c.rope
        pos = inp["rope_pos"].view(Z, c.m, 2)
        t = v[..., :nc].reshape(Z, c.m, nc // 64, 64).permute(0, 2, 1, 3)
        # (the oracle builds its table from the positions; the case's fp32 table is the same function of the position)
        cos, sin = O.rope2d_table(G.ROPE_MAX_POS, 64)
        assert torch.equal(cos, inp["rope_cos"]) and torch.equal(sin, inp["rope_sin"])
        r = O.rope2d(t, pos).permute(0, 2, 1, 3).reshape(Z, c.m, nc)
        v = torch.cat([r, v[..., nc:]], dim=-1)
    if c.act == 1:
        v = F.gelu(v)
    elif c.act == 2:
        v = F.relu(v)
    if c.up_src:
        cv = c.conv
        u = F.interpolate(inp["up"].double().permute(0, 3, 1, 2), size=(cv.oh, cv.ow), mode="bilinear", align_corners=True)
        v = v + u.permute(0, 2, 3, 1).reshape(1, c.m, c.n)
    if c.res:
        v = v + inp["residual"].double()
    return v


def check_ln_statistics(c, inp):
    """mean / rstd of the reference are those of F.layer_norm over the fp32 rows; the partials merge to them; and with unrounded rows
    (bf16x3) the fold equals LayerNorm followed by the Linear"""
    part = inp["ln_part"].double()
    T = part.shape[2]
    cnt = torch.tensor([min(64, c.k - 64 * t) for t in range(T)], dtype=torch.float64)
    mean = (part[..., 0] * cnt).sum(-1) / c.k
    m2 = (part[..., 1] + cnt * (part[..., 0] - mean[..., None]) ** 2).sum(-1)
    assert torch.allclose(mean, inp["ln_mean"], rtol=0, atol=1e-6)
    assert torch.allclose(1.0 / torch.sqrt(m2 / c.k + 1e-6), inp["ln_rstd"], rtol=1e-5)
    if c.mode == "bf16x3":
        A = inp["A"].double()
        ln = F.layer_norm(A, (c.k,), eps=float(np.float32(1e-6)))
        assert torch.allclose((A - inp["ln_mean"][..., None]) * inp["ln_rstd"][..., None], ln, rtol=1e-9, atol=1e-9)
        W = G.weights(c, inp)
        ref = G.reference(c, inp)["out"]
        want = torch.stack([F.linear(ln[c.a_index(z)], W[z]) + inp["ln_c2"].double()[c.bias_index(z)] for z in range(c.Z)])
        if not (c.act or c.res or c.rope):
            assert torch.allclose(ref, want, rtol=1e-6, atol=1e-5)  # (c1 is the fp32 value the kernel reads)


# ------------------------------------------------------------------------------------------------
# faithful emulation and the wrong answers
# ------------------------------------------------------------------------------------------------
class Emulation:
    """float32 arithmetic of the kernels: per K step (16 fp32 / 32 bf16 elements) the three bf16 products with fp32 sums, accumulated
    step by step inside a split-K slice and slice by slice; then the epilogue in float32 (G.epilogue with a float32 accumulator)."""

    def __init__(self, c, inp, *, trunc_a=False, same_side=False):
        self.c, self.inp = c, inp
        st, kp = c.step, c.kpad
        if trunc_a:    # fp32 rows cut to their upper 16 bits where the kernel rounds to nearest even
            A = G.trunc_bf16(G.gather_rows(_AsX3(c), inp, torch.float32))
        else:          # (same_side: every inner batch index reads its own rows, as if sa_i were not negative)
            A = G.gather_rows(_Unflipped(c) if same_side else c, inp, torch.float32)
        A = F.pad(A, (0, kp - c.k))
        Whi = inp["w_hi"][[c.w_index(z) for z in range(c.Z)]]
        Wlo = inp["w_lo"][[c.w_index(z) for z in range(c.Z)]]
        if c.mode == "bf16x3":
            # ping-pong / LDS-DMA / skinny kernels: hi = the upper 16 bits; the register-staged kernel rounds hi (split_bf16x8)
            Ahi = G.rne_bf16(A) if c.kernel.startswith("gemm_kernel") else G.trunc_bf16(A)
            Alo = G.rne_bf16(A - Ahi)
        else:
            Ahi, Alo = A, None
        s4 = lambda t: t.reshape(t.shape[0], t.shape[1], kp // st, st)
        prod = lambda a, w: torch.einsum("zmsk,znsk->szmn", s4(a), s4(w))
        self.hh = prod(Ahi, Whi)
        self.lh = prod(Alo, Whi) if Alo is not None else None
        self.hl = prod(Ahi, Wlo) if Alo is not None else None
        self.S = torch.einsum("zmk,znk->zmn", A.double().abs(), (Whi.double() + Wlo.double()).abs())

    def acc(self, mut=None, step=None):
        c, st = self.c, self.c.step
        ns = c.kpad // st
        starts = [s0 // st for s0 in c.slice_starts()] + [ns]
        tail0 = (c.k // 64 * 64) // st
        total = None
        for j in range(len(starts) - 1):
            a = torch.zeros_like(self.hh[0])
            steps = list(range(starts[j], starts[j + 1]))
            if mut == "skip" and j == 1:
                steps = steps[1:]
            if mut == "twice" and j == 1:
                steps = [steps[0]] + steps
            for s in steps:
                if mut == "tail" and s >= tail0:
                    continue
                if self.lh is not None:
                    if not (mut == "drop_lh" and s == step):
                        a = a + self.lh[s]
                    if not (mut == "drop_hl" and s == step):
                        a = a + self.hl[s]
                a = a + self.hh[s]
            total = a if total is None else total + a
        return total

    def run(self, mut=None, step=None):
        acc = self.acc(mut, step)
        return G.epilogue(self.c, self.inp, acc, self.S.float(), mut)


class _Proxy:
    def __init__(self, c):
        self.__dict__["_c"] = c

    def __getattr__(self, k):
        return getattr(self._c, k)


class _Unflipped(_Proxy):
    def a_index(self, z):
        return z


class _AsX3(_Proxy):
    mode = "bf16x3"  # (gather_rows leaves fp32 rows unrounded)


def _ratio(c, got, ref, key="out", stored=True):
    """stored: as the launch stores it (a bf16 C is rounded, and allowed that one rounding); else the fp32 value in front of the store"""
    bnd = G.bound(c)
    bf = c.c_bf16 and key == "out" and stored
    extra = G.bf16_extra(ref[key], ref["S"], bnd) if bf else None
    o = got[key]
    if bf:
        o = G.rne_bf16(o)
    return G.worst_ratio(o, ref[key], ref["S"] if key == "out" else ref["stats_S"], bnd, extra)[0]


def mutations(c, inp):
    """(kind, step) of every wrong answer that applies to the case.  The dropped product's step: the one the first sentinel column of W
    lives in (every other row of A is dense there); with a single row of A, that row's own step"""
    s = next(s for (kind, _, s) in inp["sentinels"] if kind == ("w" if c.m > 1 or c.a_mode else "a"))
    out = []
    if c.mode == "bf16x3":
        out += [("drop_lh", s), ("drop_hl", s)]
    if c.splitk > 1:
        out += [("skip", None), ("twice", None)]
    if c.k % 64:
        out.append(("tail", None))
    if c.bias:
        out.append(("bias_shift", None))
    if c.res:
        out.append(("res_shift", None))
        if c.act:
            out.append(("res_first", None))
        if c.stats:
            out.append(("stats_pre", None))
    if c.rope:
        out.append(("rope_sign", None))
        if c.rope + 64 <= c.n:
            out.append(("rope_head", None))
    if c.mode == "f32":
        out.append(("trunc_a", None))
    if c.flip:
        out.append(("same_side", None))
    return out


@pytest.mark.parametrize("c", G.CASES, ids=[c.id for c in G.CASES])
def test_reference_emulation_and_wrong_answers(c):
    inp = G.make_inputs(c)
    ref = G.reference(c, inp)
    assert torch.isfinite(ref["out"]).all() and (ref["S"] > 0).all()
    # ---- the reference against float64 torch
    want = torch_composition(c, inp)
    if want is not None:
        assert torch.allclose(ref["out"], want, rtol=1e-11, atol=1e-11), float((ref["out"] - want).abs().max())
    else:
        check_ln_statistics(c, inp)
    if c.stats:
        T = (c.n + 63) // 64
        for t in range(T):
            blk = ref["out"][..., 64 * t:min(c.n, 64 * t + 64)]
            assert torch.allclose(ref["stats"][..., t, 0], blk.mean(-1)) and torch.allclose(ref["stats"][..., t, 1], blk.var(-1, unbiased=False) * blk.shape[-1])
    # ---- sentinels: every sentinel row / column is zero outside its step, and the covered steps are the ones the case asks for
    st = c.step
    assert {s for (_, _, s) in inp["sentinels"]} >= set(c.sentinel_steps()) or len(inp["sentinels"]) < len(c.sentinel_steps())
    for (kind, r, s) in inp["sentinels"]:
        row = inp["A"][:, r] if kind == "a" else inp["W"][:, r]
        assert (row[..., :s * st] == 0).all() and (row[..., (s + 1) * st:] == 0).all() and (row[..., s * st:(s + 1) * st] != 0).any()
    # ---- the faithful emulation: at most half the bound
    emu = Emulation(c, inp)
    good = emu.run()
    w = _ratio(c, good, ref, stored=False)
    line = f"[emulation] {c.id}: faithful {w:.3f} of the bound {G.bound(c):.2e}"
    assert w <= 0.5, f"{c.id}: the faithful emulation reaches {w:.3f} of the bound: change the case's inputs, not the bound"
    assert _ratio(c, good, ref) <= 1.0  # (a bf16 C: plus its one rounding, which is tight)
    if c.stats:
        ws = _ratio(c, good, ref, "stats")
        line += f", statistics {ws:.3f}"
        assert ws <= 0.5, (c.id, ws)
    # ---- every wrong answer: above the bound
    for (kind, step) in mutations(c, inp):
        if kind == "trunc_a":
            bad = Emulation(c, inp, trunc_a=True).run()
        elif kind == "same_side":
            bad = Emulation(c, inp, same_side=True).run()
        else:
            bad = emu.run(kind, step)
        r = _ratio(c, bad, ref, "stats" if kind == "stats_pre" else "out")
        line += f", {kind} {r:.1f}"
        assert r > 1.0, f"{c.id}: the wrong answer `{kind}` (step {step}) stays at {r:.3f} of the bound: the metric would not notice it"
    # ---- a stub row written at row M, and planes that start 64 columns late: the buffer checks notice
    if not c.shuffle:
        lay = G.layouts(c)["c"]
        parent = torch.full((lay.numel,), -1, dtype=torch.int32)
        idx = lay.index()
        written = torch.zeros(lay.numel, dtype=torch.bool)
        written[idx.flatten()] = True
        parent[idx.flatten()] = 5
        assert G.untouched(parent, -1, written) == []
        parent[idx[:, -1].flatten() + lay.ld] = 5  # row M of every batch item
        assert G.untouched(parent, -1, written), c.id
    if c.planes and c.planes[0] + 64 <= c.n:
        col0 = c.planes[0]
        o32 = good["out"].float()
        buf = o32.clone()
        buf[..., col0 + 64:] = G.split_planes(o32[..., col0 + 64:].contiguous())  # planes from col0 + 64 on: fp32 left in [col0, col0 + 64)
        with pytest.raises(AssertionError):
            G.check_planes(buf, col0, c32=o32, name=c.id)
        buf[..., col0:] = G.split_planes(o32[..., col0:].contiguous())
        G.check_planes(buf, col0, c32=o32, ref=ref["out"], S=ref["S"], bnd=G.bound(c), name=c.id)
    print(line)


def test_planes_round_trip():
    x = torch.randn(3, 5, 128)
    hi, lo = G.join_planes(G.split_planes(x))
    assert torch.equal(hi, G.trunc_bf16(x)) and torch.equal(lo, (x - hi).to(torch.bfloat16).float())
    assert ((hi.double() + lo.double() - x.double()).abs() <= G.PLANES_REL * x.double().abs()).all()


def test_gelu_fast_constant():
    """GELU_FAST_MEASURED is the polynomial's worst error against the exact erf form over [-8, 8], relative to |x| (float32 restatement
    with an exact reciprocal); the bound term doubles it plus one ulp of the reciprocal"""
    x = np.concatenate([np.linspace(-8, 8, 2_000_001), np.float32(10.0) ** np.linspace(-6, 0.9, 20001), -(np.float32(10.0) ** np.linspace(-6, 0.9, 20001))]).astype(np.float32)
    x = x[x != 0]
    got = G.gelu_fast32(x).astype(np.float64)
    xd = x.astype(np.float64)
    want = 0.5 * xd * (1.0 + np.vectorize(math.erf)(xd / math.sqrt(2.0)))
    rel = float(np.max(np.abs(got - want) / np.abs(xd)))
    print(f"[gelu_fast] worst |gelu_fast - gelu| / |x| over [-8, 8] = {rel:.3e} (constant {G.GELU_FAST_MEASURED:.3e})")
    assert 0.8 * G.GELU_FAST_MEASURED <= rel <= G.GELU_FAST_MEASURED
    assert G.GELU_FAST_REL == 2.0 * (G.GELU_FAST_MEASURED + 2.0 ** -24)
    assert G.GELU_LIP >= 1.1290


# ------------------------------------------------------------------------------------------------
# plans (host function), closure of the lists
# ------------------------------------------------------------------------------------------------
def query_plan(c, ptr=None):
    from siu3r_amd import _lib

    lib = _lib.lib()
    p = G.fill_params(c, _lib.GemmParams(), ptr or G.fake_ptr(c))
    pl = _lib.GemmPlan()
    tune = {3: 1, **c.tune}
    try:
        for k, v in tune.items():
            _lib.check(lib.siu3r_gemm_tune(k, v))
        _lib.check(lib.siu3r_gemm_plan(C.byref(p), C.byref(pl)))
    finally:
        for k in tune:
            lib.siu3r_gemm_tune(k, 0)
    return p, pl


def assert_plan(c, pl):
    got = dict(kernel=pl.kernel.decode(), tile_cfg=pl.tile_cfg, splitk=pl.splitk, skinny_rows=pl.skinny_rows, skinny_path=pl.skinny_path,
               a_x3_ok=pl.a_x3_ok, c_x3_ok=pl.c_x3_ok)
    want = dict(kernel=c.kernel, tile_cfg=c.tile, splitk=c.splitk, skinny_rows=c.skinny, skinny_path=c.path, a_x3_ok=G.expect_a_x3_ok(c),
                c_x3_ok=G.expect_c_x3_ok(c))
    assert got == want, f"{c.id}: the plan is {got}, the case was written for {want}"
    wide = re.search(r"gemm_dma_kernel<2,|gemm_kernel<\d, \d, 2", c.kernel) is not None  # the 128 x 128 tile of the 128 x 64 family (A/B switch)
    assert (pl.bm, pl.bn) == ((128, 128) if wide else G.TILES[c.tile])
    return G.plan_key(got["kernel"], pl.skinny_path, c.x3, c.ln)


def test_every_default_case_gets_its_plan_and_every_kernel_a_case():
    """siu3r_gemm_plan on the placement the GPU test uses (fake addresses with the same alignment): every default case gets the kernel,
    tile, slices, remainder-row path and plane flags it was written for, and the plan names over the default cases are exactly
    KERNELS_DEFAULT -- a retuned cost constant or a new dispatch branch that moves a case, or leaves a kernel without one, fails here
    by name"""
    keys = [assert_plan(c, query_plan(c)[1]) for c in G.DEFAULT_CASES]
    seen = sorted({k for k, _ in keys})
    assert seen == G.KERNELS_DEFAULT, f"without a case: {sorted(set(G.KERNELS_DEFAULT) - set(seen))}; not in the list: {sorted(set(seen) - set(G.KERNELS_DEFAULT))}"
    skinny = sorted({s for _, s in keys if s})
    assert skinny == G.SKINNY_DEFAULT, (skinny, G.SKINNY_DEFAULT)


def test_kernel_lists_are_closed():
    assert not set(G.KERNELS_SWITCH_ONLY) & set(G.KERNELS_DEFAULT)
    assert len(set(G.KERNELS_DEFAULT)) == len(G.KERNELS_DEFAULT) and len(set(G.KERNELS_SWITCH_ONLY)) == len(G.KERNELS_SWITCH_ONLY)
    assert {c.kernel for c in G.DEFAULT_CASES} == set(G.KERNELS_DEFAULT)
    assert set(G.KERNELS_SWITCH_ONLY) <= {c.kernel for c in G.SWITCH_CASES}
    assert {c.kernel for c in G.SWITCH_CASES} <= set(G.KERNELS_SWITCH_ONLY) | set(G.KERNELS_DEFAULT)  # (remainder-row switches keep the tile kernel)
    # every instantiation the launch code names is on one of the lists
    import re
    src = lambda f: open(os.path.join(ROOT, "siu3r_amd", "csrc", f)).read()
    n_pp = sum(len(re.findall(r"SIU3R_PP_GO\(\d", src(f"gemm_pp_t{n}{m}.hip"))) + len(re.findall(r"hipLaunchKernelGGL\(\(gemm_pp_kernel<", src(f"gemm_pp_t{n}{m}.hip"))) - 1
               for n in (1, 2, 3) for m in "xb")
    assert n_pp == len([k for k in G.KERNELS_DEFAULT if "gemm_pp_kernel" in k]) == 39
    assert len(re.findall(r"hipLaunchKernelGGL\(\(gemm_kernel<", src("gemm.hip"))) * 2 == len([k for k in G.KERNELS_DEFAULT + G.KERNELS_SWITCH_ONLY if k.startswith("gemm_kernel<")]) == 12
    assert len([k for k in G.KERNELS_DEFAULT + G.KERNELS_SWITCH_ONLY if "gemm_dma_kernel<" in k]) == 5 * 4      # SIU3R_DMA_MODES: 5 launches x (NI, KS)
    assert len(re.findall(r"hipLaunchKernelGGL\(\(gemm_dma_x3_kernel<", src("gemm_dma.hip"))) == len([k for k in G.KERNELS_DEFAULT + G.KERNELS_SWITCH_ONLY if "gemm_dma_x3_kernel<" in k]) == 10
    assert len(re.findall(r"hipLaunchKernelGGL\(\(gemm_skinny(?:_gemv)?_kernel<", src("gemm_pp.hip"))) == len([s for s in G.SKINNY_DEFAULT if s[0] > 1]) == 8


def test_cost_model_reaches_every_tile():
    """tile_cfg 0 with the table off: the cost model picks each ping-pong tile and the 128 x 64 kernel somewhere (shapes too large to
    run as cases: the plan is only queried)"""
    from siu3r_amd import _lib

    lib = _lib.lib()
    want = {(8192, 4096, 1024): 1, (4096, 2048, 1024): 2, (1024, 1024, 4096): 3, (129, 64, 64): -1}
    try:
        _lib.check(lib.siu3r_gemm_tune(3, 1))
        for (m, n, k), cfg in want.items():
            p = _lib.GemmParams()
            p.a, p.w_hi, p.w_lo, p.w_x3, p.c = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 30
            p.m, p.n, p.k, p.kpad, p.lda, p.ldc = m, n, k, k, k, n
            p.a_dtype = p.c_dtype = _lib.F32
            p.splitk = 1
            pl = _lib.GemmPlan()
            _lib.check(lib.siu3r_gemm_plan(C.byref(p), C.byref(pl)))
            assert pl.tile_cfg == cfg, ((m, n, k), pl.tile_cfg, pl.kernel)
    finally:
        lib.siu3r_gemm_tune(3, 0)


# ------------------------------------------------------------------------------------------------
# error paths (shared with the GPU test)
# ------------------------------------------------------------------------------------------------
VALIDATION_ERRORS = [
    (dict(a=0), r"null operand pointer"),
    (dict(c=0), r"null operand pointer"),
    (dict(m=0), r"empty problem \(m=0"),
    (dict(kpad=72), r"kpad=72 must be a multiple of 64"),
    (dict(k=128, lda=128), r"kpad=64 must be a multiple of 64 and >= k=128"),
    (dict(a_dtype=5), r"bad a_dtype 5"),
    (dict(c_dtype=7), r"bad c_dtype 7"),
    (dict(a_dtype=0), r"bf16x3 mode needs fp32 activations"),
    (dict(a_mode=3), r"bad a_mode 3"),
    (dict(a_mode=1, ih=8, iw=8, cin=8, kh=1, kw=1, stride=1, oh=0, ow=8), r"conv geometry must be positive"),
    (dict(k=60, lda=64), r"dense A needs k % 8 == 0"),
    (dict(lda=68), r"dense A needs k % 8 == 0 and lda % 8 == 0"),
    (dict(a_mode=1, ih=8, iw=8, cin=6, kh=1, kw=1, stride=1, oh=8, ow=8), r"conv gather needs cin % 8 == 0"),
    (dict(a_mode=1, ih=8, iw=8, cin=8, kh=3, kw=3, stride=1, pad=1, oh=8, ow=8), r"conv k=64 != kh\*kw\*cin"),
    (dict(a_mode=1, ih=8, iw=8, cin=64, kh=1, kw=1, stride=1, oh=8, ow=7), r"conv m=128 not a multiple of oh\*ow"),
    (dict(a_mode=2, ih=32, iw=64, oh=2, ow=4), r"patchify mode needs fp32 NCHW input, k=768"),
    (dict(out_mode=1, up=2, cout=12, ih=8, iw=16), r"bad conv-transpose geometry"),
    (dict(rope_cos=1 << 20), r"bad RoPE epilogue arguments"),
    (dict(rope_cos=1 << 20, rope_sin=1 << 20, rope_pos=1 << 20, rope_ncols=32), r"bad RoPE epilogue arguments"),
    (dict(up_src=1 << 20), r"up_src needs conv mode with even output size"),
    (dict(ln_stats=1 << 20, ln_c1=1 << 20, ln_c2=1 << 20, ln_tiles=2, bias=0), r"folded LayerNorm needs .*\(k=64, ln_tiles=2\)"),
    (dict(ln_stats=1 << 20, ln_c1=1 << 20, ln_c2=1 << 20, ln_tiles=1), r"folded LayerNorm needs c1/c2, no bias"),
    (dict(out_mode=1, up=2, cout=16, ih=8, iw=16, stats_out=1 << 20), r"stats_out needs a plain row-major output"),
    (dict(out_mode=1, up=2, cout=16, ih=8, iw=16, c_aux=1 << 20), r"c_aux needs a plain row-major output"),
    (dict(splitk=2, sk_ws=0), r"split-K needs a workspace, zeroed counters and splitk <= kpad / 64 \(splitk=2\)"),
    (dict(tile_cfg=4), r"bad tile_cfg 4"),
    (dict(batch=3, bmod=2), r"batch 3 is not a multiple of bmod 2"),
]
LAUNCH_ERRORS = [  # siu3r_gemm's own checks, behind the plan
    (dict(a_x3=1, tile_cfg=-1), r"a_x3 \(pre-split A planes\) needs a ping-pong plan.*this block runs siu3r_gemm_dma::gemm_dma_x3_kernel<0, false, 2, false>"),
    (dict(c_x3=1 << 21, tile_cfg=-1), r"c_x3 \(output planes\) needs a ping-pong plan"),
    (dict(c_x3=1 << 21, tile_cfg=3, ldc=68), r"c_x3 \(output planes\) needs a ping-pong plan and the plain fp32 row-major output form"),
    (dict(splitk=2, k=128, kpad=128, lda=128, sk_ws_floats=64), r"splitk=2 was requested but .* cannot split K for this problem"),
]


def error_params(_lib, **fields):
    """a valid bf16x3 block (128 x 64 x 64, bias) with the fields overridden; the addresses are never dereferenced by what fails"""
    p = _lib.GemmParams()
    p.a, p.w_hi, p.w_lo, p.w_x3, p.c, p.bias = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
    p.m, p.n, p.k, p.kpad, p.lda, p.ldc = 128, 64, 64, 64, 64, 64
    p.a_dtype = p.c_dtype = p.r_dtype = _lib.F32
    p.splitk = 1
    p.sk_ws, p.sk_cnt, p.sk_ws_floats, p.sk_cnt_n = 7 << 20, 8 << 20, 1 << 20, 64
    for f, v in fields.items():
        setattr(p, f, v)
    return p


def error_paths(params, call, launch=False):
    """every SIU3R_CHECK of validate_gemm (launch=False: through whatever `call` reaches, the plan query or the launch) and of
    siu3r_gemm itself (launch=True), each with its own message"""
    for fields, msg in (LAUNCH_ERRORS if launch else VALIDATION_ERRORS):
        with pytest.raises(RuntimeError, match=msg):
            call(params(**fields))


def test_error_paths_through_the_plan_query():
    from siu3r_amd import _lib

    def plan(p):
        pl = _lib.GemmPlan()
        _lib.check(_lib.lib().siu3r_gemm_plan(C.byref(p), C.byref(pl)))
        return pl

    assert plan(error_params(_lib)).kernel.decode() == G.k_dmax()
    error_paths(lambda **f: error_params(_lib, **f), plan)
    # every check of validate_gemm has an entry (three of them have two)
    import re
    body = open(os.path.join(ROOT, "siu3r_amd", "csrc", "gemm.hip")).read()
    body = body[body.index("static int validate_gemm"):body.index('extern "C" int siu3r_gemm_plan')]
    assert len(re.findall(r"SIU3R_CHECK\(", body)) == len(VALIDATION_ERRORS) - 5 == 22
