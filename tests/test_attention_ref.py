"""CPU tests of the attention reference and metric (tests/dense_attention64.py): the float64 reference agrees with torch's own
attention and the oracle's RoPE2D; for every case shape of tests/test_attention_gpu.py the sentinel margins and the row-size
condition hold on the reference alone, and assert_rows_close rejects every kind of wrong answer a kernel could plausibly give, at the
case's own tolerance; siu3r_attention_plan (a host function) gives every case the kernel it expects and validates like the launch."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import dense_attention64 as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -1.0e30  # the kernels' NEG_BIG


# ------------------------------------------------------------------------------------------------
# the reference itself
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 17, 33, 32), (1, 2, 5, 70, 64)], ids=["d32", "d64"])
def test_reference_agrees_with_torch_sdpa(shape):
    B, H, Nq, Nk, D = shape
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(B, n, H, D, generator=g, dtype=torch.float64) for n in (Nq, Nk, Nk))
    blocked = torch.rand(B, Nq, Nk, generator=g) < 0.6
    blocked[:, :, 3] = False
    perm = lambda t: t.permute(0, 2, 1, 3)
    for mask in (None, blocked):
        ref = F.scaled_dot_product_attention(perm(q), perm(k), perm(v), attn_mask=None if mask is None else ~mask[:, None], scale=0.25)
        ld = 128
        mpad = None
        if mask is not None:
            mpad = torch.zeros(B, Nq, ld, dtype=torch.uint8)  # padding of zeros ("admitted") must be ignored
            mpad[:, :, :Nk] = mask.to(torch.uint8)
        got = A.dense_attention64(q, k, v, 0.25, mask=mpad)
        assert torch.allclose(got, perm(ref).flatten(2), rtol=0, atol=1e-12)
    # kv_bxor: batch item b reads the K / V of item b ^ 1; strided views
    big = torch.randn(2, Nk + 3, 3, H, D, generator=g, dtype=torch.float64)
    kk, vv = big[:, :Nk, 1], big[:, :Nk, 2]
    ref = F.scaled_dot_product_attention(perm(q), perm(kk.flip(0)), perm(vv.flip(0)), scale=0.25) if B == 2 else None
    if ref is not None:
        assert torch.allclose(A.dense_attention64(q, kk, vv, 0.25, kv_bxor=1), perm(ref).flatten(2), rtol=0, atol=1e-12)


def test_reference_rope_agrees_with_the_oracle():
    from oracle import siu3r_oracle as O

    B, H, N, D = 2, 3, 19, 64
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, N, H, D, generator=g)
    pos = torch.randint(0, 30, (B, N, 2), generator=g)
    pos[0, 0], pos[0, 1] = torch.tensor([0, 29]), torch.tensor([29, 0])
    cos, sin = O.rope2d_table(30, D)
    want = O.rope2d(x.permute(0, 2, 1, 3), pos).permute(0, 2, 1, 3)
    got = A.rope2d64(x.double(), pos, cos, sin)
    assert (got - want.double()).abs().max() < 2e-5  # the oracle works in float32
    # and through the whole reference: RoPE on q and k, then plain attention
    q, k, v = x, torch.randn(B, N, H, D, generator=g), torch.randn(B, N, H, D, generator=g)
    kpos = torch.randint(0, 30, (B, N, 2), generator=g)
    perm = lambda t: t.permute(0, 2, 1, 3)
    ref = F.scaled_dot_product_attention(O.rope2d(perm(q), pos).double(), O.rope2d(perm(k), kpos).double(), perm(v).double(), scale=0.125)
    got = A.dense_attention64(q, k, v, 0.125, rope=(cos, sin), qpos=pos, kpos=kpos)
    assert (got - perm(ref).flatten(2)).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------
# wrong answers the metric must reject
# ------------------------------------------------------------------------------------------------
def _softmax_v(s, v):
    """like A.weighted64, but a row without keys gives NaN (what a kernel's 0 / 0 gives) instead of an assertion; v already per batch item"""
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    return torch.einsum("bhqk,bkhd->bqhd", p / p.sum(-1, keepdim=True), v).flatten(2)


def _vv(c, inp):
    v = inp["v"].double()
    return v[torch.arange(c.B) ^ c.kv_bxor]


def _logits(c, inp, **over):
    kw = dict(rope=inp["rope"], qpos=inp["qpos"], kpos=inp["kpos"], mask=inp["mask"], kv_bxor=c.kv_bxor)
    kw.update(over)
    return A.logits64(inp["q"], inp["k"], inp["scale"], **kw)


def mut_last_key_dropped(c, inp, s):
    s = s.clone()
    s[..., c.Nk - 1] = float("-inf")
    return _softmax_v(s, _vv(c, inp))


def mut_first_key_of_a_range_dropped(c, inp, s):
    s = s.clone()
    s[..., int(c.key_parts()[0][0])] = float("-inf")
    return _softmax_v(s, _vv(c, inp))


def mut_keys_beyond_nk_admitted(c, inp, s):
    """the clamped loads supply K / V row Nk - 1 for the keys Nk .. 64 * nkt - 1; their mask bytes are the padding"""
    ndup = -c.Nk % 64
    if ndup == 0 or c.Nk < 2 or c.mask == "ones":  # (padding of ones masks them again: exactly why the cases also pad with zeros)
        return None
    raw = _logits(c, inp, mask=None)[..., c.Nk - 1:]
    s = torch.cat([s, raw + math.log(ndup)], -1)
    v = _vv(c, inp)
    return _softmax_v(s, torch.cat([v, v[:, -1:]], 1))


def mut_mask_shifted_by_one_key(c, inp, s):
    if inp["mask"] is None or c.Nk < 2:
        return None
    m = inp["mask"].clone()
    m[:, :, :c.Nk] = torch.roll(inp["mask"][:, :, :c.Nk], 1, dims=2)
    return _softmax_v(_logits(c, inp, mask=m), _vv(c, inp))


def mut_mask_padding_honoured_as_data(c, inp, s):
    """rows taken ceil64(Nk) bytes apart instead of mask_ld: the padding is read as the next rows' mask"""
    if inp["mask"] is None or c.ld_extra == 0:
        return None
    nk64 = (c.Nk + 63) // 64 * 64
    flat = inp["mask"].flatten()
    m = flat[:c.B * c.Nq * nk64].view(c.B, c.Nq, nk64).clone()
    if torch.equal(m[:, :, :c.Nk], inp["mask"][:, :, :c.Nk]):  # (one key, open in every row, zeros behind it: nothing to get wrong)
        return None
    return _softmax_v(_logits(c, inp, mask=m), _vv(c, inp))


def mut_two_v_rows_swapped(c, inp, s):
    if c.Nk < 2:
        return None
    b, r, h, t, _ = inp["sentinels"][0]
    v = _vv(c, inp).clone()
    t2 = (t + 1) % c.Nk
    v[b, [t, t2], h] = v[b, [t2, t], h]
    return _softmax_v(s, v)


def mut_kv_of_the_own_batch_item(c, inp, s):
    if c.kv_bxor == 0:
        return None
    return _softmax_v(_logits(c, inp, kv_bxor=0), inp["v"].double())


def mut_rope_skipped_on_k(c, inp, s):
    if inp["rope"] is None:
        return None
    zero = torch.zeros_like(inp["kpos"])  # position 0 = identity
    return _softmax_v(_logits(c, inp, kpos=zero), _vv(c, inp))


def mut_q_position_used_for_k(c, inp, s):
    if inp["rope"] is None:
        return None
    kpos = inp["qpos"][:, torch.arange(c.Nk) % c.Nq]
    return _softmax_v(_logits(c, inp, kpos=kpos), _vv(c, inp))


def mut_normaliser_misses_one_key(c, inp, s):
    near = [x for x in inp["sentinels"] if x[4] >= 0]
    b, r, h, t, n = near[0] if near else inp["sentinels"][0]
    key = n if n >= 0 else t
    out = _softmax_v(s, _vv(c, inp)).view(c.B, c.Nq, c.H, c.D).clone()
    w = torch.softmax(s[b, h, r], -1)[key]
    out[b, r, h] = out[b, r, h] / (1 - w)
    return out.flatten(2)


def mut_partial_merged_with_weight_one(c, inp, s):
    """the partial (m_s, l_s, O_s) of the FIRST key part enters the merge with weight 1 instead of exp(m_s - M); a fully masked part
    is the kernels' (NEG_BIG, count, sum of V rows)"""
    parts = c.key_parts()
    if len(parts) < 2:
        return None
    v = _vv(c, inp)
    sn = torch.where(torch.isfinite(s), s, torch.full_like(s, NEG))
    ms, ls, os_ = [], [], []
    for p in parts:
        sp = sn[..., p]
        m = sp.amax(-1, keepdim=True)
        e = torch.exp(sp - m)
        ms.append(m)
        ls.append(e.sum(-1, keepdim=True))
        os_.append(torch.einsum("bhqk,bkhd->bhqd", e, v[:, p]))
    M = torch.stack(ms).amax(0)
    ws = [torch.exp(m - M) for m in ms]
    ws[0] = torch.ones_like(ws[0])
    L = sum(w * l for w, l in zip(ws, ls))
    O = sum(w * o for w, o in zip(ws, os_))
    return (O / L).permute(0, 2, 1, 3).flatten(2)


MUTATIONS = [mut_last_key_dropped, mut_first_key_of_a_range_dropped, mut_keys_beyond_nk_admitted, mut_mask_shifted_by_one_key,
             mut_mask_padding_honoured_as_data, mut_two_v_rows_swapped, mut_kv_of_the_own_batch_item, mut_rope_skipped_on_k,
             mut_q_position_used_for_k, mut_normaliser_misses_one_key, mut_partial_merged_with_weight_one]


@pytest.mark.parametrize("c", A.CASES, ids=[c.id for c in A.CASES])
def test_metric_rejects_every_wrong_answer(c):
    inp = A.make_inputs(c)
    s, ref = A.reference(c, inp)
    tol = A.MODES[c.mode][2]
    A.check_margins(c, inp, s)
    # the conditions on the reference alone (row size), and the reference against itself
    assert A.assert_rows_close(ref, ref, inp["v_scale_ref"], tol, kv_bxor=c.kv_bxor, name=c.id, quiet=True) == 0.0
    applied = 0
    for mut in MUTATIONS:
        wrong = mut(c, inp, s)
        if wrong is None:
            continue
        applied += 1
        with pytest.raises(AssertionError, match=r"\|out - ref\|"):
            A.assert_rows_close(wrong, ref, inp["v_scale_ref"], tol, kv_bxor=c.kv_bxor, name=f"{c.id} {mut.__name__}", quiet=True)
    assert applied >= (3 if c.Nk > 1 else 2), applied
    # a result off by just over the tolerance in one element is rejected, just under it accepted
    vmax = A.row_scales(inp["v_scale_ref"], c.kv_bxor)
    b, r, h = c.B - 1, c.Nq - 1, c.H - 1
    for f, ok in ((0.98, True), (1.02, False)):
        o = ref.clone()
        o[b, r, h * c.D + c.D - 1] += f * tol * vmax[b, h]
        if ok:
            A.assert_rows_close(o, ref, inp["v_scale_ref"], tol, kv_bxor=c.kv_bxor, quiet=True)
        else:
            with pytest.raises(AssertionError, match=rf"b={b}, q={r}, h={h}, d={c.D - 1}"):
                A.assert_rows_close(o, ref, inp["v_scale_ref"], tol, kv_bxor=c.kv_bxor, quiet=True)


def test_merge_emulation_is_the_reference_with_the_right_weights():
    """the key-part merge used by the weight-1 mutation reproduces the reference when its weights are exp(m_s - M), fully masked parts
    included: so the mutation differs from the reference by the weight alone"""
    c = next(x for x in A.CASES if x.ranges == 16 and x.mask and x.D == 32 and x.mode == "bf16")
    inp = A.make_inputs(c)
    s, ref = A.reference(c, inp)
    v = _vv(c, inp)
    sn = torch.where(torch.isfinite(s), s, torch.full_like(s, NEG))
    M = sn.amax(-1, keepdim=True)
    L, O = 0, 0
    for p in c.key_parts():
        sp = sn[..., p]
        m = sp.amax(-1, keepdim=True)
        e = torch.exp(sp - m)
        L = L + torch.exp(m - M) * e.sum(-1, keepdim=True)
        O = O + torch.exp(m - M) * torch.einsum("bhqk,bkhd->bhqd", e, v[:, p])
    assert ((O / L).permute(0, 2, 1, 3).flatten(2) - ref).abs().max() < 1e-12
    assert c.empty_ranges() == 3 and next(x for x in A.CASES if x.Nk == 2100).empty_ranges() == 1


def test_case_list_reaches_every_kernel():
    assert sorted({c.kernel for c in A.DEFAULT_CASES}) == A.KERNELS_DEFAULT
    assert set(A.KERNELS_SWITCH_ONLY) <= {c.kernel for c in A.SWITCH_CASES}
    assert not set(A.KERNELS_SWITCH_ONLY) & set(A.KERNELS_DEFAULT)


# ------------------------------------------------------------------------------------------------
# the plan query (a host function: pointers are only tested for null and alignment)
# ------------------------------------------------------------------------------------------------
def plan_params(c, **over):
    from siu3r_amd import _lib

    p = _lib.AttnParams()
    base = (1 << 20) + (0 if c.planes else 16)
    p.q, p.k, p.v, p.out = base, base, base, 1 << 20
    p.dtype = _lib.BF16 if c.mode == "bf16" else _lib.F32
    p.B, p.H, p.Nq, p.Nk, p.D = c.B, c.H, c.Nq, c.Nk, c.D
    sh, sn = c.D, 3 * (c.H + 2) * c.D
    p.q_sh = p.k_sh = p.v_sh = sh
    p.q_sn = p.k_sn = p.v_sn = sn
    p.q_sb, p.k_sb, p.v_sb = (c.Nq + 3) * sn, (c.Nk + 3) * sn, (c.Nk + 3) * sn
    p.scale = c.D ** -0.5
    if c.rope:
        p.rope_cos = p.rope_sin = p.qpos = p.kpos = 1 << 20
        p.rope_max_pos = A.ROPE_MAX_POS
    if c.mask:
        p.mask, p.mask_ld = (1 << 20) + 16, (c.Nk + 63) // 64 * 64 + c.ld_extra
    p.split3 = int(c.mode == "bf16x3")
    p.kv_bxor, p.kv_x3 = c.kv_bxor, int(c.planes)
    if c.splits > 1:
        p.splits, p.ws = c.splits, 1 << 20
    for k_, v_ in over.items():
        setattr(p, k_, v_)
    return p


def _plan(p):
    from siu3r_amd import _lib

    pl = _lib.AttnPlan()
    _lib.check(_lib.lib().siu3r_attention_plan(C.byref(p), C.byref(pl)))
    return pl


def check_plans(cases):
    for c in cases:
        pl = _plan(plan_params(c))
        got = (pl.kernel.decode(), pl.queries_per_wg, pl.key_ranges)
        assert got == (c.kernel, c.qpw, c.ranges), (c.id, got)
        assert pl.combine == int(c.ranges > 1) and pl.key_halves == int(c.qpw == 64 or "pipe" in c.kernel), (c.id, pl.combine, pl.key_halves)
        assert pl.side_path == int("pipe" in c.kernel and c.Nq > 128 and c.Nq % 128 == 1), (c.id, pl.side_path)


def test_plan_of_every_case():
    check_plans(A.DEFAULT_CASES)


@pytest.mark.parametrize("env", sorted({c.env for c in A.SWITCH_CASES}))
def test_plan_of_the_switch_cases(env):
    """the library reads its A/B switches when first used: a child process each"""
    code = f"import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests'); import test_attention_ref as T, dense_attention64 as A; " \
           f"T.check_plans([c for c in A.SWITCH_CASES if c.env == '{env}']); print('PLANS_OK')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **{env: "1"}), capture_output=True, text=True, timeout=120)
    assert "PLANS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def error_paths(params, call):
    """Every SIU3R_CHECK of siu3r_attention's validation, each with its own message.  params(**fields) -> a valid parameter block with
    the fields overridden; call(p) raises what the entry point under test reports."""
    sn = params().q_sn
    bad = [
        (dict(D=48), r"head_dim 48 unsupported"),
        (dict(Nk=0), r"empty problem"),
        (dict(Nq=0), r"empty problem"),
        (dict(mask=(1 << 20) + 16, mask_ld=96), r"key mask needs .*mask_ld=96 Nk=70"),
        (dict(mask=(1 << 20) + 16, mask_ld=64), r"key mask needs .*mask_ld=64 Nk=70"),
        (dict(mask=(1 << 20) + 8, mask_ld=128), r"key mask needs a 16-byte aligned buffer"),
        (dict(kv_bxor=2), r"kv_bxor=2 must be 2\^n - 1"),
        (dict(kv_bxor=1, B=3), r"kv_bxor=1 must be 2\^n - 1 with B a multiple"),
        (dict(kv_bxor=3, B=6), r"kv_bxor=3 must be 2\^n - 1 with B a multiple"),
        (dict(kv_bxor=1, rope_cos=1 << 20, rope_sin=1 << 20, qpos=1 << 20, kpos=1 << 20), r"kv_bxor=1 .*excludes RoPE on load"),
        (dict(D=32, rope_cos=1 << 20, rope_sin=1 << 20, qpos=1 << 20, kpos=1 << 20), r"RoPE2D path is specialised for head_dim 64"),
        (dict(rope_cos=1 << 20, rope_sin=1 << 20), r"rope tables/positions missing"),
        (dict(rope_cos=1 << 20, qpos=1 << 20, kpos=1 << 20), r"rope tables/positions missing"),
        (dict(k_sn=sn + 2), r"strides must keep 16-byte alignment"),
        (dict(v_sh=66), r"strides must keep 16-byte alignment"),
        (dict(dtype=0, split3=1), r"bf16x3 mode needs fp32 tensors"),
        (dict(kv_x3=1, Nk=40), r"kv_x3 \(pre-split K / V planes\) needs the pipelined"),
        (dict(kv_x3=1, mask=(1 << 20) + 16, mask_ld=128), r"kv_x3 \(pre-split K / V planes\) needs the pipelined"),
        (dict(q=0), r"null pointer"),
    ]
    for fields, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            call(params(**fields))


def _error_case():
    return A.Case("err", "bf16x3", 4, 2, 65, 70, 64, ("", 128, 1), planes=True)  # (planes: 128-byte aligned fake pointers)


def test_plan_and_launch_validate_alike():
    """(the launch returns from its validation before it touches the device: safe without a GPU)"""
    from siu3r_amd import _lib

    c = _error_case()
    params = lambda **f: plan_params(c, **dict(dict(kv_x3=0), **f))
    assert _plan(params()).kernel.decode() == "siu3r_attn_pipe::attn_pipe_kernel<true, false>"
    error_paths(params, _plan)
    error_paths(params, lambda p: _lib.check(_lib.lib().siu3r_attention(C.byref(p), None)))
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(_lib.lib().siu3r_attention_plan(C.byref(params()), None))
