"""Every dispatch branch of siu3r_attention against the float64 reference, row by row (tests/dense_attention64.py holds the reference,
the metric, the generator and the case list; tests/test_attention_ref.py shows on the CPU that the metric rejects every kind of
wrong answer at every case shape).

Every case asks siu3r_attention_plan which kernel will run and asserts it, runs once, and compares with assert_rows_close:
|out - ref| <= tol * Vmax per element, Vmax = max |v| of the (batch item, head) the row draws from, tol = the suite's TOL_BF16 / TOL_F32.
q, k, v and the mask are views into larger NaN-filled parents (other slots of an interleaved storage, rows beyond Nq / Nk, spare
heads), based 16 bytes off a 128-byte line (pre-split planes: on the line, as siu3r_attn_params.kv_x3 demands)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

import dense_attention64 as A
from test_attention_ref import error_paths

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_seen = {}  # case id -> kernel name the plan query gave


def _ops():
    from siu3r_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def _reference(cid):
    c = next(x for x in A.CASES if x.id == cid)
    inp = A.make_inputs(c)
    s, ref = A.reference(c, inp)
    A.check_margins(c, inp, s)
    return inp, ref


def _planes(x):
    """fp32 [B, N, H, 64] -> the same bytes as pre-split planes: per token and head two 128-byte segments [hi 32 | lo 32] bf16
    (hi = upper 16 bits, lo = bf16(x - hi)), carried in an fp32 tensor of the same shape"""
    x = x.contiguous()
    bits = x.view(torch.int32)
    hi = (bits >> 16).to(torch.int16)
    lo = (x - (bits & -65536).view(torch.float32)).to(torch.bfloat16).view(torch.int16)
    B, N, H, D = x.shape
    return torch.stack((hi.view(B, N, H, D // 32, 32), lo.view(B, N, H, D // 32, 32)), dim=4).reshape(B, N, H, 2 * D).view(torch.float32)


def _strided(x, dt, off_bytes):
    """x CPU fp32 [B, N, H, D] -> a device view of that shape inside a NaN-filled parent [B, N + 3, 3 slots, H + spare, D] whose first
    element lies off_bytes behind a 128-byte line"""
    B, N, H, D = x.shape
    Hp, S, Np = H + 2 + H % 2, 3, N + 3
    n = B * Np * S * Hp * D
    esz = 2 if dt == torch.bfloat16 else 4
    flat = torch.full((n + 64,), float("nan"), dtype=dt, device="cuda")
    assert flat.data_ptr() % 128 == 0
    parent = flat[off_bytes // esz:off_bytes // esz + n].view(B, Np, S, Hp, D)
    view = parent[:, :N, 1, :H]
    view.copy_(x.to(dt) if x.dtype != dt else x)
    assert view.data_ptr() % 128 == off_bytes and view.stride() == (Np * S * Hp * D, S * Hp * D, D, 1)
    return view


def _device_inputs(c, inp):
    dt = A.MODES[c.mode][0]
    q = _strided(inp["q"], dt, 16)
    if c.planes:
        k, v = _strided(_planes(inp["k"]), dt, 0), _strided(_planes(inp["v"]), dt, 0)
    else:
        k, v = _strided(inp["k"], dt, 16), _strided(inp["v"], dt, 16)
    kw = dict(heads=c.H, head_dim=c.D, scale=inp["scale"], split3=A.MODES[c.mode][1], kv_bxor=c.kv_bxor, kv_planes=c.planes)
    if inp["mask"] is not None:
        m = inp["mask"]
        flat = torch.full((m.numel() + 80,), 1, dtype=torch.uint8, device="cuda")
        mv = flat[16:16 + m.numel()].view(m.shape)
        mv.copy_(m)
        assert mv.data_ptr() % 128 == 16 and mv.is_contiguous()
        kw["mask"] = mv
    if inp["rope"] is not None:
        kw.update(rope=(inp["rope"][0].cuda(), inp["rope"][1].cuda()), qpos=inp["qpos"].cuda(), kpos=inp["kpos"].cuda())
    return q, k, v, kw


def run_case(c):
    ops = _ops()
    inp, ref = _reference(c.id)
    q, k, v, kw = _device_inputs(c, inp)
    pl = ops.attention(q, k, v, plan=True, **kw)
    got = (pl.kernel.decode(), pl.queries_per_wg, pl.key_ranges)
    _seen[c.id] = got[0]
    assert got == (c.kernel, c.qpw, c.ranges), f"{c.id}: the plan is {got}, the case was written for {(c.kernel, c.qpw, c.ranges)}"
    assert pl.combine == int(c.ranges > 1) and pl.side_path == int("pipe" in c.kernel and c.Nq > 128 and c.Nq % 128 == 1)
    out = ops.attention(q, k, v, **kw)
    torch.cuda.synchronize()
    assert out.shape == (c.B, c.Nq, c.H * c.D) and out.dtype == A.MODES[c.mode][0]
    return A.assert_rows_close(out, ref, inp["v_scale_ref"], A.MODES[c.mode][2], kv_bxor=c.kv_bxor, name=f"{c.id} {got[0]}")


@pytest.mark.parametrize("c", A.DEFAULT_CASES, ids=[c.id for c in A.DEFAULT_CASES])
def test_attention_branch(c):
    run_case(c)


def run_switch_cases(env):
    """(child process, the switch set in its environment)"""
    for c in A.SWITCH_CASES:
        if c.env == env:
            run_case(c)
    print(f"SWITCH_CASES_OK {env} " + " | ".join(sorted(set(_seen.values()))))


@pytest.mark.parametrize("env", sorted({c.env for c in A.SWITCH_CASES}))
def test_attention_switch_only_instantiations(env):
    """SIU3R_ATTN_NO_FAST / SIU3R_ATTN_NO_PIPE are read when the library is first used: one child process each, one at a time"""
    code = f"import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests'); import test_attention_gpu as T; T.run_switch_cases('{env}')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **{env: "1"}), capture_output=True, text=True, timeout=300)
    print(out.stdout[-6000:])
    marker = [l for l in out.stdout.splitlines() if l.startswith(f"SWITCH_CASES_OK {env} ")]
    assert out.returncode == 0 and marker, out.stdout[-3000:] + out.stderr[-3000:]
    want = {c.kernel for c in A.SWITCH_CASES if c.env == env}
    assert set(marker[0][len(f"SWITCH_CASES_OK {env} "):].split(" | ")) == want


def test_every_default_kernel_has_a_case():
    """The kernels siu3r_attention can launch without a switch (A.KERNELS_DEFAULT, written out by hand from the dispatch code) are exactly
    the plan names of the parametrised cases: a new dispatch branch without a case, or a retuned threshold that moves a case to
    another kernel, fails here.  (Cases that did not run in this session are asked for their plan now; nothing is launched.)"""
    ops = _ops()
    for c in A.DEFAULT_CASES:
        if c.id not in _seen:
            inp, _ = _reference(c.id)
            q, k, v, kw = _device_inputs(c, inp)
            _seen[c.id] = ops.attention(q, k, v, plan=True, **kw).kernel.decode()
    assert sorted({_seen[c.id] for c in A.DEFAULT_CASES}) == A.KERNELS_DEFAULT
    assert not set(A.KERNELS_SWITCH_ONLY) & set(A.KERNELS_DEFAULT)
    assert set(A.KERNELS_SWITCH_ONLY) <= {c.kernel for c in A.SWITCH_CASES}


def test_attention_error_paths():
    """every SIU3R_CHECK of the validation, through the plan query and through the launch (the query first: a block it accepted would
    be launched)"""
    from siu3r_amd import _lib

    ops = _ops()
    B, H, Nq, Nk, D = 4, 2, 65, 70, 64
    q, k, v = (torch.zeros(B, n, H, D, device="cuda") for n in (Nq, Nk, Nk))
    out = torch.empty(B, Nq, H * D, device="cuda")

    def params(**fields):
        p = _lib.AttnParams()
        p.q, p.k, p.v, p.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
        p.dtype, p.split3 = _lib.F32, 1
        p.B, p.H, p.Nq, p.Nk, p.D = B, H, Nq, Nk, D
        p.q_sb, p.q_sn, p.q_sh = q.stride(0), q.stride(1), q.stride(2)
        p.k_sb, p.k_sn, p.k_sh = k.stride(0), k.stride(1), k.stride(2)
        p.v_sb, p.v_sn, p.v_sh = v.stride(0), v.stride(1), v.stride(2)
        p.scale = D ** -0.5
        for f, val in fields.items():
            setattr(p, f, val)
        return p

    def plan(p):
        pl = _lib.AttnPlan()
        _lib.check(_lib.lib().siu3r_attention_plan(C.byref(p), C.byref(pl)))
        return pl

    assert plan(params()).kernel.decode() == "siu3r_attn_pipe::attn_pipe_kernel<true, false>"
    error_paths(params, plan)
    error_paths(params, lambda p: _lib.check(_lib.lib().siu3r_attention(C.byref(p), torch.cuda.current_stream().cuda_stream)))
    # and through the Python surface
    q48 = torch.zeros(1, 8, 2, 48, device="cuda")
    for kw in (dict(plan=True), dict()):
        with pytest.raises(RuntimeError, match="head_dim 48 unsupported"):
            ops.attention(q48, q48, q48, heads=2, head_dim=48, scale=1.0, **kw)
        with pytest.raises(RuntimeError, match="kv_x3"):
            ops.attention(q[:, :, :, :], k[:, :40], v[:, :40], heads=H, head_dim=D, scale=1.0, split3=True, kv_planes=True, **kw)
    assert ops.attention_plan(q, k, v, heads=H, head_dim=D, scale=1.0, split3=True).queries_per_wg == 128
