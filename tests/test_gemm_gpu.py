"""Every dispatch branch and epilogue of siu3r_gemm against the float64 reference, element by element (tests/dense_gemm64.py holds the
reference, the metric, the generator, the buffer placement and the case list; tests/test_gemm_ref.py shows on the CPU that the metric
rejects every kind of wrong answer at every case shape and that the reference is what float64 torch computes).

Every case builds its device tensors as views inside larger parents -- row stride beyond n (k), spare rows behind M, a spare batch
slot, bases offset as the case says; output parents NaN-filled, A's parent NaN outside the rows except A[m, k .. kpad), which holds a
large finite value (dense_gemm64's header says why) -- asks siu3r_gemm_plan which kernel will run and asserts kernel name, tile,
split-K slices, remainder rows and their path, a_x3_ok and c_x3_ok, launches once (split-K: twice on the stream, the second launch
finds the tickets reset), holds every output element to |out - ref| <= bound * S and every parent element outside the views to its
fill bit pattern."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_gemm64 as G  # noqa: E402
import test_gemm_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_seen = {}   # case id -> (kernel, skinny key)
_ws = {}


def _lib():
    from siu3r_amd import _lib

    return _lib


def _workspace():
    """one split-K workspace for the whole session: the counters are zeroed ONCE (the tickets reset themselves)"""
    if not _ws:
        _ws["ws"] = torch.empty(G.WS_FLOATS, dtype=torch.float32, device="cuda")
        _ws["cnt"] = torch.zeros(G.WS_COUNTERS, dtype=torch.int32, device="cuda")
    return _ws["ws"], _ws["cnt"]


def _nan_bits(dt):
    return int(torch.full((1,), float("nan"), dtype=dt).view(torch.int16 if dt == torch.bfloat16 else torch.int32).item())


class Buffers:
    """the device tensors of a case: parents (flat, NaN-filled) and the views inside them"""

    def __init__(self):
        self.parents = {}   # name -> (parent, view)
        self.plain = {}     # name -> contiguous tensor

    def strided(self, name, numel, off, shape, stride, dt, data=None):
        parent = torch.full((numel,), float("nan"), dtype=dt, device="cuda")
        assert parent.data_ptr() % 128 == 0
        view = parent.as_strided(shape, stride, off)
        if data is not None:
            view.copy_(data.to(dt))
        self.parents[name] = (parent, view)
        return view

    def rows(self, name, lay, dt, data=None):
        assert dt.itemsize == lay.esz, (name, dt, lay.esz)
        return self.strided(name, lay.numel, lay.off, (lay.Z, lay.M, lay.cols), (lay.sz, lay.ld, 1), dt, data)

    def flat(self, name, shape, dt, off_bytes=0, data=None):
        n = 1
        for s in shape:
            n *= s
        off = (128 + off_bytes) // dt.itemsize
        st, acc = [], 1
        for s in reversed(shape):
            st.insert(0, acc)
            acc *= s
        return self.strided(name, off + n + 64, off, tuple(shape), tuple(st), dt, data)

    def put(self, name, t):
        self.plain[name] = t.contiguous().cuda()
        return self.plain[name]

    def ptr(self, name):
        if name in self.parents:
            return self.parents[name][1].data_ptr()
        if name in self.plain:
            return self.plain[name].data_ptr()
        return None

    def assert_outside_untouched(self, cid):
        for name, (parent, view) in self.parents.items():
            it = torch.int16 if parent.dtype == torch.bfloat16 else torch.int32
            inside = torch.zeros(parent.numel(), dtype=torch.bool, device="cuda")
            inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
            if name == "a" and hasattr(self, "a_tail"):
                inside.as_strided(self.a_tail.shape, self.a_tail.stride(), self.a_tail.storage_offset()).fill_(True)
            bad = G.untouched(parent.view(it), _nan_bits(parent.dtype), inside)
            assert not bad, f"{cid}: `{name}` was written outside its view at flat elements {bad} (view offset {view.storage_offset()}, strides {view.stride()})"


def build(c, inp):
    b = Buffers()
    L = G.layouts(c)
    a_dt = torch.bfloat16 if c.mode == "bf16" else torch.float32
    if c.a_mode == 0:
        A = inp["A"]
        if c.a_x3:
            A = G.split_planes(A)
        b.rows("a", L["a"], a_dt, A)
        lay = L["a"]
        tail = min(c.kpad, lay.ld) - c.k
        if tail > 0:  # A[m, k .. kpad) may be fetched (times W's zero padding): finite
            parent = b.parents["a"][0]
            b.a_tail = parent.as_strided((lay.Z, lay.M, tail), (lay.sz, lay.ld, 1), lay.off + c.k)
            b.a_tail.fill_(G.A_TAIL_FILL)
    else:
        img = inp["img"]
        if c.a_x3:
            img = G.split_planes(img)
        b.flat("a", img.shape, a_dt, 0 if c.a_x3 else 16, img)
    wn = c.wn
    b.put("w_hi", inp["w_hi"].to(torch.bfloat16))
    if c.mode == "bf16x3":
        lo = inp["w_lo"].to(torch.bfloat16)
        b.put("w_lo", lo)
        hi = inp["w_hi"].to(torch.bfloat16)
        b.put("w_x3", torch.stack((hi.view(wn, c.n, c.kpad // 32, 32), lo.view(wn, c.n, c.kpad // 32, 32)), dim=3))
    c_dt = torch.bfloat16 if c.c_bf16 else torch.float32
    if c.shuffle:
        up, co = c.shuffle
        B, ih, iw = c.smap
        b.flat("c", (B, ih * up, iw * up, co), c_dt)
        if c.res:
            b.flat("r", (B, ih * up, iw * up, co), torch.bfloat16 if c.res == "bf16" else torch.float32, 0, G.shuffle_out(c, inp["residual"]))
    else:
        b.rows("c", L["c"], c_dt)
        if c.res:
            b.rows("r", L["r"], torch.bfloat16 if c.res == "bf16" else torch.float32, inp["residual"])
        if c.aux:
            b.rows("aux", L["aux"], torch.bfloat16)
        if "x3" in L:
            b.rows("x3", L["x3"], torch.float32)
    if c.ln:
        b.put("c1", inp["ln_c1"])
        b.put("c2", inp["ln_c2"])
        T = (c.k + 63) // 64
        rows = 2 * (c.m + 3)
        b.strided("ln_part", 32 + (c.Z + 1) * rows * T * 2 + 64, 32, (c.Z, c.m, T, 2), (rows * T * 2, 2 * T * 2, 2, 1), torch.float32, inp["ln_part"])
    elif c.bias:
        b.put("bias", inp["bias"])
    if c.stats:
        T = (c.n + 63) // 64
        rows = 2 * (c.m + 3)
        b.strided("stats", 32 + (c.Z + 1) * rows * T * 2 + 64, 32, (c.Z, c.m, T, 2), (rows * T * 2, 2 * T * 2, 2, 1), torch.float32)
    if c.rope:
        b.put("cos", inp["rope_cos"])
        b.put("sin", inp["rope_sin"])
        b.put("pos", inp["rope_pos"])
    if c.up_src:
        b.flat("up", inp["up"].shape, torch.bfloat16 if c.up_src == "bf16" else torch.float32, 0, inp["up"])
    ws, cnt = _workspace()
    b.plain["ws"], b.plain["cnt"] = ws, cnt
    return b


def _record(cid, kernel, worst):
    path = os.environ.get("SIU3R_GEMM_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(id=cid, kernel=kernel, worst_ratio=round(worst, 4))) + "\n")


def run_case(c, inp=None):
    """plan, launch, compare; returns (fp32 output [Z, M, N] or None, statistics [Z, M, T, 2] or None) as read back"""
    _lib_ = _lib()
    lib = _lib_.lib()
    inp = inp if inp is not None else G.make_inputs(c)
    ref = G.reference(c, inp)
    b = build(c, inp)
    p, pl = TR.query_plan(c, b.ptr)
    _seen[c.id] = TR.assert_plan(c, pl)
    kernel = pl.kernel.decode()
    tune = {3: 1, **c.tune}
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for k, v in tune.items():
            _lib_.check(lib.siu3r_gemm_tune(k, v))
        for _ in range(2 if c.splitk > 1 else 1):
            _lib_.check(lib.siu3r_gemm(C.byref(p), stream))
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "launch failed" in str(e) or "HIP error" in str(e) or "illegal memory" in str(e):
            pytest.exit(f"{c.id} ({kernel}): the GPU reported {e}: nothing further is launched", returncode=3)  # a faulted device runs no more cases
        raise
    finally:
        for k in tune:
            lib.siu3r_gemm_tune(k, 0)
    if c.splitk > 1:
        assert int(b.plain["cnt"].abs().max()) == 0, f"{c.id}: the split-K tickets did not reset themselves"
    bnd, name = G.bound(c), f"{c.id} {kernel}" + (f" +skinny_path {pl.skinny_path}" if pl.skinny_path else "")
    worst, out32 = 0.0, None
    cbuf = b.parents["c"][1].float().cpu()
    if c.shuffle:
        cbuf = G.unshuffle_out(c, cbuf)
    col0, kind = c.planes if c.planes else (c.n, None)
    ncmp = c.n if kind in (None, "sep") else (col0 if kind == "same" else 0)  # columns that hold the fp32 (or bf16) output
    if ncmp:
        extra = G.bf16_extra(ref["out"], ref["S"], bnd)[..., :ncmp] if c.c_bf16 else None
        worst = G.assert_elems_close(cbuf[..., :ncmp], ref["out"][..., :ncmp], ref["S"][..., :ncmp], bnd, extra=extra, name=name)
        out32 = cbuf
    if c.aux:
        aux = b.parents["aux"][1].float().cpu()
        worst = max(worst, G.assert_elems_close(aux, ref["out"], ref["S"], bnd, extra=G.bf16_extra(ref["out"], ref["S"], bnd), name=name, what="c_aux"))
        if not c.c_bf16:
            assert torch.equal(aux, G.rne_bf16(cbuf)), f"{c.id}: c_aux is not the bf16 rounding of c"
    if c.planes:
        pbuf = (b.parents["c"][1] if kind == "same" else b.parents["x3"][1]).cpu()
        worst = max(worst, G.check_planes(pbuf, col0, c32=cbuf if kind == "sep" else None, ref=ref["out"], S=ref["S"], bnd=bnd, name=name))
        if kind == "sep" and col0:
            assert torch.isnan(pbuf[..., :col0]).all(), f"{c.id}: planes were written in front of c_x3_col0"
        if kind == "only":
            assert torch.isnan(b.parents["c"][0]).all(), f"{c.id}: the fp32 output was written although c is NULL"
    stats = None
    if c.stats:
        stats = b.parents["stats"][1].cpu()
        worst = max(worst, G.assert_elems_close(stats, ref["stats"], ref["stats_S"], bnd, name=name, what="stats_out"))
    b.assert_outside_untouched(c.id)
    _record(c.id, kernel, worst)
    return out32, stats


@pytest.mark.parametrize("c", G.DEFAULT_CASES, ids=[c.id for c in G.DEFAULT_CASES])
def test_gemm_case(c):
    run_case(c)


def test_stats_out_feeds_the_folded_layernorm():
    """a GEMM writes its rows and their statistics; the next one folds the LayerNorm of those rows from them (per family: the ping-pong
    and the 128 x 64 epilogues write and merge the partials separately)"""
    for (tile, kp, kc) in ((3, G.k_pp(True, 3), G.k_pp(True, 3, lnf=True)), (-1, G.k_dmax(), G.k_dmax(lnf=True))):
        for n in (72, 64):
            prod = G.Case(f"chain-producer-{tile}-n{n}", "bf16x3", 161, n, 72, kp, tile, stats=True, res="f32", act=1)
            rows, part = run_case(prod)
            cons = G.Case(f"chain-consumer-{tile}-k{n}", "bf16x3", 161, 200, n, kc, tile, ln=True)
            run_case(cons, G.make_inputs(cons, chain=(rows, part)))


def run_switch_cases(env):
    """(child process, the switches set in its environment)"""
    for c in G.SWITCH_CASES:
        if c.env == env:
            run_case(c)
    print(f"SWITCH_CASES_OK {env} " + " | ".join(sorted({f"{k} {s}" for k, s in _seen.values()})))


@pytest.mark.parametrize("env", G.SWITCHES)
def test_gemm_switch_only_instantiations(env):
    """the A/B switches are read when the library is first used: one child process per switch setting, one at a time, each under its
    own timeout; a child that exits non-zero or dies fails the test and nothing further is launched in it"""
    code = f"import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests'); import test_gemm_gpu as T; T.run_switch_cases('{env}')"
    sets = dict(kv.split("=") for kv in env.split(","))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **sets), capture_output=True, text=True, timeout=300)
    print(out.stdout[-8000:])
    marker = [l for l in out.stdout.splitlines() if l.startswith(f"SWITCH_CASES_OK {env} ")]
    assert out.returncode == 0 and marker, out.stdout[-3000:] + out.stderr[-3000:]
    want = {f"{c.kernel} {G.plan_key(c.kernel, c.path, c.x3, c.ln)[1]}" for c in G.SWITCH_CASES if c.env == env}
    assert set(marker[0][len(f"SWITCH_CASES_OK {env} "):].split(" | ")) == want


def test_every_default_kernel_has_a_case():
    """The kernels siu3r_gemm can launch without a switch (G.KERNELS_DEFAULT, written out by hand from the launch code) are exactly the
    plan names of the parametrised cases, and the remainder-row paths are G.SKINNY_DEFAULT.  (Cases that did not run in this session
    are asked for their plan now, on the real placement; nothing is launched.)"""
    for c in G.DEFAULT_CASES:
        if c.id not in _seen:
            b = build(c, G.make_inputs(c))
            _seen[c.id] = TR.assert_plan(c, TR.query_plan(c, b.ptr)[1])
    keys = [_seen[c.id] for c in G.DEFAULT_CASES]
    seen = sorted({k for k, _ in keys})
    assert seen == G.KERNELS_DEFAULT, f"without a case: {sorted(set(G.KERNELS_DEFAULT) - set(seen))}; not in the list: {sorted(set(seen) - set(G.KERNELS_DEFAULT))}"
    assert sorted({s for _, s in keys if s}) == G.SKINNY_DEFAULT


def test_gemm_error_paths():
    """every SIU3R_CHECK of the validation through the plan query, then through the launch (the query first: a block it accepted would
    be launched); siu3r_gemm's own checks; the Python surface"""
    _lib_ = _lib()
    from siu3r_amd import ops

    def plan(p):
        pl = _lib_.GemmPlan()
        _lib_.check(_lib_.lib().siu3r_gemm_plan(C.byref(p), C.byref(pl)))
        return pl

    launch = lambda p: _lib_.check(_lib_.lib().siu3r_gemm(C.byref(p), torch.cuda.current_stream().cuda_stream))
    params = lambda **f: TR.error_params(_lib_, **f)
    TR.error_paths(params, plan)
    TR.error_paths(params, launch)
    TR.error_paths(params, launch, launch=True)
    w = ops.pack_linear(torch.randn(64, 64, device="cuda"), None, True)
    x = torch.randn(128, 64, device="cuda")
    with pytest.raises(RuntimeError, match="bf16x3 weights need fp32 activations"):
        ops.linear(x.bfloat16(), w)
    with pytest.raises(RuntimeError, match="split-K needs a workspace.*splitk=4"):
        ops.linear(x, w, splitk=4)
    assert ops.linear(x, w, dry_run=True).skinny_path == 0
