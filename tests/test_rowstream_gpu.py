"""siu3r_stem7x7_x3 (csrc/stem.hip) and siu3r_proj_rows_x3 (csrc/proj.hip) against the float64 restatements of
tests/dense_rowstream64.py, element by element, at the case list that file derives from the kernels' persistent tile loops: one tile per
workgroup, three tiles with a ragged last round, tiles of one workgroup in different batch items, the 256 / Z < 1 clamp
(tests/test_rowstream_ref.py shows on the CPU that the bound holds for a float32 emulation of the kernels and rejects every wrong
answer a stale prefetch, a wrong head index, a dropped product or an off-by-one corner would give).

Every case goes through ops.stem7x7_x3 / ops.proj_rows_x3.  Inputs live in NaN-filled parents; every output lives inside a parent
filled with one bit pattern, guard rows in front and behind, and everything outside the written elements -- proj's columns N .. ldc - 1
and the gap between z slots included -- must keep that pattern.  Every launch is repeated on the same buffers and must give identical
bits (no atomics: a difference is a race in the tile loop).  The stem's planes must equal split_planes(fp32 output) bitwise.
SIU3R_ROWSTREAM_PARITY_LOG=<file> appends one JSON line per case (profiles/rowstream_parity.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_rowstream64 as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096   # canary elements in front of and behind every output


def _ops():
    from siu3r_amd import ops

    return ops


def _lib():
    from siu3r_amd import _lib

    return _lib


def _record(c, grid, per, worst):
    path = os.environ.get("SIU3R_ROWSTREAM_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(id=c.id, grid=list(grid), tiles=c.ntiles, tiles_per_wg=[max(per), min(per)], ragged_round=c.ntiles % c.nwg != 0,
                                     worst_ratio=round(worst, 4))) + "\n")


def _guarded(t):
    """a contiguous device copy of t inside a NaN-filled parent"""
    parent = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    view = parent[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


class Canary:
    """an fp32 output view (shape, strides, offset) inside a flat parent filled with R.FILL_BITS"""

    def __init__(self, numel, shape, stride, off):
        self.bits = torch.full((numel,), R.FILL_BITS, dtype=torch.int32, device="cuda")
        self.parent = self.bits.view(torch.float32)
        self.view = self.parent.as_strided(shape, stride, off)
        self.written = torch.zeros(numel, dtype=torch.bool, device="cuda")
        self.written.as_strided(shape, stride, off).fill_(True)

    def assert_outside_untouched(self, cid, what="out"):
        bad = R.untouched(self.bits, R.FILL_BITS, self.written)
        assert not bad, f"{cid}: `{what}` was written outside its view at flat elements {bad} (view offset {self.view.storage_offset()}, strides {self.view.stride()})"

    def assert_all_untouched(self, cid):
        bad = R.untouched(self.bits, R.FILL_BITS, torch.zeros_like(self.written))
        assert not bad, f"{cid}: a refused launch wrote flat elements {bad}"


def _launch(cid, fn):
    try:
        fn()
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "launch failed" in str(e) or "HIP error" in str(e) or "illegal memory" in str(e):
            pytest.exit(f"{cid}: the GPU reported {e}: nothing further is launched", returncode=3)  # a faulted device runs no more cases
        raise


def _twice(cid, fn, view):
    """launch, keep the bits, launch again on the same buffers: identical bits; returns the first result on the CPU"""
    _launch(cid, fn)
    first = view.clone()
    _launch(cid, fn)
    assert torch.equal(first.view(torch.int32), view.view(torch.int32)), f"{cid}: two launches on the same buffers differ (a race in the tile loop)"
    return first.cpu()


# ------------------------------------------------------------------------------------------------
# stem
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.STEM_CASES, ids=[c.id for c in R.STEM_CASES])
def test_stem_case(c):
    ops = _ops()
    per = c.check_props()
    inp = R.stem_inputs(c)
    ref = R.stem_reference(c, inp)
    wfrag, bias = ops.pack_stem7([w.cuda() for w in inp["W"]], [inp["bias"][g].cuda() if c.bias else None for g in range(c.G)])
    assert (bias is None) == (not c.bias)
    img = _guarded(inp["img"])
    up = _guarded(inp["up"]) if c.up else None
    shape = (c.B, c.G, c.H, c.W, R.STEM_C)
    n = int(np.prod(shape))
    stride = tuple(int(np.prod(shape[i + 1:])) for i in range(5))
    out, pl = Canary(n + 2 * GUARD, shape, stride, GUARD), Canary(n + 2 * GUARD, shape, stride, GUARD)
    o32 = _twice(c.id, lambda: ops.stem7x7_x3(img, wfrag, bias, up, out.view), out.view)
    planes = _twice(c.id + " (planes)", lambda: ops.stem7x7_x3(img, wfrag, bias, up, pl.view, planes=True), pl.view)
    out.assert_outside_untouched(c.id)
    pl.assert_outside_untouched(c.id, "planes")
    worst = R.assert_elems_close(o32, ref["out"], ref["S"], R.STEM_BOUND, extra=ref["extra"], name=c.id)
    want = R.split_planes(o32)
    same = planes.view(torch.int32) == want.view(torch.int32)
    assert same.all(), f"{c.id}: the planes differ from split_planes(fp32 output) at (b, g, y, x, word) = {tuple(int(i) for i in (~same).nonzero()[0])}"
    _record(c, (c.nwg, c.G), per, worst)


# ------------------------------------------------------------------------------------------------
# proj
# ------------------------------------------------------------------------------------------------
def proj_canary(c):
    first = GUARD + (1 if c.dest == "ldc85" else 0) + (c.M * c.N if c.dest == "view" else 0)   # (ldc85: a base that is 4-byte aligned only)
    numel = first + (c.Z - 1) * c.zs + c.M * c.ldc + GUARD
    if c.G > 1:
        return Canary(numel, (c.B, c.G, c.M, c.N), (c.G * c.zs, c.zs, c.ldc, 1), first)
    return Canary(numel, (c.B, 1, c.M, c.N), (c.zs, c.zs, c.ldc, 1), first)


@pytest.mark.parametrize("c", R.PROJ_CASES, ids=[c.id for c in R.PROJ_CASES])
def test_proj_case(c):
    ops = _ops()
    per = c.check_props()
    inp = R.proj_inputs(c)
    ref = R.proj_reference(c, inp)
    assert ops.proj_rows_ok(c.K, c.N)
    wf, bias, n = ops.pack_proj([w.cuda() for w in inp["W"]], [inp["bias"][g].cuda() if c.bias else None for g in range(c.G)])
    assert n == c.N and (bias is None) == (not c.bias)
    x = _guarded(inp["x"].view(c.B, c.G, c.M, c.K))
    out = proj_canary(c)
    got = _twice(c.id, lambda: ops.proj_rows_x3(x, wf, bias, n, out.view), out.view)
    out.assert_outside_untouched(c.id)
    worst = R.assert_elems_close(got.reshape(c.Z, c.M, c.N), ref["out"], ref["S"], R.proj_bound(c), name=c.id)
    _record(c, (c.nwg, c.Z), per, worst)


# ------------------------------------------------------------------------------------------------
# the packers (they refuse CPU tensors): fragments unpacked by the lane map of their docstrings
# ------------------------------------------------------------------------------------------------
def _unpack(fr, blocks, steps):
    """[G, blocks, steps, 2, 64, 8] -> [G, 2, 32 * blocks, 16 * steps]: lane l of (block w, step s) holds column 32 w + l % 32 and
    k = 16 s + 8 (l // 32) + 0 .. 7"""
    fr = fr.float().cpu()
    G_ = fr.shape[0]
    assert tuple(fr.shape) == (G_, blocks, steps, 2, 64, 8), fr.shape
    out = torch.full((G_, 2, 32 * blocks, 16 * steps), float("nan"))
    w, s, l, j = torch.meshgrid(torch.arange(blocks), torch.arange(steps), torch.arange(64), torch.arange(8), indexing="ij")
    out[:, :, 32 * w + l % 32, 16 * s + 8 * (l // 32) + j] = fr.permute(0, 3, 1, 2, 4, 5)
    assert not torch.isnan(out).any()
    return out


def test_pack_round_trip():
    ops = _ops()
    c = R.STEM_CASES[0]
    inp = R.stem_inputs(c)
    wfrag, bias = ops.pack_stem7([w.cuda() for w in inp["W"]], [None, inp["bias"][1].cuda()])
    got = _unpack(wfrag, 8, 14).view(c.G, 2, R.STEM_C, 7, 8, 4)                     # k = (ky, kx in 0..7, c in 0..3)
    assert not got[..., 7, :].any() and not got[..., 3].any(), "kx = 7 and c = 3 carry zero weights"
    for p, name in enumerate(("w_hi", "w_lo")):
        assert torch.equal(got[:, p, :, :, :7, :3], inp[name].permute(0, 1, 3, 4, 2)), name
    assert torch.equal(got.double().sum(1)[..., :7, :3], (inp["w_hi"].double() + inp["w_lo"].double()).permute(0, 1, 3, 4, 2))
    assert torch.equal(bias.cpu(), torch.stack((torch.zeros(R.STEM_C), inp["bias"][1])))
    for c in R.PROJ_CASES:
        if "single" not in c.props or c.M != 1:
            continue
        inp = R.proj_inputs(c)
        wf, bias, n = ops.pack_proj([w.cuda() for w in inp["W"]], [None, inp["bias"][1].cuda()])
        nb = (c.N + 31) // 32
        got = _unpack(wf, nb, c.K // 16)
        assert n == c.N and not got[:, :, c.N:].any(), "columns >= N hold zeros"
        assert torch.equal(got[:, 0, :c.N], inp["w_hi"]) and torch.equal(got[:, 1, :c.N], inp["w_lo"]), c.id
        want = torch.zeros(c.G, 32 * nb)
        want[1, :c.N] = inp["bias"][1]
        assert torch.equal(bias.cpu(), want), c.id


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _refused(cid, rc, match, canary):
    _lib_ = _lib()
    assert rc != 0, f"{cid}: accepted"
    msg = _lib_.lib().siu3r_last_error().decode()
    with pytest.raises(RuntimeError, match=match) as e:
        _lib_.check(rc)
    assert msg and msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    canary.assert_all_untouched(cid)


def test_refusals():
    lib = _lib().lib()
    stream = torch.cuda.current_stream().cuda_stream
    for (H, W) in ((24, 32), (32, 40), (8, 16)):
        img = torch.zeros(1, 1, H, W, 4, device="cuda")
        wfrag = torch.zeros(1, 8, 14, 2, 64, 8, dtype=torch.bfloat16, device="cuda")
        n = H * W * R.STEM_C
        out = Canary(n + 2 * GUARD, (1, 1, H, W, R.STEM_C), (n, n, W * R.STEM_C, R.STEM_C, 1), GUARD)
        rc = lib.siu3r_stem7x7_x3(img.data_ptr(), wfrag.data_ptr(), None, None, out.view.data_ptr(), 1, 1, H, W, 0, stream)
        _refused(f"stem {H} x {W}", rc, rf"multiples of 16 \(H={H} W={W}\)", out)
    M = 70
    for (what, Z, G_, K, N, ldc, match) in (("K 256, N 64", 2, 2, 256, 64, 64, r"no instantiation for K=256 N=64"), ("K 256, N 97", 2, 2, 256, 97, 97, r"no instantiation for K=256 N=97"),
                                            ("K 128, N 33", 2, 2, 128, 33, 33, r"no instantiation for K=128 N=33"), ("K 64", 2, 2, 64, 3, 3, r"no instantiation for K=64 N=3"),
                                            ("Z % G != 0", 3, 2, 256, 83, 83, r"bad shape \(Z=3 G=2 N=83 ldc=83\)"), ("ldc < N", 2, 2, 256, 83, 80, r"bad shape \(Z=2 G=2 N=83 ldc=80\)")):
        x = torch.zeros(Z, M, K, device="cuda")
        wf = torch.zeros(2, 4, K // 16, 2, 64, 8, dtype=torch.bfloat16, device="cuda")
        n = Z * M * max(N, ldc)
        out = Canary(n + 2 * GUARD, (Z, M, N), (M * max(N, ldc), max(N, ldc), 1), GUARD)
        rc = lib.siu3r_proj_rows_x3(x.data_ptr(), wf.data_ptr(), None, out.view.data_ptr(), Z, G_, M, K, N, ldc, 0, stream)
        _refused(f"proj {what}", rc, match, out)
