"""siu3r_rowchain_x3 on the GPU against the float64 restatement of tests/dense_rowchain64.py and against the five launches it replaces
(ops.linear + residual, ops.layernorm, ops.linear + ReLU, ops.linear + residual, ops.layernorm: unchanged code) on the same inputs.

Per row, with e = max|. - ref| / max|ref| of the final output:  e_fused <= 2 e_unfused + 256 * 2^-24  (dense_rowchain64.py's header).
Every input lies inside a NaN-filled buffer, the output is carved from a sentinel-filled one (rows at M and beyond and the guard bands
must keep the sentinel), two launches must give the same bits, and a refused call writes nothing."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_rowchain64 as R  # noqa: E402

pytestmark = pytest.mark.gpu

EXTRA_ROWS = 3   # rows behind M inside the carved output: they must keep the sentinel
_layers = {}


def _layer(H, kind):
    """the packed layer on the GPU, its weights read back for the reference, and the five launches' packed weights (built once)"""
    from siu3r_amd import ops

    key = (H, kind)
    if key not in _layers:
        w = R.make_weights(H, kind)
        d = {k: v.cuda() for k, v in w.items()}
        pack = ops.pack_rowchain(d["wo"], d["bo"], d["g1"], d["b1"], d["w1"], d["c1"], d["w2"], d["c2"], d["g2"], d["b2"])
        five = dict(wo=ops.pack_matrix(d["wo"], d["bo"], True), w1=ops.pack_matrix(d["w1"], d["c1"], True), w2=ops.pack_matrix(d["w2"], d["c2"], True))
        _layers[key] = dict(w=w, d=d, pack=pack, u=ops.unpack_rowchain(pack, H), five=five)
    return _layers[key]


def _carve(t, fill_bits=R.FILL_BITS):
    """a copy of t inside a buffer of NaNs with a guard band on either side -> (view, buffer)"""
    buf = torch.full((t.numel() + 2 * R.GUARD,), fill_bits, dtype=torch.int32, device="cuda").view(torch.float32)
    v = buf[R.GUARD:R.GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def _out(M):
    buf = torch.full(((M + EXTRA_ROWS) * R.D + 2 * R.GUARD,), R.SENTINEL, dtype=torch.float32, device="cuda")
    return buf[R.GUARD:R.GUARD + M * R.D].view(M, R.D), buf


def _untouched(buf, M):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[R.GUARD:R.GUARD + M * R.D] = False
    return bool((buf[keep] == R.SENTINEL).all())


def _five(x, res, L):
    from siu3r_amd import ops

    d, f = L["d"], L["five"]
    a = ops.linear(x, f["wo"], out_dtype=torch.float32, residual=res)
    z = ops.layernorm(a, d["g1"], d["b1"], 1e-5, torch.float32)
    h = ops.linear(z, f["w1"], out_dtype=torch.float32, act=ops.ACT_RELU)
    o = ops.linear(h, f["w2"], out_dtype=torch.float32, residual=z)
    return ops.layernorm(o, d["g2"], d["b2"], 1e-5, torch.float32)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H", R.HS)
@pytest.mark.parametrize("M", R.MS)
def test_rowchain_against_float64_and_the_five_launches(M, H, kind):
    from siu3r_amd import ops

    L = _layer(H, kind)
    x, res = R.make_rows(M, kind)
    ref = R.chain64(x, res, L["u"])["out"]
    xg, _ = _carve(x.cuda())
    rg, _ = _carve(res.cuda())
    out, obuf = _out(M)
    assert ops.rowchain_x3(xg, rg, L["pack"], H, 1e-5, 1e-5, out=out) is out
    torch.cuda.synchronize()
    assert _untouched(obuf, M), "rows at M and beyond or a guard band were written"
    got = out.cpu()
    assert torch.isfinite(got).all()
    out2, obuf2 = _out(M)
    ops.rowchain_x3(xg, rg, L["pack"], H, 1e-5, 1e-5, out=out2)
    assert torch.equal(out2, out) and _untouched(obuf2, M)

    unfused = _five(xg, rg, L).cpu()
    e_f, e_u = R.row_error(got, ref), R.row_error(unfused, ref)
    slack = (e_f - (2 * e_u + R.PARITY_ADD))
    i = int(slack.argmax())
    print(f"[parity] M={M} H={H} {kind}: fused worst {e_f.max().item():.3e}, five launches worst {e_u.max().item():.3e}; "
          f"tightest row {i}: fused {e_f[i].item():.3e} against 2 x {e_u[i].item():.3e} + {R.PARITY_ADD:.3e}")
    assert (slack <= 0).all(), f"row {i}: e_fused {e_f[i].item():.3e} > 2 x {e_u[i].item():.3e} + {R.PARITY_ADD:.3e}"


def test_bit_identical_to_the_five_launches_at_the_networks_shape():
    """M = 10752, H = 1024: the five launches run on the ping-pong GEMM there, whose K order, product order per K step (hi x hi,
    hi x lo, lo x hi) and epilogue order (bias, activation, residual) the kernel keeps, and on layernorm_kernel, whose sums it keeps:
    the switch SIU3R_NO_ROWCHAIN changes no bit of the model's outputs at the benchmarked shape"""
    from siu3r_amd import ops

    L = _layer(1024, "normal")
    x, res = (t.cuda() for t in R.make_rows(10752, "normal"))
    assert torch.equal(ops.rowchain_x3(x, res, L["pack"], 1024, 1e-5, 1e-5), _five(x, res, L))


def test_leading_dimensions_fold_into_rows():
    """[2, 40, 256] is 80 rows: the model's [N2, S, 256] call"""
    from siu3r_amd import ops

    L = _layer(256, "normal")
    x, res = R.make_rows(80, "normal")
    a = ops.rowchain_x3(x.cuda().view(2, 40, 256), res.cuda().view(2, 40, 256), L["pack"], 256, 1e-5, 1e-5)
    b = ops.rowchain_x3(x.cuda(), res.cuda(), L["pack"], 256, 1e-5, 1e-5)
    assert a.shape == (2, 40, 256) and torch.equal(a.view(80, 256), b)
    assert ops.rowchain_x3(x.cuda()[:0], res.cuda()[:0], L["pack"], 256, 1e-5, 1e-5).shape == (0, 256)   # an empty M launches nothing


def test_refused_calls_write_nothing():
    from siu3r_amd import _lib

    L = _layer(256, "normal")
    x, res = (t.cuda() for t in R.make_rows(4, "normal"))
    out, obuf = _out(4)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    bad = [
        (None, p(res), p(L["pack"]), p(out), 4, 256), (p(x), None, p(L["pack"]), p(out), 4, 256), (p(x), p(res), None, p(out), 4, 256),
        (p(x), p(res), p(L["pack"]), None, 4, 256), (p(x), p(res), p(L["pack"]), p(out), 0, 256), (p(x), p(res), p(L["pack"]), p(out), -3, 256),
        (p(x), p(res), p(L["pack"]), p(out), 4, 0), (p(x), p(res), p(L["pack"]), p(out), 4, 128), (p(x), p(res), p(L["pack"]), p(out), 4, 384),
        (p(x) + 4, p(res), p(L["pack"]), p(out), 4, 256), (p(x), p(res) + 8, p(L["pack"]), p(out), 4, 256),
        (p(x), p(res), p(L["pack"]) + 2, p(out), 4, 256), (p(x), p(res), p(L["pack"]), p(out) + 4, 4, 256),
    ]
    for (a, b, c, d, M, H) in bad:
        assert lib.siu3r_rowchain_x3(a, b, c, d, M, H, 1e-5, 1e-5, st) != 0, (M, H)
        assert b"rowchain_x3" in lib.siu3r_last_error()
    torch.cuda.synchronize()
    assert bool((obuf == R.SENTINEL).all())
