"""CPU checks of tests/dense_rowchain64.py and of the host side of siu3r_rowchain_x3: the float64 restatement against a plain fp32 torch
composition (F.linear, F.layer_norm, relu) stage by stage at M = 5, H = 256, each stage evaluated from the restatement's own stage
input so that the bound of that stage applies; the round trip of ops.pack_rowchain; the refusals of ops.rowchain_ok."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_rowchain64 as R  # noqa: E402

from siu3r_amd import ops  # noqa: E402

M, H = 5, 256


def _pack(w):
    return ops.pack_rowchain(w["wo"], w["bo"], w["g1"], w["b1"], w["w1"], w["c1"], w["w2"], w["c2"], w["g2"], w["b2"])


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_against_fp32_torch(kind):
    w = R.make_weights(H, kind)
    x, res = R.make_rows(M, kind)
    u = ops.unpack_rowchain(_pack(w), H)
    ref = R.chain64(x, res, u)
    f = lambda t: t.float()
    # the fp32 composition multiplies the fp32 weights, the restatement hi + lo: |w - (hi + lo)| <= 2^-17 |w|, inside X3_TERM's lo roundings
    stages = [
        ("y", F.linear(x, w["wo"], w["bo"]) + res, ref["y"], R.product_bound(256) * ref["S_y"]),
        ("z", F.layer_norm(f(ref["y"]), (R.D,), w["g1"], w["b1"], 1e-5), ref["z"], R.LN_TERM * R.ln_scale(ref["y"], w["g1"], w["b1"], 1e-5)),
        ("h", torch.relu(F.linear(f(ref["z"]), w["w1"], w["c1"])), ref["h"], R.product_bound(256) * ref["S_h"]),
        ("o", F.linear(f(ref["h"]), w["w2"], w["c2"]) + f(ref["z"]), ref["o"], R.product_bound(H) * ref["S_o"]),
        ("out", F.layer_norm(f(ref["o"]), (R.D,), w["g2"], w["b2"], 1e-5), ref["out"], R.LN_TERM * R.ln_scale(ref["o"], w["g2"], w["b2"], 1e-5)),
    ]
    for name, got, want, bnd in stages:
        ratio = ((got.double() - want).abs() / bnd).max().item()
        print(f"[rowchain-ref] {kind} {name}: worst {ratio:.3f} of the bound")
        assert ratio <= 1.0, (kind, name, ratio)
    # and the whole chain in fp32 torch lands on the restatement's output (a wrong stage order or a dropped residual is of order 1)
    z = F.layer_norm(F.linear(x, w["wo"], w["bo"]) + res, (R.D,), w["g1"], w["b1"], 1e-5)
    out = F.layer_norm(F.linear(torch.relu(F.linear(z, w["w1"], w["c1"])), w["w2"], w["c2"]) + z, (R.D,), w["g2"], w["b2"], 1e-5)
    assert R.row_error(out, ref["out"]).max().item() < 1e-3


def test_one_pass_variance_is_caught_by_the_offset_rows():
    """the fp32 chain with E[v^2] - E[v]^2 LayerNorms fails the GPU module's parity inequality against the two-pass fp32 chain on the
    rows of mean 50 and deviation 0.5: that input set does what it is there for"""
    w = R.make_weights(H, "offset")
    x, res = R.make_rows(33, "offset")
    ref = R.chain64(x, res, ops.unpack_rowchain(_pack(w), H))["out"]

    def ln(v, g, b, one_pass):
        mean = v.mean(-1, keepdim=True)
        var = (v * v).mean(-1, keepdim=True) - mean * mean if one_pass else ((v - mean) ** 2).mean(-1, keepdim=True)
        return (v - mean) * torch.rsqrt(var + 1e-5) * g + b

    def chain(one_pass):
        z = ln(F.linear(x, w["wo"], w["bo"]) + res, w["g1"], w["b1"], one_pass)
        return ln(F.linear(torch.relu(F.linear(z, w["w1"], w["c1"])), w["w2"], w["c2"]) + z, w["g2"], w["b2"], one_pass)

    e1, e2 = R.row_error(chain(True), ref), R.row_error(chain(False), ref)
    print(f"[rowchain-ref] one-pass variance: worst row {e1.max().item():.3e}, two-pass {e2.max().item():.3e}")
    assert (e1 > 2 * e2 + R.PARITY_ADD).any()


@pytest.mark.parametrize("H_", R.HS)
def test_pack_round_trips(H_):
    w = R.make_weights(H_, "normal")
    pack = _pack(w)
    assert pack.dtype == torch.uint8 and pack.numel() == (256 * 256 + 2 * H_ * 256) * 4 + (6 * 256 + H_) * 4
    u = ops.unpack_rowchain(pack, H_)
    for k in ("wo", "w1", "w2"):
        hi = w[k].to(torch.bfloat16)
        lo = (w[k] - hi.float()).to(torch.bfloat16)
        assert torch.equal(u[k], hi.double() + lo.double()), k
        assert ((u[k] - w[k].double()).abs() <= 2.0 ** -17 * w[k].double().abs() + 1e-40).all(), k
    for k in ("bo", "g1", "b1", "c1", "c2", "g2", "b2"):
        assert torch.equal(u[k], w[k]), k
    # the fragment layout of siu3r_proj_rows_x3: block nb, K step s, plane, lane = 32 (k % 16 / 8) + n % 32, 8 consecutive k
    fr = pack[:256 * 256 * 4].view(torch.bfloat16).reshape(8, 16, 2, 64, 8)
    for (n, k) in ((0, 0), (37, 9), (255, 255), (100, 136)):
        assert fr[n // 32, k // 16, 0, 32 * ((k % 16) // 8) + n % 32, k % 8] == w["wo"][n, k].to(torch.bfloat16)


def test_pack_refuses_a_hidden_width_that_is_no_multiple_of_256():
    w = R.make_weights(256, "normal")
    w["w1"], w["c1"], w["w2"] = w["w1"][:128], w["c1"][:128], w["w2"][:, :128]
    with pytest.raises(AssertionError):
        _pack(w)


def test_rowchain_ok_refusals():
    x, res = torch.zeros(2, 7, 256), torch.zeros(2, 7, 256)
    cases = [
        (x, res, True), (x, res, False), (x.double(), res, True), (x, res.to(torch.bfloat16), True), (x[:, ::2], res[:, ::2], True),
        (x[..., :128], res[..., :128], True), (torch.zeros(2, 7, 512), torch.zeros(2, 7, 512), True), (x, res[:1], True),
        (torch.zeros(256), torch.zeros(256), True), (x.transpose(0, 1), res.transpose(0, 1), True),
    ]
    for (a, b, split) in cases:
        assert ops.rowchain_ok(a, b, split) == R.rowchain_ok_restated(a, b, split), (a.shape, a.dtype, b.shape, split)
    assert ops.rowchain_ok(x, res, True) and sum(ops.rowchain_ok(*c) for c in cases) == 1


def test_rowchain_refuses_cpu_tensors():
    w = R.make_weights(256, "normal")
    with pytest.raises(RuntimeError):
        ops.rowchain_x3(torch.zeros(4, 256), torch.zeros(4, 256), _pack(w), 256, 1e-5, 1e-5)
