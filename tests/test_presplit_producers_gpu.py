"""Producer kernels that are not GEMMs write their result as PRE-SPLIT planes (ops.Planes: per row and 32 columns a 128-byte line
[hi 32 | lo 32] bf16, hi = the upper 16 bits, lo = bf16(value - hi)) when a bf16x3 GEMM is the only reader: the pipelined attention
kernel (siu3r_attn_params.out_x3), resize_kernel, msdeform_kernel<L, 4> and dwconv_gelu_kernel (siu3r_*_planes).

Per producer, at the smallest shapes that reach each of its store paths:
  1. the planes are, bit for bit, the host split of the fp32 result of the same kernel on the same input; the destination is carved
     out of a sentinel-filled buffer whose guard bands stay intact, and the fp32 destination of a planes-only call stays untouched;
  2. the consumer does not care: ops.linear / ops.conv2d on the planes give the bits they give on the fp32 tensor -- and the plan log
     shows that the pre-split instantiation (7th template argument of gemm_pp_kernel) really ran;
  3. a row width that is a multiple of 4 but not of 32 falls back to fp32 through the wrapper, is refused (non-zero return, nothing
     written) at the C entry point, and an empty input returns 0.
One model forward at 64 x 96 gives the same bits with and without pre-split operands."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN pattern no kernel here produces
GUARD = 64  # floats on either side of a destination (keeps it 128-byte aligned)


def _ops():
    from siu3r_amd import ops

    return ops


def _split_planes(x):
    """fp32 [..., C] (C % 32 == 0) -> the same shape holding the planes of every row: the torch emulation of the split"""
    x = x.contiguous()
    Cc = x.shape[-1]
    assert Cc % 32 == 0
    bits = x.view(torch.int32)
    hi = (bits >> 16).to(torch.int16)
    lo = (x - (bits & -65536).view(torch.float32)).to(torch.bfloat16).view(torch.int16)
    return torch.stack((hi.reshape(-1, Cc // 32, 32), lo.reshape(-1, Cc // 32, 32)), dim=2).reshape(-1, 2 * Cc).view(torch.float32).reshape(x.shape)


class _Guarded:
    """a contiguous fp32 destination of `shape` carved out of a sentinel-filled buffer"""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        assert self.t.data_ptr() % 128 == 0

    def guards_intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENTINEL).all())


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_planes(run, ref):
    """run(out, planes_out) launches the producer with planes_only=True; ref: its fp32 result.  Checks (1) of the module docstring and
    returns the planes (ops.Planes whose storage is the guarded destination)."""
    ops = _ops()
    dst, f32 = _Guarded(tuple(ref.shape)), _Guarded(tuple(ref.shape))
    P = ops.Planes(ref, storage=dst.t)
    run(f32.t, P)
    torch.cuda.synchronize()
    assert P.valid and P.only, "the producer did not take its planes form"
    assert _bits_equal(dst.t, _split_planes(ref)), "planes differ from the host split of the fp32 result"
    assert dst.guards_intact(), "a plane store left its destination"
    assert f32.untouched(), "planes_only: the fp32 destination was written"
    P._keep = dst
    return P


@pytest.fixture(scope="module")
def pingpong():
    """small consumers on the 128 x 128 ping-pong tile (the kernels that read pre-split A), whatever the cost model would pick"""
    ops = _ops()
    ops.gemm_tune(0, 3)
    yield
    ops.gemm_tune(0, 0)


def _presplit_a(pl):
    k = pl.kernel
    return b"gemm_pp_kernel<true" in k and k.count(b",") == 6 and k.endswith(b", true>")


def _consumer_same_bits(ref, P, seed):
    """(2) of the module docstring.  ref / P.t: [..., C]; rows >= 128 and C % 64 == 0: a Linear (whole 64-deep K tiles), else a 3 x 3
    convolution over the rows as a [rows, 1] map, or over the map itself for a 4-d tensor."""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    Cc = ref.shape[-1]
    rows = ref.numel() // Cc
    log = []
    ops.set_plan_log(log)
    try:
        if ref.dim() == 4 or rows < 128 or Cc % 64:
            xm = ref if ref.dim() == 4 else ref.reshape(1, rows, 1, Cc)
            pm = ops.Planes(xm, storage=P.t.view(xm.shape))
            pm.valid, pm.only = P.valid, P.only
            pw = ops.pack_conv((torch.randn(64, Cc, 3, 3, generator=g) / (3 * Cc ** 0.5)).cuda(), torch.randn(64, generator=g).cuda(), True)
            a = ops.conv2d(xm, pw, pad=1)
            b = ops.conv2d(pm.t, pw, pad=1, a_planes=pm)
        else:
            pw = ops.pack_linear((torch.randn(64, Cc, generator=g) / Cc ** 0.5).cuda(), torch.randn(64, generator=g).cuda(), True)
            a = ops.linear(ref, pw)
            b = ops.linear(P.t, pw, a_planes=P)
        torch.cuda.synchronize()
    finally:
        ops.set_plan_log(None)
    assert len(log) == 2 and not _presplit_a(log[0]) and _presplit_a(log[1]), [pl.kernel for pl in log]
    assert torch.isfinite(a).all() and _bits_equal(a, b), "the consumer's result depends on the operand form"


# ------------------------------------------------------------------------------------------------ attention
def _attn_inputs(heads, Nq, Nk, kvp, seed):
    g = torch.Generator().manual_seed(seed)
    B = 2
    q = torch.randn(B, Nq, heads, 64, generator=g).cuda()
    kv = torch.randn(B, Nk, 2, heads, 64, generator=g).cuda()
    if kvp:
        kv = _split_planes(kv.view(B, Nk, -1)).view(B, Nk, 2, heads, 64)
    return q, kv[:, :, 0], kv[:, :, 1]


@pytest.mark.parametrize("Nq", [128, 129, 130, 257])
@pytest.mark.parametrize("heads", [1, 2])
def test_attention_planes(heads, Nq, pingpong):
    """attn_pipe_kernel<true, KVP>: the 128-query body and the merge of the two key halves (every Nq), a ragged last body (130), the side
    path alone in its role (129) and behind two bodies (257); ragged and whole key tiles; K / V of the other batch item; K / V fp32 and
    pre-split."""
    ops = _ops()
    first = None
    for Nk in (64, 65, 129):
        for bxor in (0, 1):
            for kvp in (False, True):
                q, k, v = _attn_inputs(heads, Nq, Nk, kvp, 1000 * Nq + 10 * Nk + bxor)
                kw = dict(heads=heads, head_dim=64, scale=0.125, split3=True, kv_bxor=bxor, kv_planes=kvp)
                pl = ops.attention_plan(q, k, v, **kw)
                assert pl.kernel.decode() == f"siu3r_attn_pipe::attn_pipe_kernel<true, {'true' if kvp else 'false'}>", pl.kernel
                assert pl.side_path == int(Nq > 128 and Nq % 128 == 1)
                ref = ops.attention(q, k, v, **kw)
                P = _check_planes(lambda out, planes: ops.attention(q, k, v, out=out, planes_out=planes, planes_only=True, **kw), ref)
                if first is None:
                    first = (ref, P)
    _consumer_same_bits(*first, seed=heads * 1000 + Nq)


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("Cc", [32, 64])
def test_resize_planes(Cc, align, pingpong):
    ops = _ops()
    g = torch.Generator().manual_seed(Cc + int(align))
    for (ih, iw), (oh, ow) in (((1, 1), (2, 2)), ((3, 5), (6, 10))):
        seq = torch.randn(2, ih * iw + 7, Cc, generator=g).cuda()
        x = seq[:, 3:3 + ih * iw].view(2, ih, iw, Cc)  # batch items dense but further apart
        assert not x.is_contiguous()
        ref = ops.resize_bilinear(x, (oh, ow), align)
        P = _check_planes(lambda out, planes: ops.resize_bilinear(x, (oh, ow), align, out=out, planes_out=planes, planes_only=True), ref)
    _consumer_same_bits(ref, P, seed=Cc)


# ------------------------------------------------------------------------------------------------ deformable sampling
@pytest.mark.parametrize("heads,d", [(2, 16), (8, 4), (4, 16), (1, 64)], ids=["32=2x16", "32=8x4", "64=4x16", "64=1x64"])
@pytest.mark.parametrize("shapes", [[(4, 5)], [(4, 6), (2, 3), (1, 2)]], ids=["L1", "L3"])
def test_msdeform_planes(shapes, heads, d, pingpong):
    """msdeform_kernel<1, 4> / <3, 4>; d % 8 == 0 (a lane pair inside one head, queries-per-workgroup order) and d = 4 (the flat order)"""
    ops = _ops()
    g = torch.Generator().manual_seed(heads * 100 + d + len(shapes))
    B, Q, L = 2, 12, len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, heads * d, generator=g).cuda()
    offs = torch.randn(B, Q, heads, L, 4, 2, generator=g) * 3.0  # several texels wide: many corners leave the map
    logit = torch.randn(B, Q, heads, L, 4, generator=g)
    offs_aw = torch.cat((offs.reshape(B, Q, -1), logit.reshape(B, Q, -1)), dim=2).contiguous().cuda()
    ref_pts = torch.rand(Q, L, 2, generator=g)
    ref_pts[0], ref_pts[1] = 0.0, 1.0  # the map's corners
    ref_pts = ref_pts.cuda()
    ref = ops.msdeform_sample(value, offs_aw, ref_pts, shapes, heads, 4, torch.float32)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    P = _check_planes(lambda out, planes: ops.msdeform_sample(value, offs_aw, ref_pts, shapes, heads, 4, torch.float32, out=out, planes_out=planes, planes_only=True), ref)
    _consumer_same_bits(ref, P, seed=heads)


# ------------------------------------------------------------------------------------------------ depth-wise convolution
def _dw_inputs(Cc, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 21, Cc, generator=g).cuda()  # h = w = 2: a 4 x 4, a 2 x 2 and a 1 x 1 map
    w9c = (torch.randn(9, Cc, generator=g) / 3).cuda()
    bias = torch.randn(Cc, generator=g).cuda()
    return x, w9c, bias


def test_dwconv_planes(pingpong):
    ops = _ops()
    x, w9c, bias = _dw_inputs(32)
    ref = ops.dwconv3x3_gelu(x, w9c, bias, 2, 2)
    P = _check_planes(lambda out, planes: ops.dwconv3x3_gelu(x, w9c, bias, 2, 2, out=out, planes_out=planes, planes_only=True), ref)
    _consumer_same_bits(ref, P, seed=9)


# ------------------------------------------------------------------------------------------------ fallback, refusal, empty input
def _fallback(run, ref):
    """through the wrapper: the call keeps fp32 (planes invalid, the fp32 result in `out`, the planes' storage untouched)"""
    ops = _ops()
    dst, f32 = _Guarded(tuple(ref.shape)), _Guarded(tuple(ref.shape))
    P = ops.Planes(ref, storage=dst.t)
    run(f32.t, P)
    torch.cuda.synchronize()
    assert not P.valid and not P.only
    assert _bits_equal(f32.t, ref) and f32.guards_intact() and dst.untouched()


def _refused(call, dst):
    from siu3r_amd import _lib

    rc = call()
    torch.cuda.synchronize()
    assert rc != 0 and _lib.lib().siu3r_last_error(), "a planes call outside the rules must be refused"
    assert dst.untouched(), "a refused call wrote something"


def test_resize_fallback_refusal_empty():
    from siu3r_amd import _lib

    ops = _ops()
    L = _lib.lib()
    x = torch.randn(1, 3, 5, 36, generator=torch.Generator().manual_seed(1)).cuda()
    ref = ops.resize_bilinear(x, (6, 10), True)
    _fallback(lambda out, planes: ops.resize_bilinear(x, (6, 10), True, out=out, planes_out=planes, planes_only=True), ref)
    dst = _Guarded((1, 6, 10, 36))
    s = torch.cuda.current_stream().cuda_stream
    _refused(lambda: L.siu3r_resize_bilinear_planes(x.data_ptr(), _lib.F32, dst.t.data_ptr(), 1, 3, 5, 6, 10, 36, 1, 3 * 5 * 36, s), dst)
    _refused(lambda: L.siu3r_resize_bilinear_planes(x.data_ptr(), _lib.F32, dst.t.data_ptr() + 16, 1, 3, 5, 6, 10, 32, 1, 3 * 5 * 36, s), dst)  # misaligned planes
    assert L.siu3r_resize_bilinear_planes(None, _lib.F32, None, 0, 3, 5, 6, 10, 32, 1, 3 * 5 * 32, s) == 0


def test_msdeform_fallback_refusal_empty():
    from siu3r_amd import _lib

    ops = _ops()
    L = _lib.lib()
    g = torch.Generator().manual_seed(2)
    B, Q, heads, d, shapes = 1, 12, 1, 36, [(4, 5)]
    value = torch.randn(B, 20, heads * d, generator=g).cuda()
    offs_aw = torch.randn(B, Q, heads * 4 * 3, generator=g).cuda()
    ref_pts = torch.rand(Q, 1, 2, generator=g).cuda()
    ref = ops.msdeform_sample(value, offs_aw, ref_pts, shapes, heads, 4, torch.float32)
    _fallback(lambda out, planes: ops.msdeform_sample(value, offs_aw, ref_pts, shapes, heads, 4, torch.float32, out=out, planes_out=planes, planes_only=True), ref)
    dst = _Guarded((B, Q, heads * d))
    arr = (C.c_int32 * 2)(4, 5)
    s = torch.cuda.current_stream().cuda_stream
    _refused(lambda: L.siu3r_msdeform_sample_planes(value.data_ptr(), _lib.F32, offs_aw.data_ptr(), ref_pts.data_ptr(), arr, dst.t.data_ptr(), B, 20, Q, heads, d, 1, 4, s), dst)
    # two levels: no kernel specialised for it, so no planes form
    arr2 = (C.c_int32 * 4)(4, 4, 2, 2)
    _refused(lambda: L.siu3r_msdeform_sample_planes(value.data_ptr(), _lib.F32, offs_aw.data_ptr(), ref_pts.data_ptr(), arr2, dst.t.data_ptr(), B, 20, Q, 1, 32, 2, 4, s), dst)
    assert L.siu3r_msdeform_sample_planes(None, _lib.F32, None, None, arr, None, B, 20, 0, 1, 32, 1, 4, s) == 0


def test_dwconv_fallback_refusal_empty():
    from siu3r_amd import _lib

    ops = _ops()
    L = _lib.lib()
    x, w9c, bias = _dw_inputs(36, B=1)
    ref = ops.dwconv3x3_gelu(x, w9c, bias, 2, 2)
    _fallback(lambda out, planes: ops.dwconv3x3_gelu(x, w9c, bias, 2, 2, out=out, planes_out=planes, planes_only=True), ref)
    dst = _Guarded((1, 21, 36))
    s = torch.cuda.current_stream().cuda_stream
    _refused(lambda: L.siu3r_dwconv3x3_gelu_planes(x.data_ptr(), dst.t.data_ptr(), w9c.data_ptr(), bias.data_ptr(), 1, 2, 2, 36, s), dst)
    assert L.siu3r_dwconv3x3_gelu_planes(None, None, None, None, 0, 2, 2, 32, s) == 0


def test_attention_fallback_and_refusal():
    """head_dim 32 runs attn_fast_kernel, which has no planes form: the wrapper keeps fp32, the C entry point refuses out_x3"""
    from siu3r_amd import _lib

    ops = _ops()
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(1, 128, 2, 32, generator=g).cuda() for _ in range(3))
    kw = dict(heads=2, head_dim=32, scale=32 ** -0.5, split3=True)
    assert b"attn_fast_kernel" in ops.attention_plan(q, k, v, **kw).kernel
    ref = ops.attention(q, k, v, **kw)
    _fallback(lambda out, planes: ops.attention(q, k, v, out=out, planes_out=planes, planes_only=True, **kw), ref)
    dst = _Guarded((1, 128, 64))
    p = _lib.AttnParams()
    p.q, p.k, p.v, p.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), dst.t.data_ptr()
    p.dtype, p.B, p.H, p.Nq, p.Nk, p.D = _lib.F32, 1, 2, 128, 128, 32
    p.q_sb = p.k_sb = p.v_sb = 128 * 64
    p.q_sn = p.k_sn = p.v_sn = 64
    p.q_sh = p.k_sh = p.v_sh = 32
    p.scale, p.split3, p.out_x3 = 32 ** -0.5, 1, 1
    assert _lib.lib().siu3r_attention_out_x3_ok(C.byref(p)) == 0
    _refused(lambda: _lib.lib().siu3r_attention(C.byref(p), torch.cuda.current_stream().cuda_stream), dst)
    # the pipelined kernel with a destination off the 128-byte line is refused as well
    p.D, p.H, p.q_sh, p.k_sh, p.v_sh, p.out = 64, 1, 64, 64, 64, dst.t.data_ptr() + 16
    assert _lib.lib().siu3r_attention_out_x3_ok(C.byref(p)) == 0
    _refused(lambda: _lib.lib().siu3r_attention(C.byref(p), torch.cuda.current_stream().cuda_stream), dst)


# ------------------------------------------------------------------------------------------------ the model
def test_model_forward_same_bits_with_and_without_presplit():
    """SIU3RModel at 64 x 96, bf16x3: pre-split operands are a FORMAT.  The switch is read at call time, so both forwards run here."""
    from oracle import weights as OW
    from siu3r_amd import ops
    from siu3r_amd.model import SIU3RModel

    sd = OW.make_weights(0)
    g = torch.Generator().manual_seed(31)
    img = torch.rand(1, 2, 3, 64, 96, generator=g).cuda()
    K = torch.tensor([[318 / 256, 0, 0.5], [0, 318 / 256, 0.5], [0, 0, 1]])[None, None].repeat(1, 2, 1, 1).cuda()
    outs, presplit = [], []
    saved = ops._NO_PRESPLIT
    try:
        for off in (False, True):
            ops._NO_PRESPLIT = off
            m = SIU3RModel(sd, image_size=(64, 96), precision="bf16x3")
            m.use_graph = False
            log = []
            ops.set_plan_log(log)
            with torch.no_grad():
                outs.append(m(img, K, enable_query_class_logit_lift=True))
            torch.cuda.synchronize()
            ops.set_plan_log(None)
            presplit.append(sum(1 for pl in log if _presplit_a(pl)))
            del m
    finally:
        ops._NO_PRESPLIT = saved
        ops.set_plan_log(None)
    a, b = outs
    for f in ("means", "covariances", "harmonics", "opacities", "scales", "rotations", "semantic_labels", "instance_labels"):
        assert torch.equal(getattr(a[0], f), getattr(b[0], f)), f
    assert torch.equal(a[1].class_queries_logits, b[1].class_queries_logits) and torch.equal(a[1].masks_queries_logits, b[1].masks_queries_logits)
    print(f"[presplit producers] GEMM launches that read pre-split A: {presplit[0]} with planes, {presplit[1]} without")
    assert presplit[0] > 0 and presplit[1] == 0, presplit
    torch.cuda.empty_cache()
