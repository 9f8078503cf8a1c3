"""Branch coverage of csrc/elementwise.hip: every kernel through siu3r_amd.ops against a float64 CPU reference (torch.nn.functional or the
oracle) computed from the SAME dtype-rounded input, at the smallest shapes that enter each code path.  Metric: max |err| / max |ref|.
Bounds (the ones the older single-shape tests of these kernels use):
  fp32 pointwise, resize, pools, depth-wise conv, LayerNorm ... 1e-5
  GroupNorm, deformable sampler .............................. 2e-5  (GroupNorm also per group)
  Gaussian adapter ........................................... 3e-6, covariances 3e-5
  any bf16 input or output ................................... 8e-3
  max-pools, pack_image, hi plane of split_bf16 .............. bit equality
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TOL_BF16 = 8e-3
DT = {F32: "f32", BF16: "bf16", None: "none"}


def _ops():
    from siu3r_amd import ops

    return ops


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def tol_of(base, *dtypes):
    return TOL_BF16 if any(d == BF16 for d in dtypes) else base


class _Worst:
    """collects the worst error per name; every figure is recorded before it is asserted, and printed when the test ends"""

    def __init__(self):
        self.worst = {}

    def record(self, name, e, tol, what=""):
        cur = self.worst.get(name)
        if cur is None or not (e <= cur[0]):
            self.worst[name] = (e, tol)
        assert math.isfinite(e) and e <= tol, f"{name} {what}: rel_err {e:.3e} > {tol:.1e}"

    def check(self, name, got, ref, tol, what=""):
        self.record(name, rel_err(got, ref), tol, what)


@contextlib.contextmanager
def parity():
    w = _Worst()
    try:
        yield w
    finally:
        for name, (e, tol) in w.worst.items():
            print(f"[parity] {name}: rel_err={e:.3e} tol={tol:.1e}")


def off4(t):
    """the same values as a contiguous view that starts 4 bytes into a larger buffer"""
    buf = torch.empty(t.numel() + 4 // t.element_size(), dtype=t.dtype, device=t.device)
    v = buf[4 // t.element_size():].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 8 == 4
    return v


def nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().cuda().to(dt)


# ------------------------------------------------------------------------------------------------ GroupNorm
# (N, C, groups, HW): quads per pixel and group cg4 = C / groups / 4; a 1024-thread block walks total = HW * cg4 quads
GN_CASES = [
    (2, 256, 32, 37 * 41),  # cg4 = 2, total = 3034: one two-in-flight round, then a tail that threads < 986 run
    (1, 256, 32, 1024),     # total = 2048: one two-in-flight round, empty tail
    (2, 64, 8, 9 * 13),     # tail only
    (1, 128, 32, 1517),     # cg4 = 1
    (1, 128, 8, 1517),      # cg4 = 4
    (2, 72, 6, 1517),       # cg4 = 3: the general path (a division per load); groups % 8 != 0: no XCD remap
    (1, 48, 4, 5),          # total < the block size
]


def _gn_check(par, ops, xg, xq, gamma, beta, G, relu, ag, aq, odt, base):
    N, HW, C = xq.shape
    ref = F.relu(base) if relu else base
    if aq is not None:
        ref = ref + aq.double()
    out = ops.groupnorm(xg, gamma.cuda(), beta.cuda(), groups=G, relu=relu, addend=ag, out_dtype=odt)
    assert out.dtype == odt and out.shape == xg.shape
    tol = tol_of(2e-5, xq.dtype, odt, None if aq is None else aq.dtype)
    name = f"groupnorm[{DT[xq.dtype]}->{DT[odt]}]"
    what = f"N={N} C={C} groups={G} HW={HW} relu={relu} addend={DT[None if aq is None else aq.dtype]}"
    par.check(name, out, ref, tol, what)
    err = (out.double().cpu() - ref).abs().view(N, HW, G, C // G).amax(dim=(1, 3))
    mx = ref.abs().view(N, HW, G, C // G).amax(dim=(1, 3))
    par.record(name + " per group", (err / mx).max().item(), tol, what)


@pytest.mark.parametrize("case", GN_CASES, ids=[f"N{c[0]}_C{c[1]}_G{c[2]}_HW{c[3]}" for c in GN_CASES])
def test_groupnorm(case):
    ops = _ops()
    N, C, G, HW = case
    x = gen(N, HW, C, seed=100) * 2 + 5  # a mean of several standard deviations: E[x^2] - mean^2 has to be formed in double
    gamma, beta = gen(C, seed=101) * 0.5 + 1.0, gen(C, seed=102) * 0.5
    add = gen(N, HW, C, seed=103)
    with parity() as par:
        for xdt in (F32, BF16):
            xq = x.to(xdt)
            base = F.group_norm(xq.double().transpose(1, 2), G, gamma.double(), beta.double(), 1e-5).transpose(1, 2)
            xg = xq.cuda()
            for adt in (None, F32, BF16):
                aq = None if adt is None else add.to(adt)
                ag = None if aq is None else aq.cuda()
                for relu in (False, True):
                    for odt in (F32, BF16):
                        _gn_check(par, ops, xg, xq, gamma, beta, G, relu, ag, aq, odt, base)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [4, 252, 256, 260, 1024, 2044, 2048])
def test_layernorm_and_layernorm2(C):
    """one wave per row, eight register quads of 256 columns: C = 4 (one lane), a C that ends inside a round (252, 260, 2044), all eight
    quads (2048); rows 1 / 5 / 8 = a partial block, a block and a wave, two blocks"""
    ops = _ops()
    g, b = gen(C, seed=111) * 0.5 + 1.0, gen(C, seed=112) * 0.5
    gg, bg = g.cuda(), b.cuda()
    with parity() as par:
        for rows in (1, 5, 8):
            x = gen(rows, C, seed=113 + rows, scale=3.0) + 0.5
            ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)
            for odt in (F32, BF16):
                out = ops.layernorm(x.cuda(), gg, bg, 1e-6, out_dtype=odt)
                assert out.dtype == odt
                par.check(f"layernorm[->{DT[odt]}]", out, ref, tol_of(1e-5, odt), f"C={C} rows={rows}")
            o1, o2 = ops.layernorm2(x.cuda(), gg, bg, 1e-6)
            assert o1.dtype == F32 and o2.dtype == BF16 and o2.shape == o1.shape
            par.check("layernorm2[->f32]", o1, ref, 1e-5, f"C={C} rows={rows}")
            assert torch.equal(o2, o1.to(BF16)), f"layernorm2: the bf16 copy is not the rounded fp32 output (C={C} rows={rows})"
        x3 = gen(2, 4, C, seed=119, scale=2.0)
        ref3 = F.layer_norm(x3[:, :-1].double(), (C,), g.double(), b.double(), 1e-5)
        for odt in (F32, BF16):
            out3 = ops.layernorm(x3.cuda()[:, :-1], gg, bg, 1e-5, out_dtype=odt)
            par.check(f"layernorm strided[->{DT[odt]}]", out3, ref3, tol_of(1e-5, odt), f"C={C}")


@pytest.mark.parametrize("C", [2052, 6])
def test_layernorm_refuses_unsupported_widths(C):
    ops = _ops()
    x, g, b = gen(3, C, seed=120).cuda(), torch.ones(C).cuda(), torch.zeros(C).cuda()
    with pytest.raises(RuntimeError):
        ops.layernorm(x, g, b, 1e-6)
    with pytest.raises(RuntimeError):
        ops.layernorm2(x, g, b, 1e-6)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ resize
RESIZE_CASES = [((9, 13), [(1, 7), (7, 1), (9, 13), (14, 5), (27, 39)]), ((1, 13), [(4, 26)]), ((9, 1), [(18, 4)])]


@pytest.mark.parametrize("xdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [4, 36])
def test_resize_bilinear(C, xdt):
    """one output row / column (align_corners: the scale = 0 branch), identity, mixed up- and down-scaling, x3, one-pixel sources"""
    ops = _ops()
    with parity() as par:
        for (src, sizes) in RESIZE_CASES:
            x = gen(2, C, *src, seed=130 + src[0])
            xq = x.to(xdt)
            xg = nhwc(x, xdt)
            for size in sizes:
                for ac in (False, True):
                    ref = F.interpolate(xq.double(), size=size, mode="bilinear", align_corners=ac).permute(0, 2, 3, 1)
                    out = ops.resize_bilinear(xg, size, ac, out_dtype=F32)
                    par.check(f"resize[{DT[xdt]}->f32]", out, ref, tol_of(1e-5, xdt), f"C={C} {src}->{size} align={ac}")
                    if size == src:
                        assert torch.equal(out.cpu(), xq.float().permute(0, 2, 3, 1)), "identity resize changed a value"


@pytest.mark.parametrize("C", [4, 36])
def test_resize_bilinear_addend_and_affine(C):
    ops = _ops()
    x = gen(2, C, 9, 13, seed=140)
    sc, sh = gen(C, seed=141) * 0.5 + 1.0, gen(C, seed=142) * 0.5
    with parity() as par:
        for size in [(14, 5), (27, 39)]:
            add = gen(2, *size, C, seed=143).to(BF16)
            for ac in (False, True):
                ref = (F.interpolate(x.double(), size=size, mode="bilinear", align_corners=ac).permute(0, 2, 3, 1) + add.double()) * sc.double() + sh.double()
                for odt in (BF16, F32):
                    out = ops.resize_bilinear(nhwc(x, F32), size, ac, addend=add.cuda(), ch_scale=sc.cuda(), ch_shift=sh.cuda(), out_dtype=odt)
                    assert out.dtype == odt
                    par.check(f"resize+addend+affine[f32+bf16->{DT[odt]}]", out, ref, TOL_BF16, f"C={C} {size} align={ac}")


# ------------------------------------------------------------------------------------------------ affine_add / add
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["f32", "bf16"])
def test_affine_add_and_add(xdt):
    ops = _ops()
    C = 36
    x, a = gen(2, 5, 7, C, seed=150), gen(2, 5, 7, C, seed=151)
    sc, sh = gen(C, seed=152) * 0.5 + 1.0, gen(C, seed=153) * 0.5
    xq, aq = x.to(xdt), a.to(xdt)
    with parity() as par:
        for odt in (F32, BF16):
            tol = tol_of(1e-5, xdt, odt)
            out = ops.affine_add(xq.cuda(), None, sc.cuda(), sh.cuda(), out_dtype=odt)
            par.check(f"affine_add scale+shift[{DT[xdt]}->{DT[odt]}]", out, xq.double() * sc.double() + sh.double(), tol)
            out = ops.affine_add(xq.cuda(), aq.cuda(), None, None, out_dtype=odt)
            par.check(f"affine_add addend[{DT[xdt]}->{DT[odt]}]", out, xq.double() + aq.double(), tol)
            out = ops.affine_add(xq.cuda(), aq.cuda(), sc.cuda(), sh.cuda(), out_dtype=odt)
            par.check(f"affine_add addend+scale+shift[{DT[xdt]}->{DT[odt]}]", out, (xq.double() + aq.double()) * sc.double() + sh.double(), tol)
        if xdt == F32:
            rows = 30
            p = gen(6, 5, C, seed=154)
            for b_rows in (1, rows, rows // 3):
                q = gen(b_rows, C, seed=155 + b_rows)
                ref = p.double().view(rows, C) + q.double().repeat(rows // b_rows, 1)
                par.check("add", ops.add(p.cuda(), q.cuda()).view(rows, C), ref, 1e-5, f"b_rows={b_rows}")


# ------------------------------------------------------------------------------------------------ max-pools
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["f32", "bf16"])
def test_maxpools_are_exact(xdt):
    """all inputs negative: a padding value of 0 would win the max where -inf must; even, odd and one-pixel sizes"""
    ops = _ops()
    g = torch.Generator().manual_seed(160)
    for C in (4, 36):
        for size in [(8, 12), (9, 13), (1, 5), (2, 1)]:
            x = (-1 - torch.rand(2, C, *size, generator=g)).to(xdt)
            out = ops.maxpool3x3s2(nhwc(x, xdt))
            ref = F.max_pool2d(x.double(), 3, 2, 1).permute(0, 2, 3, 1)
            assert out.dtype == xdt and torch.equal(out.double().cpu(), ref), f"maxpool3x3s2 {size} C={C} [{DT[xdt]}]"
        for size in [(2, 3), (13, 18)]:
            x = (-1 - torch.rand(2, C, *size, generator=g)).to(xdt)
            out = ops.maxpool2x2s2(nhwc(x, xdt))
            ref = F.max_pool2d(x.double(), 2, 2).permute(0, 2, 3, 1)
            assert out.dtype == xdt and torch.equal(out.double().cpu(), ref), f"maxpool2x2s2 {size} C={C} [{DT[xdt]}]"
    print(f"[parity] maxpool3x3s2 / maxpool2x2s2 [{DT[xdt]}]: rel_err=0.000e+00 tol=0.0e+00")


# ------------------------------------------------------------------------------------------------ depth-wise conv
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["f32", "bf16"])
def test_dwconv3x3_gelu(xdt):
    """(2, 2): the maps are 4 x 4, 2 x 2 and 1 x 1 -- every neighbour of the coarsest map's only pixel is padding"""
    ops = _ops()
    B = 2
    with parity() as par:
        for (H, W) in [(2, 2), (4, 6), (6, 10)]:
            for C in (4, 36):
                n = H * W // 4
                x = gen(B, 21 * n, C, seed=170 + H).to(xdt)
                w, b = gen(C, 1, 3, 3, seed=171), gen(C, seed=172)
                outs = []
                for (a, e, hh, ww) in ((0, 16 * n, 2 * H, 2 * W), (16 * n, 20 * n, H, W), (20 * n, 21 * n, H // 2, W // 2)):
                    t = x.double()[:, a:e].transpose(1, 2).reshape(B, C, hh, ww)
                    outs.append(F.conv2d(t, w.double(), b.double(), padding=1, groups=C).flatten(2).transpose(1, 2))
                ref = F.gelu(torch.cat(outs, 1))
                out = ops.dwconv3x3_gelu(x.cuda(), w.reshape(C, 9).t().contiguous().cuda(), b.cuda(), H, W)
                assert out.dtype == xdt
                par.check(f"dwconv3x3_gelu[{DT[xdt]}]", out, ref, tol_of(1e-5, xdt), f"H={H} W={W} C={C}")


# ------------------------------------------------------------------------------------------------ deformable sampler
MSD_SHAPES = {1: [(6, 8)], 2: [(3, 4), (5, 2)], 3: [(3, 4), (6, 8), (12, 16)], 4: [(3, 4), (6, 8), (12, 16), (2, 3)]}
MSD_B, MSD_HEADS = 2, 2
# (L, P, d, Q)
MSD_CASES = [
    (1, 4, 32, 70), (3, 4, 32, 70), (4, 4, 32, 70),  # templated bodies, 32 queries per block, ragged last block
    (4, 4, 64, 5),                                   # templated, fewer queries than a block holds
    (3, 4, 12, 70), (3, 4, 24, 70),                  # templated body in the flat thread order (d / 4 does not divide 256)
    (2, 4, 32, 70),                                  # generic body (no L = 2 instantiation)
    (3, 2, 32, 70), (3, 8, 32, 70),                  # generic body (P != 4)
]
MSD_IDS = [f"L{c[0]}_P{c[1]}_d{c[2]}_Q{c[3]}" for c in MSD_CASES]


def _msd_place(ref_l, offs, q, shapes, fx_of, fy_of):
    """put every sample of query q at pixel coordinates (fx_of(l, p, w), fy_of(l, p, h)) of its level: with the reference point in the
    middle, pixel = 0.5 * size + offset - 0.5"""
    ref_l[q] = 0.5
    for l, (hh, ww) in enumerate(shapes):
        for p in range(offs.shape[4]):
            offs[:, q, :, l, p, 0] = fx_of(l, p, ww) + 0.5 - 0.5 * ww
            offs[:, q, :, l, p, 1] = fy_of(l, p, hh) + 0.5 - 0.5 * hh


def _msd_inputs(L, P, d, Q, seed):
    shapes = MSD_SHAPES[L]
    S = sum(a * b for a, b in shapes)
    g = torch.Generator().manual_seed(seed)
    value = gen(MSD_B, S, MSD_HEADS * d, seed=seed + 1)
    offs = gen(MSD_B, Q, MSD_HEADS, L, P, 2, seed=seed + 2, scale=3.0)  # several pixels: some samples fall outside
    logits = gen(MSD_B, Q, MSD_HEADS, L * P, seed=seed + 3, scale=2.0)
    ref_l = torch.rand(Q, L, 2, generator=g)
    # hand-placed rows: texel centres, the four coordinates at which a corner enters or leaves the map, ten maps outside on either side
    kinds = [lambda s: 0.5 * s, lambda s: -1.0, lambda s: -0.5, lambda s: s - 1.0, lambda s: s - 0.5, lambda s: 10.5 * s - 0.5, lambda s: -9.5 * s - 0.5,
             lambda s: 0.0, lambda s: 1.0]
    for q in range(min(Q, len(kinds))):
        _msd_place(ref_l, offs, q, shapes, lambda l, p, w: kinds[(q + p) % len(kinds)](w), lambda l, p, h: kinds[(q + 3 * p + l) % len(kinds)](h))
    return shapes, S, value, offs, logits, ref_l


def _msd_reference(value_q, shapes, offs, logits, ref_l, d):
    from oracle import siu3r_oracle as O

    B, Q, heads, L, P, _ = offs.shape
    norm = torch.tensor([[s[1], s[0]] for s in shapes], dtype=torch.float64)
    loc = ref_l.double()[None, :, None, :, None, :] + offs.double() / norm[None, None, None, :, None, :]
    aw = logits.double().softmax(-1).view(B, Q, heads, L, P)
    return O.msdeform_core(value_q.double().view(B, -1, heads, d), shapes, loc, aw), loc


def _offs_aw(offs, logits):
    B, Q = offs.shape[:2]
    return torch.cat([offs.reshape(B, Q, -1), logits.reshape(B, Q, -1)], -1).contiguous()


@pytest.mark.parametrize("adt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", MSD_CASES, ids=MSD_IDS)
def test_msdeform_sample(case, adt):
    ops = _ops()
    L, P, d, Q = case
    shapes, S, value, offs, logits, ref_l = _msd_inputs(L, P, d, Q, seed=200)
    vq = value.to(adt)
    ref, _ = _msd_reference(vq, shapes, offs, logits, ref_l, d)
    oa = _offs_aw(offs, logits).cuda()
    with parity() as par:
        out = ops.msdeform_sample(vq.cuda(), oa, ref_l.cuda(), shapes, MSD_HEADS, P, F32)
        par.check(f"msdeform_sample[{DT[adt]}->f32]", out, ref, tol_of(2e-5, adt), f"L={L} P={P} d={d} Q={Q}")
        if P == 4:
            # offsets that are not 16-byte aligned take the generic body: the same products in another order
            out_g = ops.msdeform_sample(vq.cuda(), off4(oa), ref_l.cuda(), shapes, MSD_HEADS, P, F32)
            par.check(f"msdeform_sample generic body[{DT[adt]}->f32]", out_g, ref, tol_of(2e-5, adt), f"L={L} P={P} d={d} Q={Q}")
            par.check("msdeform_sample templated vs generic body", out, out_g, 2e-6, f"L={L} P={P} d={d} Q={Q} [{DT[adt]}]")
        if adt == BF16:
            outb = ops.msdeform_sample(vq.cuda(), oa, ref_l.cuda(), shapes, MSD_HEADS, P, BF16)
            assert outb.dtype == BF16
            par.check("msdeform_sample[bf16->bf16]", outb, ref, TOL_BF16, f"L={L} P={P} d={d} Q={Q}")


MSD_INF_CASES = [((1, 4, 32, 70), F32), ((3, 4, 32, 70), F32), ((3, 4, 32, 70), BF16), ((4, 4, 32, 70), F32), ((4, 4, 64, 5), F32), ((3, 4, 12, 70), F32),
                 ((2, 4, 32, 70), F32), ((3, 2, 32, 70), F32)]


@pytest.mark.parametrize("case,adt", MSD_INF_CASES, ids=[f"L{c[0]}_P{c[1]}_d{c[2]}_Q{c[3]}_{DT[a]}" for c, a in MSD_INF_CASES])
def test_msdeform_sample_non_finite_texel(case, adt):
    """texel (0, 0) of one level is +inf.  grid_sample's zero padding, the oracle and the generic body SKIP an out-of-range corner; a body
    that loads the clamped texel instead must not let it through (0 * inf = NaN): an output whose in-range corners never include the
    texel stays finite, one that samples it with a positive weight is non-finite exactly where the oracle is."""
    ops = _ops()
    L, P, d, Q = case
    shapes, S, value, offs, logits, ref_l = _msd_inputs(L, P, d, Q, seed=230)
    li = min(1, L - 1)
    hh, ww = shapes[li]
    # query 0: every sample left of the map beside row 0 (both corners out of range, both clamp onto column 0); query 1: ten maps
    # outside towards negative coordinates (all four corners clamp onto texel (0, 0)); query 2: inside the texel's support
    _msd_place(ref_l, offs, 0, shapes, lambda l, p, w: -1.5, lambda l, p, h: 0.3 - 0.1 * p)
    _msd_place(ref_l, offs, 1, shapes, lambda l, p, w: -9.5 * w - 0.5, lambda l, p, h: -9.5 * h - 0.5)
    _msd_place(ref_l, offs, 2, shapes, lambda l, p, w: 0.25, lambda l, p, h: 0.25)
    start = sum(a * b for a, b in shapes[:li])
    value[:, start] = float("inf")
    vq = value.to(adt)
    ref, loc = _msd_reference(vq, shapes, offs, logits, ref_l, d)
    fx, fy = loc[:, :, :, li, :, 0] * ww - 0.5, loc[:, :, :, li, :, 1] * hh - 0.5  # [B, Q, heads, P]
    m = 1e-3  # fp32 pixel coordinates of this size carry ~1e-6: a sample this close to the edge of the texel's support is not classified
    near = (fx.abs() < 1 + m) & (fy.abs() < 1 + m)          # texel (0, 0) may be an in-range corner of the sample
    inside = (fx.abs() < 1 - m) & (fy.abs() < 1 - m)        # ... and is one, with weight (1 - |fx|)(1 - |fy|) > 0
    clamps = (fx < 1) & (fy < 1) & ~near                    # an out-of-range corner clamps onto the texel
    clear, hit = ~near.any(-1), inside.any(-1)              # [B, Q, heads]
    assert clear[:, 0].all() and clear[:, 1].all() and hit[:, 2].all()
    assert (clear & clamps.any(-1)).sum() >= 2 * MSD_B * MSD_HEADS and hit.sum() >= MSD_B * MSD_HEADS
    ref = ref.view(MSD_B, Q, MSD_HEADS, d)
    assert torch.isfinite(ref[clear]).all() and not torch.isfinite(ref[hit]).any()  # what the float64 oracle does
    out = ops.msdeform_sample(vq.cuda(), _offs_aw(offs, logits).cuda(), ref_l.cuda(), shapes, MSD_HEADS, P, F32).cpu().view(MSD_B, Q, MSD_HEADS, d)
    bad = (~torch.isfinite(out[clear])).sum().item()
    assert bad == 0, f"{bad} outputs whose in-range corners never include the non-finite texel are not finite"
    assert torch.equal(torch.isfinite(out[hit]), torch.isfinite(ref[hit])), "outputs that sample the non-finite texel differ from the oracle in finiteness"
    with parity() as par:
        par.check(f"msdeform_sample beside a non-finite texel[{DT[adt]}->f32]", out[clear], ref[clear], tol_of(2e-5, adt), f"L={L} P={P} d={d} Q={Q}")


# ------------------------------------------------------------------------------------------------ Gaussian adapter / pts3d
def _adapter_check(par, out, raw_q, tag):
    from oracle import siu3r_oracle as O

    n = raw_q.shape[0]
    g = O.gaussian_adapter(torch.zeros(n, 3, dtype=torch.float64), raw_q.double())
    hand = torch.zeros(n, dtype=torch.bool)
    hand[:3] = True  # the hand-set rows are 10 .. 100 x larger: checked on their own so that they do not set the scale for the others
    for rows, rn in ((hand, "hand-set rows"), (~hand, "ordinary rows")):
        if not rows.any():
            continue
        for kk in ("opacities", "scales", "rotations", "harmonics", "covariances"):
            assert out[kk].dtype == F32 and out[kk].shape == g[kk].shape
            base = 3e-5 if kk == "covariances" else 3e-6
            par.check(f"gaussian_adapter.{kk}[{DT[raw_q.dtype]}]", out[kk].cpu()[rows], g[kk][rows], tol_of(base, raw_q.dtype), f"{tag} {rn}")


def _adapter_raw(n, seed):
    raw = gen(n, 83, seed=seed, scale=4.0)
    raw[0, 1:4] = 30.0  # softplus threshold (x > 20)
    if n > 1:
        raw[1, 4:8] = 0.0  # zero quaternion -> eps path
    if n > 2:
        raw[2, 1:4] = 400.0  # 0.001 * 400 > the 0.3 clamp
    return raw


@pytest.mark.parametrize("adt", [F32, BF16], ids=["f32", "bf16"])
def test_gaussian_adapter(adt):
    """128 rows per block: one row, one short of a block, a block, a block and a row, two blocks and five rows"""
    ops = _ops()
    with parity() as par:
        for n in (1, 127, 128, 129, 256 + 5):
            raw_q = _adapter_raw(n, 300 + n).to(adt)
            _adapter_check(par, ops.gaussian_adapter(raw_q.cuda()), raw_q, f"n={n}")


def test_gaussian_adapter_reads_a_view_that_is_only_4_byte_aligned():
    """two full blocks whose first row is row 1 of a larger buffer: 83 floats = 332 bytes into it, no 16-byte vector load may be used"""
    ops = _ops()
    raw = _adapter_raw(256, 310)
    buf = torch.zeros(257, 83).cuda()
    view = buf[1:]
    view.copy_(raw)
    assert view.is_contiguous() and view.data_ptr() % 16 == 12
    with parity() as par:
        _adapter_check(par, ops.gaussian_adapter(view), raw, "n=256 from row 1")


@pytest.mark.parametrize("n", [1, 255, 257])
def test_pts3d_exp(n):
    ops = _ops()
    xyz = gen(n, 3, seed=320 + n, scale=2.0)
    if n > 1:
        xyz[0] = 0.0  # |xyz| = 0 -> clip(min=1e-8) branch
        xyz[-1] = 0.0
    d = xyz.double().norm(dim=-1, keepdim=True)
    ref = xyz.double() / d.clip(min=1e-8) * torch.expm1(d)
    out = ops.pts3d_exp_(xyz.cuda().clone())
    with parity() as par:
        par.check("pts3d_exp", out, ref, 2e-6, f"n={n}")
    if n > 1:
        assert float(out[0].abs().max()) == 0.0 and float(out[-1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ Mask2Former attention mask
@pytest.mark.parametrize("Q", [100, 7])
@pytest.mark.parametrize("T", [1, 2])
def test_m2f_attn_mask(T, Q):
    ops = _ops()
    B, IH, IW = 2, 8, 12
    ml = gen(B, Q, T, IH, IW, seed=340 + 10 * T + Q, scale=3.0)
    ml[0, 3] = -5.0  # fully blocked row, in batch item 0 only -> re-opened
    mg = ml.permute(0, 2, 3, 4, 1).contiguous().cuda()
    for size in [(4, 6), (8, 12), (16, 24), (1, 1)]:
        lg = F.interpolate(ml.double().flatten(0, 1), size=size, mode="bilinear", align_corners=False).view(B, Q, T, *size)
        # no sample of these seeded inputs is a tie: the mismatch allowance below is never used up by rounding
        assert lg.abs().min().item() > 1e-6, f"a logit sample within 1e-6 of 0 at {size}: move the seed"
        am = lg.flatten(2) < 0
        full = am.all(-1)
        assert full[0, 3] and (size == (1, 1) or not full[1, 3])
        am[full] = False
        out = ops.m2f_attn_mask(mg, size)
        nk = am.shape[-1]
        assert out.dtype == torch.uint8 and out.shape[:2] == (B, Q) and out.shape[-1] % 64 == 0 and out.shape[-1] >= nk
        out = out[:, :, :nk].cpu()
        assert int(out.max()) <= 1
        mism = (out.bool() != am).double().mean().item()
        print(f"[parity] m2f_attn_mask T={T} Q={Q} {size}: mismatch fraction {mism:.2e} tol=1.0e-04")
        assert mism <= 1e-4
        assert not out[0, 3].any()


# ------------------------------------------------------------------------------------------------ pack_image / split_bf16
def test_pack_image_nhwc():
    ops = _ops()
    img = gen(2, 3, 5, 7, seed=360)
    for cpad, odt in ((4, F32), (8, F32), (8, BF16)):
        out = ops.pack_image_nhwc(img.cuda(), odt, cpad)
        assert out.dtype == odt and tuple(out.shape) == (2, 5, 7, cpad)
        assert torch.equal(out[..., :3].cpu(), img.permute(0, 2, 3, 1).to(odt)), f"pack_image cpad={cpad} [{DT[odt]}]: RGB"
        assert float(out[..., 3:].float().abs().max()) == 0.0, f"pack_image cpad={cpad} [{DT[odt]}]: padding channels"
    print("[parity] pack_image_nhwc: rel_err=0.000e+00 tol=0.0e+00")


@pytest.mark.parametrize("k,kpad", [(1, 32), (32, 32), (32, 64), (100, 128)])
def test_split_bf16(k, kpad):
    """a source whose rows lie k + 4 apart; k == kpad (no padding column), one to four 32-deep tiles in the interleaved form"""
    ops = _ops()
    rows = 7
    full = gen(rows, k + 4, seed=370 + k)
    x = full[:, :k]
    xg = full.cuda()[:, :k]
    assert xg.stride(0) == k + 4
    hi, lo, kp, x3 = ops.split_bf16(xg, True, kpad=kpad, want_x3=True)
    assert kp == kpad and hi.shape == (rows, kpad) and lo.shape == (rows, kpad) and x3.shape == (rows, kpad // 32, 2, 32)
    assert torch.equal(hi[:, :k].cpu(), x.to(BF16)), "hi plane is not the rounded input"
    err = (hi[:, :k].double().cpu() + lo[:, :k].double().cpu() - x.double()).abs()
    worst = (err / x.double().abs()).max().item()
    print(f"[parity] split_bf16 k={k} kpad={kpad}: rel_err={worst:.3e} tol={2.0 ** -16:.1e}")
    assert (err <= 2.0 ** -16 * x.double().abs()).all()
    if kpad > k:
        assert float(hi[:, k:].float().abs().max()) == 0.0 and float(lo[:, k:].float().abs().max()) == 0.0
    assert torch.equal(x3[:, :, 0].reshape(rows, kpad), hi) and torch.equal(x3[:, :, 1].reshape(rows, kpad), lo)
    hi1, lo1, _ = ops.split_bf16(xg, False, kpad=kpad)
    assert lo1 is None and torch.equal(hi1, hi)


# ------------------------------------------------------------------------------------------------ empty inputs, alignment
def test_empty_inputs_return_empty_outputs():
    """an empty leading dimension is a no-op that returns the empty tensor of the right shape and dtype; the next ordinary call is unaffected"""
    ops = _ops()
    C = 8
    e = lambda *s, dt=F32: torch.empty(*s, dtype=dt).cuda()
    ones, zeros = torch.ones(C).cuda(), torch.zeros(C).cuda()

    def same(t, shape, dt):
        assert tuple(t.shape) == tuple(shape) and t.dtype == dt and t.is_cuda, (t.shape, t.dtype, shape, dt)

    for dt in (F32, BF16):
        same(ops.resize_bilinear(e(0, 3, 5, C, dt=dt), (6, 10), False), (0, 6, 10, C), dt)
        same(ops.resize_bilinear(e(0, 3, 5, C, dt=dt), (6, 10), True, addend=e(0, 6, 10, C), ch_scale=ones, ch_shift=zeros, out_dtype=F32), (0, 6, 10, C), F32)
        same(ops.affine_add(e(0, 3, 5, C, dt=dt), e(0, 3, 5, C, dt=dt), ones, zeros), (0, 3, 5, C), dt)
        same(ops.maxpool3x3s2(e(0, 5, 7, C, dt=dt)), (0, 3, 4, C), dt)
        same(ops.maxpool2x2s2(e(0, 5, 7, C, dt=dt)), (0, 2, 3, C), dt)
        same(ops.dwconv3x3_gelu(e(0, 21 * 6, C, dt=dt), e(9, C), zeros, 4, 6), (0, 21 * 6, C), dt)
        same(ops.groupnorm(e(0, 5, 7, C, dt=dt), ones, zeros, groups=2, relu=True), (0, 5, 7, C), dt)
        same(ops.groupnorm(e(0, 35, C, dt=dt), ones, zeros, groups=2, addend=e(0, 35, C), out_dtype=F32), (0, 35, C), F32)
        same(ops.gaussian_adapter(e(0, 83, dt=dt))["covariances"], (0, 3, 3), F32)
        for (B, Q) in ((0, 5), (2, 0)):
            out = ops.msdeform_sample(e(B, 6 * 8, 2 * C, dt=dt), e(B, Q, 2 * 1 * 4 * 3), e(Q, 1, 2), [(6, 8)], 2, 4, F32)
            same(out, (B, Q, 2 * C), F32)
    g = ops.gaussian_adapter(e(0, 4, 83))
    for kk, tail in (("opacities", ()), ("scales", (3,)), ("rotations", (4,)), ("harmonics", (3, 25)), ("covariances", (3, 3))):
        same(g[kk], (0, 4, *tail), F32)
    same(ops.pts3d_exp_(e(0, 3)), (0, 3), F32)
    same(ops.m2f_attn_mask(e(0, 2, 8, 12, 7), (4, 6)), (0, 7, 64), torch.uint8)
    same(ops.layernorm(e(0, C), ones, zeros, 1e-6), (0, C), F32)
    same(ops.layernorm(e(0, C), ones, zeros, 1e-6, out_dtype=BF16), (0, C), BF16)
    o1, o2 = ops.layernorm2(e(0, C), ones, zeros, 1e-6)
    same(o1, (0, C), F32)
    same(o2, (0, C), BF16)
    same(ops.add(e(0, C), e(1, C)), (0, C), F32)
    same(ops.pack_image_nhwc(e(0, 3, 5, 7), BF16, 8), (0, 5, 7, 8), BF16)
    hi, lo, kpad = ops.split_bf16(e(0, 40), True)
    same(hi, (0, 64), BF16)
    same(lo, (0, 64), BF16)
    torch.cuda.synchronize()
    # ordinary calls straight afterwards
    with parity() as par:
        x = gen(2, C, 5, 7, seed=380)
        par.check("resize after an empty call", ops.resize_bilinear(nhwc(x, F32), (10, 14), False),
                  F.interpolate(x.double(), size=(10, 14), mode="bilinear", align_corners=False).permute(0, 2, 3, 1), 1e-5)
        gm, bt = gen(C, seed=381) * 0.5 + 1.0, gen(C, seed=382) * 0.5
        par.check("groupnorm after an empty call", ops.groupnorm(nhwc(x, F32), gm.cuda(), bt.cuda(), groups=2),
                  F.group_norm(x.double(), 2, gm.double(), bt.double(), 1e-5).permute(0, 2, 3, 1), 2e-5)
        assert torch.equal(ops.maxpool3x3s2(nhwc(x, F32)).cpu(), F.max_pool2d(x, 3, 2, 1).permute(0, 2, 3, 1))
        raw = _adapter_raw(5, 383)
        _adapter_check(par, ops.gaussian_adapter(raw.cuda()), raw, "after an empty call")


def test_misaligned_base_pointers_are_refused():
    """the kernels load 4 elements per lane (16 bytes of fp32, 8 of bf16): a contiguous view that starts 4 bytes into a buffer is refused
    on the host, before anything is launched"""
    ops = _ops()
    C = 8
    x = gen(2, 5, 7, C, seed=390).cuda()
    ones, zeros = torch.ones(C).cuda(), torch.zeros(C).cuda()
    calls = [
        lambda: ops.add(off4(x), x),
        lambda: ops.add(x, off4(x)),
        lambda: ops.maxpool3x3s2(off4(x)),
        lambda: ops.maxpool2x2s2(off4(x)),
        lambda: ops.layernorm(off4(x), ones, zeros, 1e-6),
        lambda: ops.layernorm(x, off4(ones), zeros, 1e-6),
        lambda: ops.layernorm2(off4(x), ones, zeros, 1e-6),
        lambda: ops.resize_bilinear(off4(x), (10, 14), False),
        lambda: ops.resize_bilinear(x, (5, 7), False, addend=off4(x)),
        lambda: ops.affine_add(off4(x), None, ones, zeros),
        lambda: ops.groupnorm(off4(x), ones, zeros, groups=2),
        lambda: ops.groupnorm(x, ones, zeros, groups=2, addend=off4(x)),
        lambda: ops.dwconv3x3_gelu(off4(gen(2, 21, C, seed=391).cuda()), torch.zeros(9, C).cuda(), zeros, 2, 2),
        lambda: ops.msdeform_sample(off4(gen(2, 48, 2 * C, seed=392).cuda()), torch.zeros(2, 5, 24).cuda(), torch.zeros(5, 1, 2).cuda(), [(6, 8)], 2, 4, F32),
        lambda: ops.maxpool3x3s2(off4(x.to(BF16))),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="align"):
            call()
        torch.cuda.synchronize()
    # (bf16: off4 starts 2 elements = 4 bytes in, short of the 8 bytes a 4-element load needs)
    assert torch.equal(ops.add(x, x), x + x) and torch.equal(ops.maxpool3x3s2(x).cpu(), F.max_pool2d(x.cpu().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
