"""Dense float64 restatements of the two dedicated bf16x3 row-stream kernels at the ends of the DPT heads, written from the ABI comments
of include/siu3r_hip.h and from ops.pack_stem7 / ops.pack_proj (not from the kernels), plus the scales, the derived bounds, the launch
arithmetic, the input generators and the case lists that tests/test_rowstream_ref.py (CPU) and tests/test_rowstream_gpu.py (GPU) share.
The metric, the plane helpers and the constants are those of tests/dense_gemm64.py.

    siu3r_stem7x7_x3:   out[z, y, x, n] = ReLU( sum_{ky, kx, c} img[z, y + ky - 3, x + kx - 3, c] W_g[n, c, ky, kx] + bias_g[n] )
                                          + up_x2(up_src[z])[y, x, n]              z = b * G + g, pixels outside the image are zero,
                        up_x2 = bilinear, align_corners: fy = y (sh - 1) / (H - 1), y0 = floor(fy), y1 = min(y0 + 1, sh - 1) (x alike)
    siu3r_proj_rows_x3: out[z, m, n] = sum_k x[z, m, k] W_g[n, k] + bias_g[n]      g = z % G

Operands as the kernel sees them: fp32 activations; weights as the packed planes read back, hi = bf16(w) and lo = bf16(w - hi), both
round-to-nearest-even (test_rowstream_gpu.py unpacks ops.pack_stem7 / ops.pack_proj by their lane map and requires exactly these).

SCALES AND BOUNDS.  u = 2^-24.  Every element is held to |out - ref| <= bound * S + extra.

  proj   S = sum_k |x||w| + |bias|,  bound = K u + X3_TERM,  extra = 0.
         K u: the fp32 accumulation of the K products and the bias in any order (the three MFMAs of a K step add 16 exact bf16 x bf16
         products each into the fp32 accumulator: K / 16 * 3 + 1 <= K roundings of partial sums, each at most u S).  X3_TERM = 3 * 2^-16:
         the two lo roundings and the dropped lo * lo product (dense_gemm64.py's header; A's hi plane is truncated here as well).
  stem   convolution part: S = S_conv = sum |a||w| + |bias|, bound = (224 + 1) u + X3_TERM.  224 is the kernel's padded K
         (ky, kx in 0..7, c in 0..3: 14 steps of 16), its products and the bias as above; + 1 u for the last addition of the
         epilogue (the ReLU'd value plus the upsampled one), whose rounding is relative to the sum and |ReLU(v)| <= S_conv.  ReLU is
         1-Lipschitz and exact: the error of its argument passes through unamplified.
         upsample part (extra), two terms:
           UP_OPS u S_up, S_up = the interpolated |up_src|.  The lerp as the kernel writes it (no contraction: the library is built
           with -ffp-contract=off):  v += (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d).
           Roundings on the longest path, corner a: 1 - lx, its product with a, the sum with lx * b, 1 - ly, the product with it, the
           sum of the two rows, the sum with v: UP_OPS = 7 (b: 6; c, d alike).  fx - x0 is exact (x0 = trunc(fx) <= fx < 2^24).
           (dy + dx) C, the coordinates.  The kernel computes ry = fl(fl(sh - 1) / fl(H - 1)) and fy = fl(ry * oy): two roundings, so
           |fy32 - fy| <= dy = ((1 + u)^2 - 1) fy, and truncates; near an integer its y0 may differ from the float64 floor.  The
           interpolant is continuous and piecewise bilinear, and inside a cell |d/dy| <= (1 - lx)|c - a| + lx |d - b| <= the UNWEIGHTED
           sum of the four |corners| (|d/dx| alike), so the effect is at most (dy + dx) C with C that sum -- taken over the cell of
           the float64 coordinate and, where that coordinate lies within dy (dx) of a cell boundary, the neighbouring cell too: the
           kernel may be in either.  The interpolated value would not do: it vanishes where the corners cancel.
  planes (stem, planes_out): not bounded but required BITWISE equal to split_planes(the fp32 output of the same launch arguments).

No number here comes from a GPU run.

LAUNCH ARITHMETIC, restated from the comments of the entry points (one workgroup per CU, 256 CUs shared by the G heads / the Z
problems): stem_grid, proj_grid.  Both kernels are persistent: workgroup i of a head (a z) runs tiles i, i + nwg, i + 2 nwg, ...

Not a test module."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_gemm64 import (PLANES_REL, SENTINEL_ROWS, U24, X3_TERM, assert_elems_close, join_planes, rne_bf16, split_planes,  # noqa: E402,F401
                          trunc_bf16, untouched, worst_ratio)

CUS = 256
STEM_C = 256                 # output channels of the stem
STEM_TW, STEM_TH = 16, 8     # a workgroup's tile: 16 x 8 pixels
STEM_KPAD = 224              # (ky, kx in 0..7, c in 0..3)
UP_OPS = 7
FILL_BITS = 0x7FA5C3D2       # the canary: one NaN bit pattern everywhere outside (and, before the launch, inside) the outputs
PROJ_ROWS = {256: 64, 128: 128}   # rows per tile of the two instantiations


def _u(g, *shape, lo=-1.0, hi=1.0):
    return (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)).float()


def split_w(w):
    """fp32 weights -> the packed planes read back (hi, lo) as fp32 tensors"""
    hi = rne_bf16(w)
    return hi, rne_bf16(w - hi)


# ------------------------------------------------------------------------------------------------
# launch arithmetic
# ------------------------------------------------------------------------------------------------
def stem_grid(B, G, H, W):
    """(workgroups per head, tiles per head): 16 x 8 pixel tiles over the B images of a head, min(256 / G, tiles) workgroups"""
    ntiles = B * (H // STEM_TH) * (W // STEM_TW)
    return min(max(CUS // G, 1), ntiles), ntiles


def proj_grid(Z, M, K, N):
    """(workgroups per z, tiles per z, rows per tile): min(max(256 / Z, 1), tiles) workgroups"""
    rows = PROJ_ROWS[K]
    ntiles = (M + rows - 1) // rows
    return min(max(CUS // Z, 1), ntiles), ntiles, rows


def tiles_per_wg(nwg, ntiles):
    """tiles that workgroup 0 .. nwg - 1 runs"""
    return [len(range(i, ntiles, nwg)) for i in range(nwg)]


def proj_dispatch(K, n):
    """the dispatch conditions of siu3r_proj_rows_x3 restated by hand: (K, column blocks of 32) must be (256, 3) or (128, 1)"""
    nb = (n + 31) // 32
    return n > 0 and ((K == 256 and nb == 3) or (K == 128 and nb == 1))


# ------------------------------------------------------------------------------------------------
# stem: cases and inputs
# ------------------------------------------------------------------------------------------------
class StemCase:
    """props: what the case is there for, asserted on stem_grid by check_props -- "single" (one tile per workgroup), "multi2" / "multi3"
    (some workgroup runs >= 2 / 3 tiles), "ragged" (ntiles % nwg != 0), "cross" (consecutive tiles of a workgroup lie in different
    batch items)"""

    def __init__(self, B, G, H, W, up, bias, props, impulse=False):
        self.B, self.G, self.H, self.W, self.up, self.bias, self.props, self.impulse = B, G, H, W, up, bias, tuple(props), impulse
        self.Z, self.sh, self.sw = B * G, H // 2, W // 2
        self.shape = (B, G, H, W, impulse)
        self.id = f"stem-g{G}-b{B}-{H}x{W}" + ("-impulse" if impulse else "") + ("-up" if up else "") + ("-bias" if bias else "")
        self.nwg, self.ntiles = stem_grid(B, G, H, W)
        self.per_img = (H // STEM_TH) * (W // STEM_TW)

    def check_props(self):
        per = tiles_per_wg(self.nwg, self.ntiles)
        if "single" in self.props:
            assert max(per) == 1, (self.id, per)
        if "multi2" in self.props:
            assert max(per) >= 2, (self.id, per)
        if "multi3" in self.props:
            assert max(per) >= 3, (self.id, per)
        if "ragged" in self.props:
            assert self.ntiles % self.nwg != 0, (self.id, self.nwg, self.ntiles)
        if "cross" in self.props:
            assert all(t // self.per_img != (t + self.nwg) // self.per_img for t in range(self.ntiles - self.nwg)), self.id
        return per


def impulse_sites(H, W):
    """the four image corners, both sides of a tile seam in x (columns 15 | 16) and in y (rows 7 | 8), one interior pixel"""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2 + 3, 15), (H // 2 + 3, 16), (7, W // 2 - 3), (8, W // 2 - 3), (H // 2 + 2, W // 2 + 5)]


def stem_inputs(c):
    """seeded CPU inputs of the case's shape (shared by its up / bias variants): img [B, G, H, W, 4] (channel 3 zero), W [G, 256, 3, 7, 7]
    with its planes w_hi / w_lo, bias [G, 256], up [B, G, H/2, W/2, 256] rough (independent per source pixel).  Impulse images: one
    non-zero pixel in one channel per image -- image z takes site z % 9 and channel (z / 9) % 3 -- and a positive bias above the
    largest product, so that the ReLU passes every tap and S is of one tap's magnitude."""
    g = torch.Generator().manual_seed(9100 + 7 * c.G + 131 * c.B + c.H + 3 * c.W)
    img = _u(g, c.B, c.G, c.H, c.W, 4)
    img[..., 3] = 0
    W = _u(g, c.G, STEM_C, 3, 7, 7, lo=-0.2, hi=0.2)
    bias = _u(g, c.G, STEM_C)
    if c.impulse:
        val = _u(g, c.Z, lo=0.5, hi=1.0) * torch.where(torch.arange(c.Z) % 2 == 0, 1.0, -1.0)
        img.zero_()
        sites = impulse_sites(c.H, c.W)
        for z in range(c.Z):
            y, x = sites[z % len(sites)]
            img[z // c.G, z % c.G, y, x, (z // len(sites)) % 3] = val[z]
        bias = _u(g, c.G, STEM_C, lo=0.25, hi=0.5)
    up = _u(g, c.B, c.G, c.sh, c.sw, STEM_C, lo=-2.0, hi=2.0)
    hi, lo = split_w(W)
    return dict(img=img, W=W, w_hi=hi, w_lo=lo, bias=bias, up=up)


def _stem_cases():
    cs = []
    for (B, G, H, W, props) in ((2, 2, 48, 32, ("single",)), (3, 16, 32, 48, ("multi3", "ragged", "cross")),
                                (3, 2, 64, 128, ("multi2", "ragged", "cross")), (1, 1, 16, 16, ("single",))):
        for up in (True, False):
            for bias in (True, False):
                cs.append(StemCase(B, G, H, W, up, bias, props))
    cs.append(StemCase(5, 2, 64, 128, True, True, ("multi3", "ragged", "cross")))   # the production head count with three tiles: 320 on 128
    cs.append(StemCase(3, 16, 32, 48, False, True, ("multi3", "ragged", "cross"), impulse=True))
    return cs


STEM_CASES = _stem_cases()


# ------------------------------------------------------------------------------------------------
# stem: reference
# ------------------------------------------------------------------------------------------------
def stem_patches(img_z, kxn=7, cn=3, mode="constant"):
    """[H, W, 4] -> [H * W, 7 * kxn * cn]: the taps of every output pixel, k = (ky, kx, c); pixels outside the image are zero.
    (kxn = 8, cn = 4: the kernel's padded K order, whose extra taps meet zero weights.)"""
    H, W, _ = img_z.shape
    x = img_z.permute(2, 0, 1)[None]                                   # [1, 4, H, W]
    x = F.pad(x, (3, 3, 3, 3), mode=mode)
    x = F.pad(x, (0, kxn - 7, 0, 0))[0].permute(1, 2, 0)                # (the column the zero-weight tap kx = 7 reads)
    p = x.unfold(0, 7, 1).unfold(1, kxn, 1)                            # [H, W, 4, ky, kx]
    return p.permute(0, 1, 3, 4, 2)[..., :cn].reshape(H * W, 7 * kxn * cn)


def stem_weights(w, kxn=7, cn=3):
    """[G, 256, 3, 7, 7] -> [G, 256, 7 * kxn * cn] in the K order of stem_patches (zero at kx = 7 and c = 3)"""
    G_ = w.shape[0]
    wk = torch.zeros(G_, STEM_C, 7, kxn, cn, dtype=w.dtype)
    wk[:, :, :, :7, :3] = w.permute(0, 1, 3, 4, 2)
    return wk.reshape(G_, STEM_C, 7 * kxn * cn)


def up_coords64(n_out, n_src):
    f = torch.arange(n_out, dtype=torch.float64) * ((n_src - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = f.floor().long().clamp(max=n_src - 1)
    return f, i0, (i0 + 1).clamp(max=n_src - 1), f - i0


def lerp4(a, b, c_, d, ly, lx):
    """the bilinear form in the operation order of the ABI's definition (and of the kernel), in the operands' dtype"""
    return (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c_ + lx * d)


def stem_upsample64(c, src):
    """src [B, G, sh, sw, C] float64 -> [B, G, H, W, C]"""
    _, y0, y1, ly = up_coords64(c.H, c.sh)
    _, x0, x1, lx = up_coords64(c.W, c.sw)
    ly, lx = ly[:, None, None], lx[None, :, None]
    r0, r1 = src[:, :, y0], src[:, :, y1]
    return lerp4(r0[:, :, :, x0], r0[:, :, :, x1], r1[:, :, :, x0], r1[:, :, :, x1], ly, lx)


def _near_cells(n_out, n_src):
    """indices and 0/1 masks of the source rows (columns) whose |values| enter C for every output row: the cell of the float64
    coordinate, and its neighbour where the coordinate lies within the fp32 coordinate error of the cell boundary"""
    f, i0, i1, l = up_coords64(n_out, n_src)
    d = ((1 + U24) ** 2 - 1) * f
    idx = torch.stack(((i0 - 1).clamp(min=0), i0, i1, (i0 + 2).clamp(max=n_src - 1)))
    one = torch.ones_like(f)
    m = torch.stack(((l <= d).double(), one, one, ((1 - l) <= d).double()))
    return idx, m, d


def stem_corner_term(c, src_abs):
    """(dy + dx) C of the header: [B, G, H, W, C]"""
    yi, ym, dy = _near_cells(c.H, c.sh)
    xi, xm, dx = _near_cells(c.W, c.sw)
    rows = sum(ym[j][:, None, None] * src_abs[:, :, yi[j]] for j in range(4))            # [B, G, H, sw, C]
    C = sum(xm[j][:, None] * rows[:, :, :, xi[j]] for j in range(4))                      # [B, G, H, W, C]
    return (dy[:, None, None] + dx[None, :, None]) * C


STEM_BOUND = (STEM_KPAD + 1) * U24 + X3_TERM
_stem_cache = {}


def _stem_conv64(c, inp):
    """(conv without bias, sum |a||w|) [B, G, H, W, 256] float64: shared by the variants of a shape (one shape is kept)"""
    if _stem_cache.get("shape") != c.shape:
        w = stem_weights(inp["w_hi"].double() + inp["w_lo"].double())
        acc = torch.empty(c.B, c.G, c.H, c.W, STEM_C, dtype=torch.float64)
        S = torch.empty_like(acc)
        for b in range(c.B):
            for g in range(c.G):
                A = stem_patches(inp["img"][b, g].double())
                acc[b, g] = (A @ w[g].t()).view(c.H, c.W, STEM_C)
                S[b, g] = (A.abs() @ w[g].abs().t()).view(c.H, c.W, STEM_C)
        _stem_cache.clear()
        _stem_cache.update(shape=c.shape, acc=acc, S=S)
    return _stem_cache["acc"], _stem_cache["S"]


def stem_reference(c, inp):
    """dict(out, S, extra) [B, G, H, W, 256] float64 (extra: None without the upsample)"""
    acc, S = _stem_conv64(c, inp)
    if c.bias:
        b = inp["bias"].double()[None, :, None, None, :]
        acc, S = acc + b, S + b.abs()
    v, extra = acc.clamp_min(0), None
    if c.up:
        src = inp["up"].double()
        v = v + stem_upsample64(c, src)
        extra = UP_OPS * U24 * stem_upsample64(c, src.abs()) + stem_corner_term(c, src.abs())
    return dict(out=v, S=S, extra=extra)


# ------------------------------------------------------------------------------------------------
# proj: cases, inputs, reference
# ------------------------------------------------------------------------------------------------
class ProjCase:
    """x [B, G, M, K] -> out [B, G, M, N], Z = B * G.  dest: "dense"; "ldc88" / "ldc85" (row stride beyond N: 352-byte rows, and
    340-byte rows that are not 16-byte aligned); "zgap" (out_z_stride > M * ldc); "view" (G = 1: one head's slot of every batch item
    inside a [B, 2, M, N] buffer, the destination of the model's per-view launch).  props as StemCase's, on proj_grid."""

    def __init__(self, K, N, B, G, M, props, bias=True, dest="dense"):
        self.K, self.N, self.B, self.G, self.M, self.props, self.bias, self.dest = K, N, B, G, M, tuple(props), bias, dest
        self.Z = B * G
        self.id = f"proj-k{K}-n{N}-b{B}-g{G}-m{M}-{dest}" + ("" if bias else "-nobias")
        self.nwg, self.ntiles, self.rows = proj_grid(self.Z, M, K, N)
        self.ldc = {"ldc88": 88, "ldc85": 85}.get(dest, N)
        assert self.ldc >= N and (dest != "view" or G == 1)
        self.zs = M * self.ldc + (3 * self.ldc + 5 if dest == "zgap" else 0) if dest != "view" else 2 * M * N

    def check_props(self):
        per = tiles_per_wg(self.nwg, self.ntiles)
        if "single" in self.props:
            assert self.ntiles == 1, (self.id, self.ntiles)
        if "multi2" in self.props:
            assert max(per) >= 2, (self.id, per)
        if "multi3" in self.props:
            assert max(per) >= 3 and self.M % self.rows != 0, (self.id, per)
        if "ragged" in self.props:
            assert self.ntiles % self.nwg != 0, (self.id, self.nwg, self.ntiles)
        if "clamp" in self.props:
            assert CUS // self.Z < 1 and self.nwg == 1 and self.ntiles >= 2, (self.id, self.nwg, self.ntiles)
        if "zg" in self.props:   # z % G and z / G disagree somewhere, and do so inside the weight sets' range
            assert any(z % self.G != (z // self.G) % self.G for z in range(self.Z)), self.id
        return per

    def sentinel_steps(self):
        """first, second and last K step"""
        return [0, 1, self.K // 16 - 1]


def proj_inputs(c):
    """x [Z, M, K], W [G, N, K] with its planes, bias [G, N].  Sentinel rows of x (dense_gemm64.SENTINEL_ROWS and M - 1) and sentinel
    rows of W (columns of the output) are zero outside ONE K step, taken in turn from the first, the second and the last: a dropped or
    doubled step shows there at full scale."""
    g = torch.Generator().manual_seed(9500 + c.K + 17 * c.N + 3 * c.M + c.Z)
    x = _u(g, c.Z, c.M, c.K)
    W = _u(g, c.G, c.N, c.K, lo=-0.2, hi=0.2)
    steps, sent = c.sentinel_steps(), []
    rows = [r for r in dict.fromkeys(SENTINEL_ROWS + (c.M - 1,)) if r < c.M]
    cols = [n for n in dict.fromkeys(SENTINEL_ROWS + (c.N - 1,)) if n < c.N]
    for i, r in enumerate(rows):
        s = steps[i % 3]
        keep = x[:, r, 16 * s:16 * s + 16].clone()
        x[:, r] = 0
        x[:, r, 16 * s:16 * s + 16] = keep
        sent.append(("x", r, s))
    for i, n in enumerate(cols):
        s = steps[(i + len(rows)) % 3]
        keep = W[:, n, 16 * s:16 * s + 16].clone()
        W[:, n] = 0
        W[:, n, 16 * s:16 * s + 16] = keep
        sent.append(("w", n, s))
    hi, lo = split_w(W)
    return dict(x=x, W=W, w_hi=hi, w_lo=lo, bias=_u(g, c.G, c.N, lo=-2.0, hi=2.0), sentinels=sent)


def proj_bound(c):
    return c.K * U24 + X3_TERM


def proj_reference(c, inp):
    """dict(out, S) [Z, M, N] float64"""
    w = (inp["w_hi"].double() + inp["w_lo"].double())[[z % c.G for z in range(c.Z)]]      # [Z, N, K]
    x = inp["x"].double()
    out = torch.einsum("zmk,znk->zmn", x, w)
    S = torch.einsum("zmk,znk->zmn", x.abs(), w.abs())
    if c.bias:
        b = inp["bias"].double()[[z % c.G for z in range(c.Z)]][:, None, :]
        out, S = out + b, S + b.abs()
    return dict(out=out, S=S)


def _proj_cases():
    cs = []
    for (K, Ns) in ((128, (3, 4, 32)), (256, (65, 83, 96))):
        rows = PROJ_ROWS[K]
        for N in Ns:
            for M in (1, rows - 1):
                cs.append(ProjCase(K, N, 2, 2, M, ("single",)))
    for (K, M, Ns) in ((256, 1093, (83, 96)), (128, 2181, (3, 32))):
        for N in Ns:
            cs.append(ProjCase(K, N, 16, 2, M, ("multi3", "ragged", "zg")))
        cs.append(ProjCase(K, Ns[0], 16, 2, M, ("multi3", "ragged", "zg"), bias=False))
        cs.append(ProjCase(K, Ns[0], 16, 2, M, ("multi3", "ragged", "zg"), dest="zgap"))
        cs.append(ProjCase(K, Ns[0], 32, 1, M, ("multi3", "ragged"), dest="view"))
    cs.append(ProjCase(256, 83, 16, 2, 1093, ("multi3", "ragged", "zg"), dest="ldc88"))
    cs.append(ProjCase(256, 83, 16, 2, 1093, ("multi3", "ragged", "zg"), dest="ldc85", bias=False))
    cs.append(ProjCase(128, 3, 16, 2, 2181, ("multi3", "ragged", "zg"), dest="ldc85"))
    cs.append(ProjCase(256, 83, 129, 2, 70, ("clamp", "multi2", "zg")))      # Z = 258: 256 / Z < 1, one workgroup per z walks both tiles
    cs.append(ProjCase(128, 4, 129, 2, 130, ("clamp", "multi2", "zg")))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), ids
    return cs


PROJ_CASES = _proj_cases()
