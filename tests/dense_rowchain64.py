"""Dense float64 restatement of siu3r_rowchain_x3, written from the ABI comment of include/siu3r_hip.h (not from the kernel), with the
input generators, the per-stage scales and the bounds that tests/test_rowchain_ref.py (CPU) and tests/test_rowchain_gpu.py (GPU) share.

    y = x Wo^T + bo + res;  z = LN(y; g1, b1, eps1);  h = relu(z W1^T + c1);  o = h W2^T + c2 + z;  out = LN(o; g2, b2, eps2)
    LN(v; g, b, eps) = (v - mean) / sqrt(var + eps) * g + b,  mean = sum v / 256,  var = sum (v - mean)^2 / 256   (two passes)

Operands as the kernel sees them: the fp32 rows x and res; the matrices as the packed planes read back, hi + lo (ops.unpack_rowchain);
the fp32 vectors.

BOUNDS.  u = 2^-24 (dense_gemm64.U24), X3_TERM = 3 * 2^-16 (dense_gemm64.py's header: the two lo roundings and the dropped lo * lo).
  product stages (y, h, o), against an fp32 evaluation from the SAME stage input:  |got - ref| <= (K u + X3_TERM) S,
      S = sum_k |a||w| + |bias| (+ |residual|), K the inner dimension (256, 256, H).  ReLU is exact and 1-Lipschitz.
  LayerNorm stages, against an fp32 LayerNorm of the fp32-rounded stage input:  |got - ref| <= LN_TERM * (max_row|v - mean| rstd |g| + |b|)
      with LN_TERM = 512 u: the input rounding moves v - mean by at most 2 u max|v|; an fp32 sum of 256 terms in any order is within
      256 u of its scale, which bounds the mean and (relatively) the variance, so rstd is within (128 + 1) u; the remaining
      subtractions, products and the final addition are a handful of u.  For rows whose mean is large against their spread the first
      term is taken with max|v| in place of max|v - mean| (the rounding of v itself), which is what `ln_scale` does.

PARITY (GPU module): per row, e = max|got - ref| / max|ref| of the final output; e_fused <= 2 e_unfused + 256 * 2^-24.  Both
evaluate the same products in the same precision, only the summation orders differ.

No number here comes from a GPU run.  Not a test module."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_gemm64 import U24, X3_TERM  # noqa: E402

D = 256
LN_TERM = 512 * U24
PARITY_ADD = 256 * 2.0 ** -24
FILL_BITS = 0x7FA5C3D2       # one NaN bit pattern around every input
SENTINEL = -777.25           # the fill of the output buffer (never a LayerNorm result of these inputs)
GUARD = 64                   # floats of guard band on either side of a carved tensor (keeps 16-byte alignment)
MS = (1, 33, 64, 65, 129)
HS = (256, 512, 1024)
KINDS = ("normal", "offset")


def make_weights(H, kind, seed=0):
    """fp32 CPU weights of one layer.  gamma / beta are not constant.  kind "offset": the first LayerNorm shifts every row to mean 50
    (b1) with a small gain (g1), so that the second LayerNorm meets a large mean as well."""
    g = torch.Generator().manual_seed(4100 + H + seed)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    w = dict(wo=r(D, D) / 16, bo=r(D), g1=1 + 0.5 * r(D), b1=0.5 * r(D), w1=r(H, D) / 16, c1=0.5 * r(H), w2=r(D, H) / 32, c2=r(D),
             g2=1 + 0.5 * r(D), b2=0.5 * r(D))
    if kind == "offset":
        w["g1"] = 0.5 * w["g1"]
        w["b1"] = 50 + w["b1"]
    return w


def make_rows(M, kind, seed=0):
    """(x, res) fp32 [M, 256].  "normal": seeded normal rows.  "offset": every row of the residual stream has mean 50 and standard
    deviation 0.5 (a one-pass E[v^2] - E[v]^2 variance loses all its digits there)."""
    g = torch.Generator().manual_seed(7300 + 13 * M + seed)
    x, res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    if kind == "offset":
        x, res = 0.5 * x, 50 + 0.5 * res
    return x, res


def ln64(v, g, b, eps):
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * g.double() + b.double()


def ln_scale(v, g, b, eps):
    """the scale of the LayerNorm bound, [M, 256] float64"""
    mean = v.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + eps)
    return v.abs().amax(-1, keepdim=True) * rstd * g.double().abs() + b.double().abs()


def chain64(x, res, w, eps1=1e-5, eps2=1e-5):
    """w: ops.unpack_rowchain(pack, H) (float64 matrices, fp32 vectors).  Every stage and the product stages' scales, float64."""
    x, res = x.double(), res.double()
    wo, w1, w2 = w["wo"].double(), w["w1"].double(), w["w2"].double()
    bo, c1, c2 = w["bo"].double(), w["c1"].double(), w["c2"].double()
    y = x @ wo.t() + bo + res
    z = ln64(y, w["g1"], w["b1"], eps1)
    h = torch.relu(z @ w1.t() + c1)
    o = h @ w2.t() + c2 + z
    out = ln64(o, w["g2"], w["b2"], eps2)
    return dict(y=y, z=z, h=h, o=o, out=out,
                S_y=x.abs() @ wo.abs().t() + bo.abs() + res.abs(), S_h=z.abs() @ w1.abs().t() + c1.abs(),
                S_o=h.abs() @ w2.abs().t() + c2.abs() + z.abs())


def product_bound(K):
    return K * U24 + X3_TERM


def row_error(got, ref):
    """per row: max|got - ref| / max|ref|, float64 [M]"""
    return (got.double() - ref).abs().amax(-1) / ref.abs().amax(-1)


def rowchain_ok_restated(x, res, split):
    """ops.rowchain_ok restated by hand: bf16x3 only, fp32, contiguous, 256 columns, one shape"""
    for t in (x, res):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 2 or t.shape[-1] != D:
            return False
    return bool(split) and x.shape == res.shape
