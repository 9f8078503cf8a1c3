"""Dense float64 restatement of siu3r_gemm (include/siu3r_hip.h), written from the ABI's definition, plus the per-element comparison, the
input generator, the buffer layouts and the case list that tests/test_gemm_ref.py (CPU) and tests/test_gemm_gpu.py (GPU) share.

    C[z, m, n] = epilogue( sum_k A[z, m, k] W[zw, n, k] )

A addressing: dense rows (a_mode 0), the NHWC gather of a convolution (a_mode 1: row m = (b, oy, ox), k = (ky, kx, c), taps outside the
image are zero), the 16 x 16 patchify of an NCHW image (a_mode 2: k = (c, ky, kx)); relu_in clamps A at zero.  Epilogue, in this order:
bias (out_mode 1: per output channel) or the folded LayerNorm rstd (acc - mean c1) + c2; RoPE2D on the first rope_ncols columns (heads
of 64 laid out [u_Y v_Y u_X v_X], (u, v) -> (u c - v s, v c + u s)); activation (exact-erf GELU / ReLU); the bilinear x2
(align_corners) upsample-add of up_src; the residual; then the row statistics of that value (stats_out: per 64-column tile the mean and
the centred sum of squares), the store (row-major, or the pixel shuffle of out_mode 1), its bf16 copy c_aux and its planes c_x3.

The reference receives the operands as the kernel sees them: the bf16 values for bf16 A; the fp32 values for bf16x3; for fp32 A without
the split the value rounded to bf16 with round-to-nearest-even (the only kernels that take such a launch are the register-staged ones
of gemm.hip: pack_bf16x8 -> v_cvt_pk_bf16_f32; the LDS-DMA, ping-pong and skinny kernels refuse fp32 A without w_x3).  The weights
are the packed w_hi (+ w_lo) read back.

A[m, k .. kpad) MAY be fetched and multiplied by the zero padding of W: gemm_dma_x3_kernel masks the K tail only when k % 32 != 0, so at
k % 64 == 32 it reads the 32 elements behind every row but the last (inside the operand's extent), and every kernel does when the
caller packs W with a kpad beyond the next multiple of 64.  The device tests therefore fill those positions with a large FINITE value
(times zero = zero) and everything else around A with NaN.

Every value carries its scale S[z, m, n], the magnitude the rounding errors of its computation are proportional to: sum_k |a||w| + |bias|
(LayerNorm fold: rstd sum_k |a||w'| + |c2|), times 1.13 (the Lipschitz bound of GELU) behind a GELU, S_u |c| + S_v |s| behind RoPE, plus
the interpolated |up_src|, plus |residual|.  assert_elems_close holds every element to |out - ref| <= bound * S.  bound(case) is derived:
    K 2^-24                 fp32 accumulation of K products in any order
  + 3 * 2^-16  (bf16x3)     the two lo roundings and the dropped lo * lo product (each 2^-16 for round-to-nearest planes.  The ping-pong
                            and LDS-DMA kernels TRUNCATE A's hi plane, whose worst case is 5 * 2^-16; the errors of a row's products do
                            not align, the faithful emulation of test_gemm_ref.py stays below half of 3 * 2^-16, and the figure stays)
  + GELU_FAST_REL (GELU)    the polynomial of gemm_epilogue.h against the exact erf form, relative to |x| <= S
and, on top, one bf16 rounding (2^-8, round-to-nearest-even: store8_from_f32 / pack_bf16x2) of the value for a bf16 C or c_aux.

Not a test module."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
BF16_U = 2.0 ** -8          # unit roundoff of bf16 (8 significant bits), round-to-nearest-even
X3_TERM = 3 * 2.0 ** -16
PLANES_REL = 2.0 ** -15     # |hi + lo - out| <= 2^-15 |out|: hi = the upper 16 bits (|out - hi| < 2^-7 |out|), lo = bf16(out - hi)
GELU_LIP = 1.13             # max |GELU'| = 1.1289
# gelu_fast (csrc/gemm_epilogue.h) against 0.5 x (1 + erf(x / sqrt 2)), relative to |x|, over [-8, 8]: measured by
# test_gemm_ref.py::test_gelu_fast_constant with a float32 restatement of the polynomial (exact reciprocal), plus one ulp (2^-23 of
# erf's complement <= 1, halved by the 0.5) for the device reciprocal, which is specified to 1 ulp and not bit-exactly; margin 2x.
GELU_FAST_MEASURED = 9.1e-7
GELU_FAST_REL = 2.0 * (GELU_FAST_MEASURED + 2.0 ** -24)
A_TAIL_FILL = 30000.0       # finite fill of A[m, k .. kpad): see the header
ROPE_MAX_POS = 23
SENTINEL_ROWS = (0, 31, 32, 127, 128, 255, 256)

MODES = ("bf16", "f32", "bf16x3")
TILES = {1: (256, 256), 2: (256, 128), 3: (128, 128), -1: (128, 64)}


def rne_bf16(x):
    return x.float().to(torch.bfloat16).float()


def trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def split_planes(x):
    """fp32 [..., C] (C % 32 == 0) -> the pre-split planes of siu3r_gemm_params.c_x3 / a_x3 as an fp32-typed tensor of the same shape: per
    32 columns [hi 32 | lo 32] bf16, hi = the upper 16 bits, lo = bf16(x - hi)"""
    x = x.float().contiguous()
    hi = trunc_bf16(x)
    lo = (x - hi).to(torch.bfloat16)
    hi16 = (x.view(torch.int32) >> 16).to(torch.int16)
    lead, C = x.shape[:-1], x.shape[-1]
    pl = torch.stack((hi16.view(*lead, C // 32, 32), lo.view(torch.int16).view(*lead, C // 32, 32)), dim=-2)
    return pl.reshape(*lead, 2 * C).view(torch.float32)


def join_planes(p):
    """inverse of split_planes: (hi, lo) as fp32 tensors of p's shape"""
    p = p.contiguous()
    lead, C = p.shape[:-1], p.shape[-1]
    h = p.view(torch.int16).view(*lead, C // 32, 2, 32)
    f = lambda t: (t.to(torch.int32) << 16).view(torch.float32).reshape(*lead, C)
    return f(h[..., 0, :].contiguous()), f(h[..., 1, :].contiguous())


def gelu_fast32(x):
    """float32 restatement of siu3r_epi::gelu_fast (the same operations in the same order, an exact division for the reciprocal)"""
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    ax = np.abs(x)
    co = [f(4.30638e-5) * f(0.125), f(2.765672e-4) * f(0.17677669529663687), f(1.520143e-4) * f(0.25), f(9.2705272e-3) * f(0.35355339059327373),
          f(4.22820123e-2) * f(0.5), f(7.05230784e-2) * f(0.70710678118654752), f(1.0)]
    with np.errstate(over="ignore"):
        q = np.full_like(ax, co[0])
        for cf in co[1:]:
            q = (q * ax + cf).astype(np.float32)
        for _ in range(4):
            q = (q * q).astype(np.float32)
        e = (f(1.0) - (f(1.0) / q).astype(np.float32)).astype(np.float32)
    return (f(0.5) * ((ax * e).astype(np.float32) + x).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def _tf(b):
    return "true" if b else "false"


def k_pp(x3, cfg, mode=0, relu=False, lnf=False, aps=False):
    MI, NJ = {1: (2, 4), 2: (2, 2), 3: (1, 2)}[cfg]
    return f"siu3r_gemm_pp::gemm_pp_kernel<{_tf(x3)}, {MI}, {NJ}, {mode}, {_tf(relu)}, {_tf(lnf)}{', true' if aps else ''}>"


def k_dma(mode=0, relu=False, lnf=False, ni=1, ks=2):
    return f"siu3r_gemm_dma::gemm_dma_kernel<{ni}, {mode}, {_tf(relu)}, {ks}, {_tf(lnf)}>"


def k_dmax(mode=0, relu=False, lnf=False, ks=2):
    return f"siu3r_gemm_dma::gemm_dma_x3_kernel<{mode}, {_tf(relu)}, {ks}, {_tf(lnf)}>"


def k_staged(a_f32, split, lnf=False, ni=1):
    return f"gemm_kernel<{a_f32}, {split}, {ni}{', true' if lnf else ''}>"


class Conv:
    def __init__(self, B, ih, iw, cin, kh, stride, pad, real_cin=None):
        self.B, self.ih, self.iw, self.cin, self.kh, self.kw, self.stride, self.pad = B, ih, iw, cin, kh, kh, stride, pad
        self.oh, self.ow = (ih + 2 * pad - kh) // stride + 1, (iw + 2 * pad - kh) // stride + 1
        self.real_cin = real_cin or cin  # channels beyond it are layout padding: zero in the image


class Case:
    """One launch: problem, options, buffer placement, and the plan it must get."""

    def __init__(self, name, mode, m, n, k, kernel, tile, *, splitk=1, skinny=0, path=0, conv=None, patch=None, relu_in=False, ln=False,
                 act=0, res=None, c_bf16=False, rope=0, stats=False, aux=False, up_src=None, shuffle=None, planes=None, a_x3=False, batch=0,
                 bmod=0, flip=False, force=None, tune=None, env=None, c_off=0, r_off=0, ldc_odd=False, w_x3=True, bias=True, kpad=None, smap=None):
        assert mode in MODES
        self.name, self.mode, self.m, self.n, self.k, self.kpad = name, mode, m, n, k, kpad or (k + 63) // 64 * 64
        self.smap = smap                                       # out_mode 1: (B, IH, IW) of the rows; shuffle = (up, cout)
        self.kernel, self.tile, self.splitk, self.skinny, self.path = kernel, tile, splitk, skinny, path
        self.conv, self.patch, self.relu_in, self.ln, self.act, self.res, self.c_bf16 = conv, patch, relu_in, ln, act, res, c_bf16
        self.rope, self.stats, self.aux, self.up_src, self.shuffle = rope, stats, aux, up_src, shuffle
        self.planes, self.a_x3, self.batch, self.bmod, self.flip = planes, a_x3, batch, bmod, flip  # planes: None or (col0, "sep" | "same" | "only")
        self.force = tile if force is None else force          # siu3r_gemm_params.tile_cfg
        self.tune = dict(tune or {})                           # siu3r_gemm_tune keys for this case, on top of key 3 = 1 (no table)
        self.env = env                                         # the A/B switches this case needs ("A=1" or "A=1,B=0"), or None
        self.c_off, self.r_off, self.ldc_odd, self.w_x3 = c_off, r_off, ldc_odd, w_x3  # byte offsets off a 16-byte line; w_x3: attach the interleaved planes
        self.bias = bias and not ln
        self.a_mode = 1 if conv else 2 if patch else 0
        self.x3 = mode == "bf16x3"
        self.Z = batch if batch > 0 else 1
        self.G = bmod if bmod > 0 else 1
        # weight sets: one per inner index (two-level); one per batch item (one-level; shared under a folded LayerNorm, whose c1 is not batched)
        self.wn = self.G if bmod else (self.Z if batch and not ln else 1)
        self.id = name

    @property
    def step(self):
        return 16 if self.mode == "bf16x3" else 32

    @property
    def bm(self):
        return TILES[self.tile][0]

    def slice_starts(self):
        """first k of every split-K slice (ping-pong: phases of 1 or 2 steps; LDS-DMA: K tiles of 64 bf16 / 32 fp32)"""
        if self.splitk <= 1:
            return [0]
        unit = {1: self.step, 2: 2 * self.step, 3: 2 * self.step, -1: 64 if self.mode == "bf16" else 32}[self.tile]
        units = self.kpad // unit
        return [j * units // self.splitk * unit for j in range(self.splitk)]

    def sentinel_steps(self):
        """the K steps a fault is most likely in: first, second, last full one, the ragged tail, either side of every slice boundary"""
        st, ns = self.step, (self.k + self.step - 1) // self.step
        want = [0, 1, self.k // st - 1]
        if self.k % 64:
            want.append((self.k - 1) // st)
        for s0 in self.slice_starts()[1:]:
            want += [s0 // st - 1, s0 // st]
        return [s for s in dict.fromkeys(want) if 0 <= s < ns]

    def zsplit(self, z):
        return (z // self.G, z % self.G) if self.bmod else (z, 0)

    def a_index(self, z):
        """the stored A block that batch item z reads (two-level flip: the other inner index)"""
        zo, zi = self.zsplit(z)
        return zo * self.G + (self.G - 1 - zi if self.flip else zi) if self.bmod else z

    def w_index(self, z):
        return self.zsplit(z)[1] if self.bmod else (z if self.wn > 1 else 0)

    def bias_index(self, z):
        return self.zsplit(z)[1] if self.bmod else 0


def _ceil(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _u(g, *shape, lo=-1.0, hi=1.0):
    return (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)).float()


def make_inputs(c, seed=0, chain=None):
    """Seeded CPU inputs of a case as float32 tensors holding what the kernel is handed (bf16 tensors already rounded):
    A [Z, M, K] (dense; stored order) or img; W [wn, N, K] with its packed planes w_hi / w_lo [wn, N, kpad]; bias / ln_c1 / ln_c2 [G, N];
    ln_part [Z, M, tiles, 2] (fp32 partial statistics of the rows A was rounded from, stored order); residual [Z, M, N] (logical order);
    rope_cos / rope_sin [max_pos, 16], rope_pos [Z * M, 2]; up [B, oh / 2, ow / 2, N].
    chain = (rows fp32 [Z, M, K], their partial statistics [Z, M, tiles, 2]): a folded-LayerNorm case takes its A operand and ln_part
    from a producer's output and stats_out instead of generating them."""
    g = torch.Generator().manual_seed(7000 + seed)
    Z, M, N, K = c.Z, c.m, c.n, c.k
    st = c.step
    inp = {}
    a_dt = (lambda t: rne_bf16(t)) if c.mode == "bf16" else (lambda t: t)
    if c.a_mode == 0:
        A32 = _u(g, Z, M, K) + (0.25 if c.ln else 0.0)  # (LayerNorm: a mean worth subtracting)
        steps = c.sentinel_steps()
        rows = [r for r in dict.fromkeys(SENTINEL_ROWS + (M - 1,)) if r < M]
        inp["sentinels"] = []
        for i, r in enumerate(rows):  # sentinel rows: zero outside one K step
            s = steps[i % len(steps)]
            keep = A32[:, r, s * st:min(K, (s + 1) * st)].clone()
            A32[:, r] = 0
            A32[:, r, s * st:min(K, (s + 1) * st)] = keep
            inp["sentinels"].append(("a", r, s))
        if chain is not None:
            A32, inp["sentinels"] = chain[0].float().clone(), []
        if c.ln:
            T = (K + 63) // 64
            part = torch.zeros(Z, M, T, 2)
            for t in range(T):
                blk = A32[..., 64 * t:min(K, 64 * t + 64)].double()
                mu = blk.mean(-1)
                part[..., t, 0], part[..., t, 1] = mu.float(), ((blk - mu[..., None]) ** 2).sum(-1).float()
            inp["ln_part"] = part if chain is None else chain[1].float().clone()
            inp["ln_mean"] = A32.double().mean(-1)
            inp["ln_rstd"] = 1.0 / torch.sqrt(A32.double().var(-1, unbiased=False) + float(np.float32(1e-6)))
        inp["A"] = a_dt(A32)
    elif c.a_mode == 1:
        cv = c.conv
        img = _u(g, cv.B, cv.ih, cv.iw, cv.cin)
        img[..., cv.real_cin:] = 0
        inp["img"] = a_dt(img)
    else:
        B, H, W_ = c.patch
        inp["img"] = _u(g, B, 3, H, W_)
    W = _u(g, c.wn, N, K)
    steps = c.sentinel_steps()
    cols = [r for r in dict.fromkeys(SENTINEL_ROWS + (N - 1,)) if r < N]
    n_rows = len(inp.get("sentinels", []))
    for i, n_ in enumerate(cols):  # sentinel columns: rows of W, zero outside one K step (they go on where the rows' steps end)
        s = steps[(i + n_rows) % len(steps)]
        keep = W[:, n_, s * st:min(K, (s + 1) * st)].clone()
        W[:, n_] = 0
        W[:, n_, s * st:min(K, (s + 1) * st)] = keep
        inp.setdefault("sentinels", []).append(("w", n_, s))
    hi = torch.zeros(c.wn, N, c.kpad)
    lo = torch.zeros(c.wn, N, c.kpad)
    hi[..., :K] = rne_bf16(W)
    if c.mode == "bf16x3":
        lo[..., :K] = rne_bf16(W - hi[..., :K])
    inp["W"], inp["w_hi"], inp["w_lo"] = W, hi, lo
    nb = c.shuffle[1] if c.shuffle else N
    if c.ln:
        inp["ln_c1"] = (hi + lo).double().sum(-1).float()   # [wn, N]: of the rounded operand
        inp["ln_c2"] = _u(g, c.wn, N)
    elif c.bias:
        inp["bias"] = _u(g, c.G, nb, lo=-2.0, hi=2.0)
    if c.res:
        r = _u(g, Z, M, N, lo=-2.0, hi=2.0)
        inp["residual"] = rne_bf16(r) if c.res == "bf16" else r
    if c.rope:
        inv = 1.0 / torch.pow(torch.tensor(100.0), torch.arange(16, dtype=torch.float32) / 16)
        ang = torch.arange(ROPE_MAX_POS, dtype=torch.float32)[:, None] * inv[None, :]
        inp["rope_cos"], inp["rope_sin"] = torch.cos(ang), torch.sin(ang)
        pos = torch.randint(0, ROPE_MAX_POS, (Z * M, 2), generator=g)
        pos[0], pos[-1] = torch.tensor([0, ROPE_MAX_POS - 1]), torch.tensor([ROPE_MAX_POS - 1, 0])
        inp["rope_pos"] = pos
    if c.up_src:
        cv = c.conv
        u = _u(g, cv.B, cv.oh // 2, cv.ow // 2, N, lo=-2.0, hi=2.0)
        inp["up"] = rne_bf16(u) if c.up_src == "bf16" else u
    return inp


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def gather_rows(c, inp, dt=torch.float64):
    """the logical A operand [Z, M, K] of every batch item, as the kernel sees it (rounded when it rounds, ReLU'd when it clamps)"""
    if c.a_mode == 0:
        A = inp["A"][[c.a_index(z) for z in range(c.Z)]]
    elif c.a_mode == 1:
        cv = c.conv
        x = torch.nn.functional.pad(inp["img"], (0, 0, cv.pad, cv.pad, cv.pad, cv.pad))                 # [B, IH + 2p, IW + 2p, C]
        rows = []
        for ky in range(cv.kh):
            for kx in range(cv.kw):
                rows.append(x[:, ky:ky + cv.stride * (cv.oh - 1) + 1:cv.stride, kx:kx + cv.stride * (cv.ow - 1) + 1:cv.stride, :])
        A = torch.stack(rows, dim=3).reshape(1, cv.B * cv.oh * cv.ow, cv.kh * cv.kw * cv.cin)        # k = (ky, kx, c)
    else:
        B, H, W_ = c.patch
        x = inp["img"].view(B, 3, H // 16, 16, W_ // 16, 16).permute(0, 2, 4, 1, 3, 5)                 # [B, h, w, c, ky, kx]
        A = x.reshape(1, B * (H // 16) * (W_ // 16), 768)
    if c.mode == "f32":
        A = rne_bf16(A)
    if c.relu_in:
        A = A.clamp_min(0)
    return A.to(dt)


def weights(c, inp, dt=torch.float64):
    """[Z, N, K]: the packed planes read back"""
    w = (inp["w_hi"].double() + inp["w_lo"].double())[..., :c.k]
    return w[[c.w_index(z) for z in range(c.Z)]].to(dt)


def upsample2(c, src):
    """bilinear x2, align_corners: src [B, sh, sw, N] -> [1, B * oh * ow, N]"""
    cv = c.conv
    sh, sw = cv.oh // 2, cv.ow // 2
    fy = torch.arange(cv.oh, dtype=src.dtype) * ((sh - 1) / (cv.oh - 1) if cv.oh > 1 else 0.0)
    fx = torch.arange(cv.ow, dtype=src.dtype) * ((sw - 1) / (cv.ow - 1) if cv.ow > 1 else 0.0)
    y0, x0 = fy.floor().long().clamp(max=sh - 1), fx.floor().long().clamp(max=sw - 1)
    y1, x1 = (y0 + 1).clamp(max=sh - 1), (x0 + 1).clamp(max=sw - 1)
    ly, lx = (fy - y0)[None, :, None, None], (fx - x0)[None, None, :, None]
    top = src[:, y0][:, :, x0] * (1 - lx) + src[:, y0][:, :, x1] * lx
    bot = src[:, y1][:, :, x0] * (1 - lx) + src[:, y1][:, :, x1] * lx
    return (top * (1 - ly) + bot * ly).reshape(1, cv.B * cv.oh * cv.ow, -1)


def _gelu(x):
    if x.dtype == torch.float64:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return torch.from_numpy(gelu_fast32(x.numpy()))


def epilogue(c, inp, acc, S, mut=None):
    """acc, S [Z, M, N] -> dict(out, S, stats [Z, M, tiles, 2], stats_S) in acc's dtype (float64: the reference; float32: the emulation
    of test_gemm_ref.py, whose wrong answers are the `mut` branches)"""
    dt = acc.dtype
    Z, M, N = acc.shape
    bi = [c.bias_index(z) for z in range(Z)]
    ncol = torch.arange(N)
    last_tile = ncol >= (N - 1) // 64 * 64
    if c.ln:
        mean, rstd = inp["ln_mean"].to(dt)[[c.a_index(z) for z in range(Z)]], inp["ln_rstd"].to(dt)[[c.a_index(z) for z in range(Z)]]
        c1, c2 = inp["ln_c1"].to(dt)[bi][:, None, :], inp["ln_c2"].to(dt)[bi][:, None, :]
        v = rstd[..., None] * (acc - mean[..., None] * c1) + c2
        S = rstd[..., None] * S + c2.abs()
    elif c.bias:
        b = inp["bias"].to(dt)[bi]                                   # [Z, nb]
        b = b[:, ncol % c.shuffle[1]] if c.shuffle else b
        if mut == "bias_shift":
            b = torch.where(last_tile[None, :], torch.roll(b, -1, dims=1), b)
        v, S = acc + b[:, None, :], S + b.abs()[:, None, :]
    else:
        v = acc.clone()
    if c.rope:
        nc = c.rope + (64 if mut == "rope_head" else 0)
        pos = inp["rope_pos"].view(Z, M, 2)
        x, Sx = v[..., :nc].reshape(Z, M, nc // 64, 4, 16).clone(), S[..., :nc].reshape(Z, M, nc // 64, 4, 16).clone()
        o, So = torch.empty_like(x), torch.empty_like(Sx)
        for ax in range(2):
            cs = inp["rope_cos"].to(dt)[pos[..., ax]][:, :, None, :]
            sn = inp["rope_sin"].to(dt)[pos[..., ax]][:, :, None, :] * (-1.0 if mut == "rope_sign" else 1.0)
            u, w = x[..., 2 * ax, :], x[..., 2 * ax + 1, :]
            o[..., 2 * ax, :], o[..., 2 * ax + 1, :] = u * cs - w * sn, w * cs + u * sn
            Su, Sw = Sx[..., 2 * ax, :], Sx[..., 2 * ax + 1, :]
            So[..., 2 * ax, :], So[..., 2 * ax + 1, :] = Su * cs.abs() + Sw * sn.abs(), Sw * cs.abs() + Su * sn.abs()
        v, S = v.clone(), S.clone()
        v[..., :nc], S[..., :nc] = o.reshape(Z, M, nc), So.reshape(Z, M, nc)
    res = None
    if c.res:
        res = inp["residual"].to(dt)
        if mut == "res_shift":  # rows of the stub row tile read the residual one row further
            stub = torch.arange(M) >= (M - 1) // c.bm * c.bm
            res = torch.where(stub[None, :, None], torch.roll(res, -1, dims=1), res)
        if mut == "res_first":
            v = v + res
    if c.act == 1:
        v, S = _gelu(v), S * GELU_LIP
    elif c.act == 2:
        v = v.clamp_min(0)
    if c.up_src:
        v, S = v + upsample2(c, inp["up"].to(dt)), S + upsample2(c, inp["up"].to(dt).abs())
    pre = v
    if res is not None and mut != "res_first":
        v = v + res
    if res is not None:
        S = S + res.abs()
    out = dict(out=v, S=S)
    if c.stats:
        sv = pre if mut == "stats_pre" else v
        T = (N + 63) // 64
        stt, stS = torch.zeros(Z, M, T, 2, dtype=dt), torch.zeros(Z, M, T, 2, dtype=dt)
        for t in range(T):
            blk, bS = sv[..., 64 * t:min(N, 64 * t + 64)], S[..., 64 * t:min(N, 64 * t + 64)]
            mu = blk.mean(-1)
            d = blk - mu[..., None]
            stt[..., t, 0], stt[..., t, 1] = mu, (d * d).sum(-1)
            # d mean = mean of the element errors; d M2 = 2 sum (v - mean) dv to first order (the shift of the mean drops out), plus the
            # fp32 summation of <= 64 squares: 2 M2 on the same bound, which is at least 64 * 2^-24
            stS[..., t, 0], stS[..., t, 1] = bS.mean(-1), 2.0 * (d.abs() * bS).sum(-1) + 2.0 * stt[..., t, 1]
        out.update(stats=stt, stats_S=stS)
    return out


def reference(c, inp):
    A, W = gather_rows(c, inp), weights(c, inp)
    acc = torch.einsum("zmk,znk->zmn", A, W)
    S = torch.einsum("zmk,znk->zmn", A.abs(), W.abs())
    return epilogue(c, inp, acc, S)


def shuffle_out(c, x):
    """[1, B * IH * IW, up * up * cout] -> [B, IH * up, IW * up, cout]: the pixel shuffle of out_mode 1"""
    up, co = c.shuffle
    B, ih, iw = c.smap
    return x.reshape(B, ih, iw, up, up, co).permute(0, 1, 3, 2, 4, 5).reshape(B, ih * up, iw * up, co)


def unshuffle_out(c, y):
    up, co = c.shuffle
    B, ih, iw = c.smap
    return y.reshape(B, ih, up, iw, up, co).permute(0, 1, 3, 2, 4, 5).reshape(1, B * ih * iw, up * up * co)


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def bound(c):
    b = c.k * U24
    if c.mode == "bf16x3":
        b += X3_TERM
    if c.act == 1:
        b += GELU_FAST_REL
    return b


def worst_ratio(out, ref, S, bnd, extra=None):
    """max over the elements of |out - ref| / (bnd * S + extra) and its index; a non-finite output is infinite error"""
    out, ref, S = out.double(), ref.double(), S.double()
    assert out.shape == ref.shape == S.shape, (out.shape, ref.shape, S.shape)
    lim = bnd * S + (extra.double() if extra is not None else 0.0)
    err = (out - ref).abs()
    ratio = err / lim.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(out), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, ratio.shape))
    return float(ratio.flatten()[i]), idx


def assert_elems_close(out, ref, S, bnd, *, extra=None, name="", quiet=False, what="c"):
    """|out - ref| <= bnd * S (+ extra) for every element of [Z, M, N]; names the worst (z, m, n); returns its ratio to the bound"""
    w, idx = worst_ratio(out, ref, S, bnd, extra)
    o, r, s = (float(t.double()[idx]) for t in (out, ref, S))
    if not quiet:
        print(f"[parity] {name}: {what} worst (z, m, n) = {idx}: |out - ref| = {abs(o - r):.3e} = {w:.3f} of the bound {bnd:.2e} * S (out {o:+.7e} ref {r:+.7e} S {s:.4e})")
    assert w <= 1.0, f"{name}: {what}{idx}: |out - ref| = {abs(o - r):.3e} is {w:.2f} x the bound {bnd:.2e} * S = {bnd * s:.3e} (out {o!r} ref {r!r})"
    return w


def bf16_extra(ref, S, bnd):
    """one round-to-nearest-even bf16 rounding of the value the kernel holds (within bnd * S of ref)"""
    return BF16_U * (ref.abs() + bnd * S)


def check_planes(buf, col0, *, c32=None, ref=None, S=None, bnd=None, name=""):
    """buf [Z, M, N] fp32-typed plane storage.  Columns >= col0: hi must be the upper 16 bits of the fp32 output exactly (c32, when the
    launch also wrote it there) and |hi + lo - out| <= 2^-15 |out|; without an fp32 output hi + lo is held to the element bound plus
    that rounding, and lo must be a residual of hi's truncation (same sign, below one bf16 step).  Returns the worst ratio."""
    hi, lo = join_planes(buf[..., col0:])
    if c32 is not None:
        want = trunc_bf16(c32[..., col0:])
        bad = (hi.view(torch.int32) != want.view(torch.int32))
        assert not bad.any(), f"{name}: hi plane differs from the upper 16 bits of the fp32 output at {tuple(int(i) for i in bad.nonzero()[0])} (+ column {col0})"
        d = (hi.double() + lo.double() - c32[..., col0:].double()).abs()
        lim = PLANES_REL * c32[..., col0:].double().abs()
        assert (d <= lim).all(), f"{name}: |hi + lo - out| > 2^-15 |out| at {tuple(int(i) for i in (d > lim).nonzero()[0])}"
    w = 0.0
    if ref is not None:
        r, s = ref[..., col0:], S[..., col0:]
        w = assert_elems_close(hi.double() + lo.double(), r, s, bnd, extra=PLANES_REL * (r.abs() + bnd * s), name=name, what="planes")
        step = hi.abs().double() * 2.0 ** -7
        ok = (lo.double().abs() <= step) & ((lo == 0) | (hi == 0) | (torch.sign(lo) == torch.sign(hi)))
        assert ok.all(), f"{name}: lo is not the residual of a truncated hi at {tuple(int(i) for i in (~ok).nonzero()[0])}"
    return w


def untouched(parent, fill_bits, written):
    """every element of the flat int-typed `parent` outside the boolean mask `written` still holds fill_bits; returns the first offenders"""
    bad = (parent != fill_bits) & ~written
    return [int(i) for i in bad.nonzero().flatten()[:8]]


# ------------------------------------------------------------------------------------------------
# buffer placement (shared by the host-only plan query of test_gemm_ref.py and the device tensors of test_gemm_gpu.py)
# ------------------------------------------------------------------------------------------------
class Rows:
    """A [Z, M, cols] view with row stride ld > cols inside a flat parent of `numel` elements: slot (z) of M + 3 rows each, one spare
    slot behind the last, `off` elements in front (off * esz bytes = a multiple of 128 plus the case's offset)."""

    def __init__(self, c, cols, esz, off_bytes=0, odd_ld=False, two_level=None):
        self.cols, self.esz = cols, esz
        self.ld = _ceil(cols, 32) + (33 if odd_ld else 32)
        self.rows = c.m + 3
        self.Z, self.M = c.Z, c.m
        self.off = 128 // esz + off_bytes // esz
        self.sz = self.rows * self.ld                      # elements between consecutive slots
        self.numel = self.off + (c.Z + 1) * self.sz + 64
        if c.bmod:
            self.s_o, self.s_i = c.G * self.sz, self.sz
        else:
            self.s_o, self.s_i = (self.sz if c.batch else 0), 0

    def index(self):
        """flat parent index of every view element [Z, M, cols]"""
        z, m, n = torch.arange(self.Z)[:, None, None], torch.arange(self.M)[None, :, None], torch.arange(self.cols)[None, None, :]
        return self.off + z * self.sz + m * self.ld + n


def layouts(c):
    """name -> Rows for the row-major buffers of the case"""
    L = {}
    a_esz = 2 if c.mode == "bf16" else 4
    if c.a_mode == 0:
        L["a"] = Rows(c, c.k, a_esz, 0 if c.a_x3 else 16)
    if not c.shuffle:
        L["c"] = Rows(c, c.n, 2 if c.c_bf16 else 4, c.c_off, c.ldc_odd)
        if c.res:
            L["r"] = Rows(c, c.n, 2 if c.res == "bf16" else 4, c.r_off, c.ldc_odd)
        if c.aux:
            L["aux"] = Rows(c, c.n, 2, c.c_off // 2, c.ldc_odd)
        if c.planes and c.planes[1] != "same":
            L["x3"] = Rows(c, c.n, 4, 0)
    return L


def expect_c_x3_ok(c):
    """wave_rows' conditions for the fp32 fast row pass (csrc/gemm_epilogue_pp.h), restated on the case: what siu3r_gemm_plan_t.c_x3_ok
    must say for a ping-pong plan"""
    if c.tile < 0 or c.shuffle or c.aux or c.c_bf16 or c.n % 64 or c.c_off % 16 or c.ldc_odd:
        return 0
    if c.res and (c.res != "f32" or c.r_off % 16):
        return 0
    if c.up_src and c.up_src != "f32":
        return 0
    return 1


def expect_a_x3_ok(c):
    if c.tile < 0 or not c.x3 or not c.w_x3:
        return 0
    if c.a_mode == 0:
        return int(c.k == c.kpad and not c.relu_in)   # (placement: 128-byte lines, ld and slot strides multiples of 32)
    return int(c.a_mode == 1 and c.conv.cin % 32 == 0 and c.conv.kh * c.conv.kw <= 31 and not c.relu_in)


def fill_params(c, p, ptr, BF16=0, F32=1):
    """the scalar fields and pointers of siu3r_gemm_params for the case; ptr(name) -> address of the buffer's FIRST VIEW ELEMENT (0 when
    the case has no such buffer).  Names: a w_hi w_lo w_x3 c r aux x3 bias c1 c2 ln_part stats cos sin pos up ws cnt"""
    L = layouts(c)
    p.a, p.w_hi, p.c = ptr("a"), ptr("w_hi"), ptr("c")
    p.w_lo = ptr("w_lo") if c.mode == "bf16x3" else None
    p.w_x3 = ptr("w_x3") if c.mode == "bf16x3" and c.w_x3 else None
    p.m, p.n, p.k, p.kpad = c.m, c.n, c.k, c.kpad
    p.a_dtype, p.c_dtype = (BF16 if c.mode == "bf16" else F32), (BF16 if c.c_bf16 else F32)
    p.r_dtype = BF16 if c.res == "bf16" else F32
    p.act, p.relu_in, p.a_mode = c.act, int(c.relu_in), c.a_mode
    p.batch, p.bmod = c.batch, c.bmod
    p.sw = c.n * c.kpad if c.wn > 1 else 0
    p.sbias = (c.shuffle[1] if c.shuffle else c.n) if c.bmod else 0
    if c.a_mode == 0:
        a = L["a"]
        p.lda, p.sa, p.sa_i = a.ld, a.s_o, (-a.s_i if c.flip else a.s_i)
        if c.flip:
            p.a = ptr("a") + (c.G - 1) * a.s_i * a.esz
        p.a_x3 = int(c.a_x3)
    elif c.a_mode == 1:
        cv = c.conv
        p.ih, p.iw, p.cin, p.kh, p.kw, p.stride, p.pad, p.oh, p.ow = cv.ih, cv.iw, cv.cin, cv.kh, cv.kw, cv.stride, cv.pad, cv.oh, cv.ow
        p.a_x3 = int(c.a_x3)
    else:
        B, H, W_ = c.patch
        p.ih, p.iw, p.oh, p.ow = H, W_, H // 16, W_ // 16
    if c.shuffle:
        p.out_mode, p.up, p.cout = 1, c.shuffle[0], c.shuffle[1]
        p.ih, p.iw = c.smap[1], c.smap[2]
        p.ldc = p.ldr = c.shuffle[1]
        p.residual = ptr("r") if c.res else None
    else:
        cl = L["c"]
        p.ldc, p.sc, p.sc_i = cl.ld, cl.s_o, cl.s_i
        if c.res:
            p.residual, p.ldr, p.sr, p.sr_i = ptr("r"), L["r"].ld, L["r"].s_o, L["r"].s_i
        if c.aux:
            p.c_aux = ptr("aux")
        if c.planes:
            col0, kind = c.planes
            p.c_x3 = ptr("c") if kind == "same" else ptr("x3")
            p.c_x3_col0 = col0
            if kind == "only":
                p.c = None
    if c.ln:
        p.ln_stats, p.ln_c1, p.ln_c2 = ptr("ln_part"), ptr("c1"), ptr("c2")
        p.ln_tiles, p.ln_eps = (c.k + 63) // 64, 1e-6
        # statistics rows: two per A row (every other one is spare), slots like A's
        p.ln_ldm, rows = 2, 2 * (c.m + 3)
        p.ln_sz, p.ln_sz_i = (c.G * rows, (-rows if c.flip else rows)) if c.bmod else ((rows if c.batch else 0), 0)
        if c.flip:
            p.ln_stats = ptr("ln_part") + (c.G - 1) * rows * p.ln_tiles * 8
    else:
        p.bias = ptr("bias") if c.bias else None
    if c.stats:
        p.stats_out, p.st_ldm, rows = ptr("stats"), 2, 2 * (c.m + 3)
        p.st_sz, p.st_sz_i = (c.G * rows, rows) if c.bmod else ((rows if c.batch else 0), 0)
    if c.rope:
        p.rope_cos, p.rope_sin, p.rope_pos, p.rope_ncols = ptr("cos"), ptr("sin"), ptr("pos"), c.rope
    if c.up_src:
        p.up_src, p.up_dtype = ptr("up"), (BF16 if c.up_src == "bf16" else F32)
    p.splitk, p.tile_cfg = c.splitk, c.force
    p.sk_ws, p.sk_cnt, p.sk_ws_floats, p.sk_cnt_n = ptr("ws"), ptr("cnt"), WS_FLOATS, WS_COUNTERS
    return p


WS_FLOATS, WS_COUNTERS = 1 << 22, 256


def fake_ptr(c):
    """addresses for the host-only plan query: every buffer on its own 128-byte line plus the case's offset"""
    L = layouts(c)
    names = ["a", "w_hi", "w_lo", "w_x3", "c", "r", "aux", "x3", "bias", "c1", "c2", "ln_part", "stats", "cos", "sin", "pos", "up", "ws", "cnt"]

    def ptr(name):
        base = (names.index(name) + 1) << 32
        if name in L:
            return base + L[name].off * L[name].esz
        if name == "c" and c.shuffle:
            return base + 128 + c.c_off
        if name == "r" and c.shuffle:
            return base + 128 + c.r_off
        return base + 128
    return ptr


def plan_key(kernel, path, x3, lnf):
    return kernel, ((path, bool(x3), bool(lnf)) if path else None)


# ------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------
NO_SKINNY, FORCE_SKINNY = {1: 1}, {4: 1}


def _cases():
    cs = []

    def add(name, mode, m, n, k, kernel, tile, **kw):
        cs.append(Case(name, mode, m, n, k, kernel, tile, **kw))

    conv_tap = lambda cin: Conv(2, 11, 12, cin, 3, 1, 1)              # 2 x 11 x 12 = 264 rows; tap-cursor gather (cin a multiple of the K step)
    conv_small = Conv(2, 22, 24, 8, 3, 2, 1)                          # stride 2 -> 11 x 12; small cin (k = 72, kpad 128)
    conv_up = lambda cin: Conv(2, 10, 12, cin, 3, 1, 1)               # even output size (up_src): 240 rows

    # ---- 1. every default instantiation --------------------------------------------------------------------------------------------
    for cfg in (1, 2, 3):
        bm, bn = TILES[cfg]
        nwide = 320 if cfg == 1 else 200
        for mode in ("bf16x3", "bf16"):
            x3 = mode == "bf16x3"
            t = f"pp{cfg}-{mode}"
            add(f"{t}-dense-m{bm + 33}-n{nwide}-k264", mode, bm + 33, nwide, 264, k_pp(x3, cfg), cfg)
            add(f"{t}-dense-m{bm + 1}-n64-k72", mode, bm + 1, 64, 72, k_pp(x3, cfg), cfg, tune=NO_SKINNY, res="f32")
            add(f"{t}-ln-m{bm + 5}-n72-k264", mode, bm + 5, 72, 264, k_pp(x3, cfg, lnf=True), cfg, ln=True, tune=NO_SKINNY)
            add(f"{t}-ln-m{bm + 33}-n64-k64", mode, bm + 33, 64, 64, k_pp(x3, cfg, lnf=True), cfg, ln=True, act=1)
            cin = 32
            add(f"{t}-conv-tap", mode, 264, 72, 9 * cin, k_pp(x3, cfg, 1), cfg, conv=conv_tap(cin))
            add(f"{t}-conv-tap-relu", mode, 264, 64, 9 * cin, k_pp(x3, cfg, 1, relu=True), cfg, conv=conv_tap(cin), relu_in=True, act=2)
            add(f"{t}-conv-small", mode, 264, 72, 72, k_pp(x3, cfg, 2), cfg, conv=conv_small)
            if x3:
                add(f"{t}-a_x3-m{bm + 33}-n{nwide}-k256", mode, bm + 33, nwide, 256, k_pp(x3, cfg, aps=True), cfg, a_x3=True)
                add(f"{t}-a_x3-ln-m{bm + 1}-n64-k64", mode, bm + 1, 64, 64, k_pp(x3, cfg, lnf=True, aps=True), cfg, a_x3=True, ln=True, tune=NO_SKINNY)
                add(f"{t}-a_x3-conv-tap", mode, 264, 72, 9 * cin, k_pp(x3, cfg, 1, aps=True), cfg, conv=conv_tap(cin), a_x3=True)
    add("pp3-bf16x3-conv-cin4", "bf16x3", 264, 64, 36, k_pp(True, 3, 2), 3, conv=Conv(2, 22, 24, 4, 3, 2, 1, real_cin=3))
    for mode in ("bf16", "bf16x3"):
        x3 = mode == "bf16x3"
        kd = k_dmax if x3 else k_dma
        t = f"dma-{mode}"
        cin = 32 if x3 else 64
        # (tile_cfg 0: the cost model's choice -- with the measured table off -- is the 128 x 64 kernel at these sizes)
        add(f"{t}-dense-auto-m161-n200-k264", mode, 161, 200, 264, kd(), -1, force=0)
        add(f"{t}-dense-auto-m129-n64-k72", mode, 129, 64, 72, kd(), -1, act=1, force=0)
        add(f"{t}-dense-m133-n72-k96", mode, 133, 72, 96, kd(), -1)                         # k % 64 == 32: the tail the bf16x3 kernel does not mask
        add(f"{t}-ln-m133-n72-k264", mode, 133, 72, 264, kd(lnf=True), -1, ln=True)
        add(f"{t}-conv-tap", mode, 264, 72, 9 * cin, kd(1), -1, conv=conv_tap(cin))
        add(f"{t}-conv-tap-relu", mode, 264, 64, 9 * cin, kd(1, relu=True), -1, conv=conv_tap(cin), relu_in=True, res="f32")
        add(f"{t}-conv-small", mode, 264, 72, 72, kd(2), -1, conv=conv_small, act=2)
    add("dma-bf16x3-conv-cin4", "bf16x3", 264, 64, 36, k_dmax(2), -1, conv=Conv(2, 22, 24, 4, 3, 2, 1, real_cin=3))
    # register-staged: fp32 A without the split, bf16x3 without the interleaved planes, patchify, a dense input ReLU
    add("staged-f32-dense-m161-n200-k264", "f32", 161, 200, 264, k_staged(1, 0), -1)
    add("staged-f32-dense-m129-n64-k72", "f32", 129, 64, 72, k_staged(1, 0), -1, act=1, res="bf16")
    add("staged-f32-ln-m133-n72-k264", "f32", 133, 72, 264, k_staged(1, 0, lnf=True), -1, ln=True)
    add("staged-f32-conv-small", "f32", 264, 72, 72, k_staged(1, 0), -1, conv=conv_small)
    add("staged-f32-patchify", "f32", 132, 72, 768, k_staged(1, 0), -1, patch=(1, 192, 176))
    add("staged-bf16x3-patchify", "bf16x3", 132, 64, 768, k_staged(1, 1), -1, patch=(1, 192, 176), stats=True, aux=True)
    add("staged-bf16x3-nox3-m161-n200-k264", "bf16x3", 161, 200, 264, k_staged(1, 1), -1, w_x3=False, force=0)
    add("staged-bf16x3-nox3-ln-m133-n72-k72", "bf16x3", 133, 72, 72, k_staged(1, 1, lnf=True), -1, w_x3=False, ln=True, force=0)
    add("staged-bf16x3-relu_in-m129-n64-k72", "bf16x3", 129, 64, 72, k_staged(1, 1), -1, relu_in=True, force=0)
    add("staged-bf16-relu_in-m161-n200-k264", "bf16", 161, 200, 264, k_staged(0, 0), -1, relu_in=True, c_bf16=True)

    # ---- 2. remainder rows ------------------------------------------------------------------------------------------------------------
    for mode in ("bf16x3", "bf16"):
        x3 = mode == "bf16x3"
        for ln in (False, True):
            t = f"skinny-{mode}{'-ln' if ln else ''}"
            kw = dict(ln=ln, tune=FORCE_SKINNY)
            add(f"{t}-fold-m133-n200-k264", mode, 133, 200, 264, k_pp(x3, 3, lnf=ln), 3, skinny=5, path=1, res="f32", **kw)
            add(f"{t}-fold-m257-n64-k72", mode, 257, 64, 72, k_pp(x3, 2, lnf=ln), 2, skinny=1, path=1, **kw)
            add(f"{t}-mfma-m17-n200-k264", mode, 17, 200, 264, k_pp(x3, 3, lnf=ln), 3, skinny=17, path=2, act=1, **kw)
            add(f"{t}-mfma-m32-n64-k72", mode, 32, 64, 72, k_pp(x3, 3, lnf=ln), 3, skinny=32, path=2, res="f32", **kw)
            # matrix-vector kernel: <= 4 rows and kpad >= 2048.  A folded LayerNorm has k <= 1024 (ln_tiles <= 16): its weight is packed to kpad 2048
            kk = dict(kpad=2048) if ln else {}
            add(f"{t}-gemv-m1-n72-k{1024 if ln else 2048}", mode, 1, 72, 1024 if ln else 2048, k_pp(x3, 3, lnf=ln), 3, skinny=1, path=3, **kk, **kw)
            add(f"{t}-gemv-m4-n200-k{1024 if ln else 2048}", mode, 4, 200, 1024 if ln else 2048, k_pp(x3, 3, lnf=ln), 3, skinny=4, path=3, res="f32", **kk, **kw)

    # ---- 3. split-K (launched twice: the ticket resets itself) ---------------------------------------------------------------------
    for mode in ("bf16x3", "bf16"):
        x3 = mode == "bf16x3"
        for cfg in (1, 2, 3):
            bm = TILES[cfg][0]
            for S in (2, 4):
                add(f"splitk{S}-pp{cfg}-{mode}-m{bm + 33}-n200-k256", mode, bm + 33, 200, 256, k_pp(x3, cfg), cfg, splitk=S, res="f32" if S == 2 else None)
        for S in (2, 4):
            add(f"splitk{S}-dma-{mode}-m161-n200-k256", mode, 161, 200, 256, (k_dmax if x3 else k_dma)(), -1, splitk=S, act=1 if S == 4 else 0)
        add(f"splitk2-pp3-{mode}-ln-fold-m133-n64-k256", mode, 133, 64, 256, k_pp(x3, 3, lnf=True), 3, splitk=2, ln=True, skinny=5, path=1, tune=FORCE_SKINNY)

    # ---- 4. epilogue features, once per family on a problem the fast row pass takes and once on one it cannot -----------------------
    fams = [("pp3-bf16x3", "bf16x3", 3, lambda **k: k_pp(True, 3, **k), 161), ("pp2-bf16", "bf16", 2, lambda **k: k_pp(False, 2, **k), 289),
            ("dma-bf16x3", "bf16x3", -1, lambda **k: k_dmax(**k), 161), ("dma-bf16", "bf16", -1, lambda **k: k_dma(**k), 161),
            ("staged-f32", "f32", -1, lambda mode=0, lnf=False: k_staged(1, 0, lnf=lnf), 161)]
    for (t, mode, cfg, kn, m) in fams:
        pp = cfg > 0
        for fast in (True, False):
            n, sfx = (320 if fast else 200), ("fast" if fast else "general")
            base = dict(mode=mode, m=m, n=n, k=72, kernel=kn(), tile=cfg)
            feats = [("gelu", dict(act=1)), ("relu", dict(act=2)), ("res-f32", dict(res="f32")), ("res-bf16", dict(res="bf16", c_bf16=True)),
                     ("c-bf16", dict(c_bf16=True, act=1)), ("rope", dict(rope=128, bias=True, res="f32")), ("stats", dict(stats=True, res="f32", act=1)),
                     ("aux", dict(aux=True)), ("batch", dict(batch=3, res="f32")), ("bmod-flip", dict(batch=4, bmod=2, flip=True, res="f32"))]
            for (f, kw) in feats:
                add(f"epi-{t}-{f}-{sfx}", **{**base, **kw})
            add(f"epi-{t}-ln-stats-{sfx}", **{**base, "ln": True, "stats": True, "k": 264, "kernel": kn(lnf=True)})
        # ineligible twins of the fast pass, one condition each (n % 64 != 0 is the `general` column above)
        base = dict(mode=mode, m=m, n=320, k=72, kernel=kn(), tile=cfg)
        add(f"epi-{t}-c-off4", **{**base, "c_off": 4, "act": 1})
        add(f"epi-{t}-res-off4", **{**base, "res": "f32", "r_off": 4})
        add(f"epi-{t}-ldc-odd", **{**base, "ldc_odd": True, "res": "f32"})
        add(f"epi-{t}-c-bf16-rope", **{**base, "c_bf16": True, "rope": 128})
        add(f"epi-{t}-c-bf16-off2", **{**base, "c_bf16": True, "c_off": 2})
        # convolution forms: the x2 upsample-add and the pixel shuffle
        cin = 64 if mode == "bf16" else 32
        ck = kn(mode=1)  # (the tap-cursor gather; the register-staged kernel has one gather)
        for ups in ("f32", "bf16"):
            for n in (64, 72):
                add(f"epi-{t}-up_src-{ups}-n{n}", mode, 240, n, 9 * cin, ck, cfg, conv=conv_up(cin), up_src=ups, act=2)
        for (up, co, name) in ((2, 16, "up2"), (4, 8, "up4")):
            add(f"epi-{t}-shuffle-{name}", mode, 264, up * up * co, 72, kn(), cfg, shuffle=(up, co), smap=(2, 11, 12), res="f32" if up == 2 else None)
        if pp and mode == "bf16x3":
            for (col0, kind) in ((0, "sep"), (64, "sep"), (64, "same"), (0, "only")):
                add(f"epi-{t}-c_x3-{kind}-col{col0}", mode, m, 320, 72, kn(), cfg, planes=(col0, kind), res="f32", act=1)
            add(f"epi-{t}-c_x3-from-a_x3", mode, m, 320, 64, kn(aps=True), cfg, a_x3=True, planes=(0, "sep"))

    # ---- 5. instantiations only an A/B switch reaches ---------------------------------------------------------------------------------
    for mode in ("bf16", "bf16x3"):
        x3 = mode == "bf16x3"
        cin = 32 if x3 else 64
        for (env, ks, ni) in (("SIU3R_GEMM_NO_KSPLIT=1", 1, 1),) + ((("SIU3R_GEMM_NARROW_MAX=0", 2, 2), ("SIU3R_GEMM_NARROW_MAX=0,SIU3R_GEMM_NO_KSPLIT=1", 1, 2)) if not x3 else ()):
            kd = (lambda mode_=0, relu=False, lnf=False: k_dmax(mode_, relu, lnf, ks=ks)) if x3 else (lambda mode_=0, relu=False, lnf=False: k_dma(mode_, relu, lnf, ni=ni, ks=ks))
            t = f"switch-ks{ks}-ni{ni}-{mode}"
            add(f"{t}-dense", mode, 161, 200, 264, kd(), -1, env=env, res="f32")
            add(f"{t}-ln", mode, 133, 72 if ni == 1 else 200, 264, kd(lnf=True), -1, env=env, ln=True)
            add(f"{t}-conv-tap", mode, 264, 72 if ni == 1 else 200, 9 * cin, kd(1), -1, env=env, conv=conv_tap(cin))
            add(f"{t}-conv-tap-relu", mode, 264, 72 if ni == 1 else 200, 9 * cin, kd(1, relu=True), -1, env=env, conv=conv_tap(cin), relu_in=True)
            add(f"{t}-conv-small", mode, 264, 72 if ni == 1 else 200, 72, kd(2), -1, env=env, conv=conv_small)
    nd = "SIU3R_GEMM_NO_DMA=1"
    add("switch-nodma-bf16-dense", "bf16", 161, 200, 264, k_staged(0, 0), -1, env=nd, res="bf16", c_bf16=True)
    add("switch-nodma-bf16-ln", "bf16", 133, 72, 264, k_staged(0, 0, lnf=True), -1, env=nd, ln=True)
    add("switch-nodma-bf16x3-dense", "bf16x3", 161, 200, 264, k_staged(1, 1), -1, env=nd, force=0)
    add("switch-nodma-bf16-conv-small", "bf16", 264, 72, 72, k_staged(0, 0), -1, env=nd, conv=conv_small)
    nm_ = "SIU3R_GEMM_NARROW_MAX=0"
    add("switch-wide-f32-dense", "f32", 161, 200, 264, k_staged(1, 0, ni=2), -1, env=nm_)
    add("switch-wide-f32-ln", "f32", 133, 200, 264, k_staged(1, 0, lnf=True, ni=2), -1, env=nm_, ln=True)
    add("switch-wide-bf16-relu_in", "bf16", 161, 200, 264, k_staged(0, 0, ni=2), -1, env=nm_, relu_in=True)
    add("switch-wide-bf16x3-nox3", "bf16x3", 161, 200, 264, k_staged(1, 1, ni=2), -1, env=nm_, w_x3=False, force=0)
    add("switch-wide-bf16x3-nox3-ln", "bf16x3", 133, 200, 72, k_staged(1, 1, lnf=True, ni=2), -1, env=nm_, w_x3=False, ln=True, force=0)
    add("switch-wide-nodma-bf16-ln", "bf16", 133, 200, 264, k_staged(0, 0, lnf=True, ni=2), -1, env=nm_ + "," + nd, ln=True)
    for mode in ("bf16x3", "bf16"):
        x3 = mode == "bf16x3"
        for ln in (False, True):
            t = f"switch-{mode}{'-ln' if ln else ''}"
            add(f"{t}-nofold-mfma-m133-n200-k264", mode, 133, 200, 264, k_pp(x3, 3, lnf=ln), 3, skinny=5, path=2, ln=ln, tune=FORCE_SKINNY, env="SIU3R_GEMM_NO_FOLD=1", res="f32")
        add(f"switch-{mode}-nofold-gemv-m129-n72-k2048", mode, 129, 72, 2048, k_pp(x3, 3), 3, skinny=1, path=3, tune=FORCE_SKINNY, env="SIU3R_GEMM_NO_FOLD=1")
        add(f"switch-{mode}-nogemv-m4-n72-k2048", mode, 4, 72, 2048, k_pp(x3, 3), 3, skinny=4, path=2, tune=FORCE_SKINNY, env="SIU3R_GEMM_NO_GEMV=1")
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = _cases()
DEFAULT_CASES = [c for c in CASES if c.env is None]
SWITCH_CASES = [c for c in CASES if c.env is not None]
SWITCHES = sorted({c.env for c in SWITCH_CASES})


def _all_pp():
    out = []
    for cfg in (1, 2, 3):
        out += [k_pp(True, cfg), k_pp(True, cfg, lnf=True), k_pp(True, cfg, aps=True), k_pp(True, cfg, lnf=True, aps=True), k_pp(True, cfg, 1),
                k_pp(True, cfg, 1, relu=True), k_pp(True, cfg, 1, aps=True), k_pp(True, cfg, 2)]                      # gemm_pp_t{1,2,3}x.hip
        out += [k_pp(False, cfg), k_pp(False, cfg, lnf=True), k_pp(False, cfg, 1), k_pp(False, cfg, 1, relu=True), k_pp(False, cfg, 2)]  # gemm_pp_t{1,2,3}b.hip
    return out


# Every kernel siu3r_gemm can launch without an environment switch, written out by hand from the launch code: the six gemm_pp_t*.hip
# units (a forced tile_cfg reaches every one of them), siu3r_gemm_dma_launch / siu3r_gemm_dma_x3_launch with their default 8-wave
# workgroups (K-split argument 2) and 128 x 64 tile, and launch<1> of gemm.hip for what those refuse.
KERNELS_DEFAULT = sorted(_all_pp() + [
    k_dma(0), k_dma(0, lnf=True), k_dma(1), k_dma(1, relu=True), k_dma(2),
    k_dmax(0), k_dmax(0, lnf=True), k_dmax(1), k_dmax(1, relu=True), k_dmax(2),
    k_staged(1, 0), k_staged(1, 0, lnf=True),            # fp32 A without the split
    k_staged(1, 1), k_staged(1, 1, lnf=True),            # bf16x3 without w_x3, patchify, a dense input ReLU
    k_staged(0, 0),                                      # bf16 with a dense input ReLU
])
KERNELS_SWITCH_ONLY = sorted([
    k_dma(0, ks=1), k_dma(0, lnf=True, ks=1), k_dma(1, ks=1), k_dma(1, relu=True, ks=1), k_dma(2, ks=1),                       # SIU3R_GEMM_NO_KSPLIT
    k_dmax(0, ks=1), k_dmax(0, lnf=True, ks=1), k_dmax(1, ks=1), k_dmax(1, relu=True, ks=1), k_dmax(2, ks=1),
    k_dma(0, ni=2), k_dma(0, lnf=True, ni=2), k_dma(1, ni=2), k_dma(1, relu=True, ni=2), k_dma(2, ni=2),                       # SIU3R_GEMM_NARROW_MAX=0
    k_dma(0, ni=2, ks=1), k_dma(0, lnf=True, ni=2, ks=1), k_dma(1, ni=2, ks=1), k_dma(1, relu=True, ni=2, ks=1), k_dma(2, ni=2, ks=1),  # ... with NO_KSPLIT
    k_staged(0, 0, lnf=True),                                                                                                  # SIU3R_GEMM_NO_DMA
    k_staged(1, 0, ni=2), k_staged(1, 0, lnf=True, ni=2), k_staged(0, 0, ni=2), k_staged(1, 1, ni=2), k_staged(1, 1, lnf=True, ni=2),  # launch<2>: NARROW_MAX=0
    k_staged(0, 0, lnf=True, ni=2),                                                                                            # ... with NO_DMA
])
# remainder-row code (siu3r_gemm_plan_t.skinny_path, bf16x3?, folded LayerNorm?): 1 = skinny_rows_body inside the ping-pong launch,
# 2 = gemm_skinny_kernel<X3, LNF>, 3 = gemm_skinny_gemv_kernel<X3, LNF>
SKINNY_DEFAULT = sorted([(1, x3, ln) for x3 in (False, True) for ln in (False, True)] + [(2, x3, ln) for x3 in (False, True) for ln in (False, True)] +
                        [(3, x3, ln) for x3 in (False, True) for ln in (False, True)])
