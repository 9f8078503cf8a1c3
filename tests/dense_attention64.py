"""Dense float64 restatement of siu3r_attention (include/siu3r_hip.h), written from the ABI's definition, plus the per-row comparison,
the input generator and the case list that tests/test_attention_ref.py (CPU) and tests/test_attention_gpu.py (GPU) share.

    out[b, i, h, :] = sum_j softmax_j(scale * <rope(q)[b, i, h], rope(k)[b ^ kv_bxor, j, h]>) v[b ^ kv_bxor, j, h, :]

over the keys j < Nk whose mask byte mask[b, i, j] is 0 (mask bytes at j >= Nk are padding and ignored).  RoPE2D: the head vector is
[u_Y v_Y u_X v_X] in quarters of D, (u, v) -> (u c - v s, v c + u s) with (c, s) = (cos, sin)[pos[axis]] of the fp32 table.

The reference receives the operands as the kernel sees them: bf16-rounded values for the bf16 mode and for fp32 tensors without
split3 (the kernel rounds them itself), the fp32 values for bf16x3.

Not a test module."""
import numpy as np
import torch

TOL_BF16 = 2e-2  # the suite's tolerances (tests/test_kernels_gpu.py), applied here per element against the row's natural scale
TOL_F32 = 2e-4
MIN_MARGIN = 20.0   # logit margin of a sentinel's winning key over every other admitted key
NEAR_GAP = 2.0      # near-tie rows: the second key lies this far below the first (weight 0.12), both MIN_MARGIN above the rest
MIN_ROW = 0.25      # every reference row reaches this fraction of Vmax in some element


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def rope2d64(x, pos, cos, sin):
    """x [B, N, H, D] float64, pos [B, N, 2] int64 (y, x), cos / sin [max_pos, D / 4]"""
    Q = x.shape[-1] // 4
    out = torch.empty_like(x)
    for ax in range(2):
        c = cos.double()[pos[:, :, ax]][:, :, None, :]
        s = sin.double()[pos[:, :, ax]][:, :, None, :]
        u, v = x[..., 2 * ax * Q:2 * ax * Q + Q], x[..., 2 * ax * Q + Q:2 * ax * Q + 2 * Q]
        out[..., 2 * ax * Q:2 * ax * Q + Q] = u * c - v * s
        out[..., 2 * ax * Q + Q:2 * ax * Q + 2 * Q] = v * c + u * s
    return out


def logits64(q, k, scale, *, rope=None, qpos=None, kpos=None, mask=None, kv_bxor=0):
    """[B, H, Nq, Nk] float64 logits, -inf where the key is masked.  q [B, Nq, H, D], k [B, Nk, H, D] (any strides)."""
    q, k = q.detach().cpu().double(), k.detach().cpu().double()
    B, Nk = k.shape[0], k.shape[1]
    if rope is not None:
        q, k = rope2d64(q, qpos.cpu(), rope[0].cpu(), rope[1].cpu()), rope2d64(k, kpos.cpu(), rope[0].cpu(), rope[1].cpu())
    k = k[torch.arange(B) ^ kv_bxor]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * float(np.float32(scale))
    if mask is not None:
        blocked = mask.cpu()[:, :, :Nk] != 0  # bytes beyond Nk are padding
        s = s.masked_fill(blocked[:, None], float("-inf"))
    return s


def weighted64(s, v, kv_bxor=0):
    """softmax over the last axis of s [B, H, Nq, Nk] applied to v [B, Nk, H, D] of batch item b ^ kv_bxor -> [B, Nq, H * D]"""
    v = v.detach().cpu().double()
    v = v[torch.arange(v.shape[0]) ^ kv_bxor]
    m = s.amax(-1, keepdim=True)
    assert torch.isfinite(m).all(), "a row without an admitted key has no defined result"
    p = torch.exp(s - m)
    o = torch.einsum("bhqk,bkhd->bqhd", p / p.sum(-1, keepdim=True), v)
    return o.flatten(2)


def dense_attention64(q, k, v, scale, *, rope=None, qpos=None, kpos=None, mask=None, kv_bxor=0):
    return weighted64(logits64(q, k, scale, rope=rope, qpos=qpos, kpos=kpos, mask=mask, kv_bxor=kv_bxor), v, kv_bxor)


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def row_scales(v, kv_bxor=0):
    """Vmax[b, h] = max |v[b ^ kv_bxor, :, h, :]|: an output row is a convex combination of those V rows"""
    v = v.detach().cpu().double()
    return v[torch.arange(v.shape[0]) ^ kv_bxor].abs().amax((1, 3))


def assert_rows_close(out, ref, v, tol, *, kv_bxor=0, name="", quiet=False):
    """every element of out [B, Nq, H * D] within tol * Vmax[b, h] of ref; names the worst (b, q, h, d); returns the worst ratio"""
    vmax = row_scales(v, kv_bxor)  # [B, H]
    B, H = vmax.shape
    ref = ref.detach().cpu().double()
    Nq, D = ref.shape[1], ref.shape[2] // H
    r4 = ref.view(B, Nq, H, D)
    ratio = r4.abs().amax(-1) / vmax[:, None, :]
    assert float(ratio.min()) >= MIN_ROW, f"{name}: reference row {tuple(int(i) for i in np.unravel_index(int(ratio.argmin()), ratio.shape))} " \
                                          f"(b, q, h) reaches only {float(ratio.min()):.3f} of Vmax: the bound would be met by a small output"
    assert tuple(out.shape) == tuple(ref.shape), (tuple(out.shape), tuple(ref.shape))
    o4 = out.detach().cpu().double().view(B, Nq, H, D)
    err = (o4 - r4).abs() / vmax[:, None, :, None]
    err = torch.where(torch.isfinite(o4), err, torch.full_like(err, float("inf")))
    b, q, h, d = (int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
    worst = float(err[b, q, h, d])
    if not quiet:
        print(f"[parity] {name}: worst row (b={b}, q={q}, h={h}) d={d}: |out - ref| / Vmax = {worst:.3e} tol={tol:.1e} "
              f"(out {float(o4[b, q, h, d]):+.6f} ref {float(r4[b, q, h, d]):+.6f} Vmax {float(vmax[b, h]):.4f})")
    assert worst <= tol, f"{name}: (b={b}, q={q}, h={h}, d={d}): |out - ref| = {worst:.3e} * Vmax > {tol:.1e} * Vmax " \
                         f"(out {float(o4[b, q, h, d])!r} ref {float(r4[b, q, h, d])!r})"
    return worst


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
MODES = {  # name -> (tensor dtype, split3, tolerance, dtype the kernel rounds its operands to)
    "bf16": (torch.bfloat16, False, TOL_BF16, torch.bfloat16),
    "f32": (torch.float32, False, TOL_BF16, torch.bfloat16),
    "bf16x3": (torch.float32, True, TOL_F32, torch.float32),
}
ROPE_MAX_POS = 37
SENTINEL_ROWS = (0, 31, 32, 63, 64, 127, 128)


class Case:
    """One launch: shape, mode, options, and the plan it must get (kernel name, queries per workgroup, key ranges)."""

    def __init__(self, branch, mode, B, H, Nq, Nk, D, expect, *, mask=None, ld_extra=0, kv_bxor=0, rope=False, planes=False, env=None):
        self.branch, self.mode, self.B, self.H, self.Nq, self.Nk, self.D = branch, mode, B, H, Nq, Nk, D
        self.kernel, self.qpw, self.ranges = expect
        self.mask, self.ld_extra, self.kv_bxor, self.rope, self.planes = mask, ld_extra, kv_bxor, rope, planes  # mask: None / "ones" / "zeros" = padding fill
        self.env = env  # the A/B switch this case needs, or None
        self.id = f"{branch}-{mode}-d{D}-b{B}h{H}-q{Nq}-k{Nk}" + (f"-mask_{mask}{ld_extra}" if mask else "") + (f"-bxor{kv_bxor}" if kv_bxor else "") + \
                  ("-rope" if rope else "") + ("-planes" if planes else "") + (f"-{env}" if env else "")

    # the split heuristic of ops.attention, restated (asserted against the plan query by the GPU tests)
    @property
    def splits(self):
        fast = not self.rope and self.mode in ("bf16", "bf16x3")
        nkt = (self.Nk + 63) // 64
        return min(16, nkt // 4) if fast and self.Nq <= 128 and self.Nk >= 1024 else 1

    def key_parts(self):
        """the key sets whose partial results the kernel merges: key ranges of whole 64-key tiles (SPLITKV), or the two 32-key halves
        of every tile (key-half and pipelined kernels); else one part"""
        keys = torch.arange(self.Nk)
        if self.ranges > 1:
            nkt = (self.Nk + 63) // 64
            per = (nkt + self.ranges - 1) // self.ranges
            parts = [keys[(keys // 64 >= r * per) & (keys // 64 < (r + 1) * per)] for r in range(self.ranges)]
            return [p for p in parts if len(p)]
        if self.qpw == 64 or "pipe" in self.kernel:
            parts = [keys[keys % 64 < 32], keys[keys % 64 >= 32]]
            return [p for p in parts if len(p)]
        return [keys]

    def empty_ranges(self):
        return self.ranges - len(self.key_parts()) if self.ranges > 1 else 0


def _u(g, *shape, lo=-1.0, hi=1.0):
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)


def make_inputs(c, seed=0):
    """Seeded CPU inputs of a case, as float32 tensors already rounded to what the kernel will see (so the float64 reference and the
    device tensors come from the same values): dict with q [B, Nq, H, D], k, v [B, Nk, H, D], scale, mask (uint8 [B, Nq, ld] or None),
    rope (cos, sin) / qpos / kpos or None, v_scale_ref (v with the never-admitted rows at their generated size: the source of Vmax),
    sentinels: list of (b, q, h, key, near) -- row (b, q, h) is won by `key` with margin >= MIN_MARGIN; near = the key NEAR_GAP below
    it or -1."""
    B, H, Nq, Nk, D = c.B, c.H, c.Nq, c.Nk, c.D
    rdt = MODES[c.mode][3]
    g = torch.Generator().manual_seed(1000 + seed)
    rnd = lambda t: t.to(rdt).double()
    q, k, v = rnd(_u(g, B, Nq, H, D, lo=-6, hi=6)), rnd(_u(g, B, Nk, H, D, lo=-6, hi=6)), rnd(_u(g, B, Nk, H, D))
    scale = D ** -0.5
    rope = qpos = kpos = None
    if c.rope:
        Q = D // 4
        inv = 1.0 / torch.pow(torch.tensor(100.0, dtype=torch.float32), torch.arange(Q, dtype=torch.float32) / Q)
        ang = torch.arange(ROPE_MAX_POS, dtype=torch.float32)[:, None] * inv[None, :]
        rope = (torch.cos(ang), torch.sin(ang))
        qpos = torch.randint(0, ROPE_MAX_POS, (B, Nq, 2), generator=g)
        kpos = torch.randint(0, ROPE_MAX_POS, (B, Nk, 2), generator=g)
        # positions 0 and rope_max_pos - 1 on the rows the sentinels use; qpos != kpos everywhere that matters
        qpos[:, 0], qpos[:, -1] = torch.tensor([0, ROPE_MAX_POS - 1]), torch.tensor([ROPE_MAX_POS - 1, 0])
        kpos[:, 0], kpos[:, -1] = torch.tensor([ROPE_MAX_POS - 1, ROPE_MAX_POS - 1]), torch.tensor([0, 0])

    parts = c.key_parts()
    nkt = (Nk + 63) // 64
    # ---- mask: i.i.d. p = 0.7 with key 0 open, then the structured rows
    mask = None
    special = {}  # (b, q) -> the only admitted key of that row
    heavy = []    # (b, keys): V rows no query of batch item b admits, scaled by 1e4
    if c.mask:
        ld = nkt * 64 + c.ld_extra
        m = torch.rand(B, Nq, Nk, generator=g) < 0.7
        m[:, :, 0] = False
        rows = [r for r in (1, 33, 65, 126, Nq - 2) if 0 <= r < Nq and r not in SENTINEL_ROWS and r != Nq - 1]
        rows = list(dict.fromkeys(rows))
        only = [0, Nk - 1]                       # only key 0; only key Nk - 1 (in the ragged tile when Nk % 64 != 0)
        if nkt >= 3:
            only.append(128 + 37 if Nk > 165 else Nk - 1)  # a key of the third tile, the first two tiles fully masked
        if len(parts) > 1:
            only += [int(parts[-1][-1]), int(parts[0][5 % len(parts[0])]), int(parts[len(parts) // 2][0])]  # survivor in the ragged last tile / in range 0 only / mid range
        for i, key in enumerate(dict.fromkeys(only)):
            if i < len(rows):
                special[(0, rows[i])] = key
        if B > 1 and nkt >= 3:
            # the last batch item: every query admits keys of the last part / from the third tile on only; the V rows in front are heavy
            first = int(parts[-1][0]) if c.ranges > 1 else 128
            m[B - 1, :, :first] = True
            m[B - 1, :, first] = False
            heavy.append((B - 1, torch.arange(first)))
        for (b, r), key in special.items():
            m[b, r, :] = True
            m[b, r, key] = False
        mask = torch.full((B, Nq, ld), 1 if c.mask == "ones" else 0, dtype=torch.uint8)
        mask[:, :, :Nk] = m.to(torch.uint8)

    # ---- sentinels: boundary keys spread over the (row, b, h) slots
    srows = [r for r in dict.fromkeys(SENTINEL_ROWS + (Nq - 1,)) if r < Nq]
    bounds = [Nk - 1, 0]
    for p in parts:
        bounds += [int(p[0]), int(p[-1])]
    bounds += [31, 32, 63, 64]
    bounds = [t for t in dict.fromkeys(bounds) if 0 <= t < Nk]
    slots = [(b, r, h) for r in srows for h in range(H) for b in range(B) if (b, r) not in special]
    want = [(t, -1) for t in bounds]
    if Nk >= 2:
        want.insert(2, (max(Nk - 2 - (5 % Nk), 0) if Nk > 2 else 0, Nk - 1))  # near-tie: key Nk - 1 second, NEAR_GAP below the winner
    hidden = {b: int(keys[-1]) + 1 for b, keys in heavy}  # batch item -> its first admissible key
    assign, wi = [], 0
    for (b, r, h) in slots:  # pass 1: targets, and their mask bytes opened (the mask row is shared by the heads)
        if len(assign) >= max(2 * len(want), 24):
            break
        t, near = want[wi % len(want)]
        if min(t, near if near >= 0 else t) < hidden.get(b, 0):
            if all(min(t2, n2 if n2 >= 0 else t2) < hidden[b] for t2, n2 in want):
                continue
            while min(t, near if near >= 0 else t) < hidden[b]:
                wi += 1
                t, near = want[wi % len(want)]
        wi += 1
        assign.append((b, r, h, t, near))
        if mask is not None:
            mask[b, r, t] = 0
            if near >= 0:
                mask[b, r, near] = 0
    kk = k if rope is None else rope2d64(k, kpos, *rope)
    sentinels = []
    for (b, r, h, t, near) in assign:  # pass 2: the query vectors
        adm = torch.ones(Nk, dtype=torch.bool) if mask is None else mask[b, r, :Nk] == 0
        K = kk[b ^ c.kv_bxor, :, h]  # [Nk, D], RoPE'd
        kt_ = K[t]
        others = adm.clone()
        others[t] = False
        if near >= 0:
            others[near] = False
            kn = K[near]
            dirv, diff = kt_ + kn, kt_ - kn
            dirv = dirv - diff * (float(dirv @ diff) / float(diff @ diff))  # scores t and near equally
            top = float(dirv @ kt_)
            rest = float((K[others] @ dirv).max()) if others.any() else -abs(top)
            if top - rest <= 0.05 * abs(top):
                continue
            qv = dirv * ((MIN_MARGIN + NEAR_GAP + 6.0) / (scale * (top - rest))) + diff * (NEAR_GAP / (scale * float(diff @ diff)))
        else:
            top = float(kt_ @ kt_)
            rest = float((K[others] @ kt_).max()) if others.any() else -top
            if top - rest <= 0.05 * top:
                continue
            qv = kt_ * ((MIN_MARGIN + 6.0) / (scale * (top - rest)))
        if rope is not None:  # q is RoPE'd by the kernel: hand it the inverse rotation
            qv = rope2d64(qv[None, None, None, :], qpos[b:b + 1, r:r + 1], rope[0], -rope[1])[0, 0, 0]
        q[b, r, h] = rnd(qv)
        sentinels.append((b, r, h, t, near))
    v_ref = v.clone()
    for b, keys in heavy:
        v[b ^ c.kv_bxor, keys] = rnd(v[b ^ c.kv_bxor, keys] * 1e4)
    f = lambda t: t.float()
    return dict(q=f(q), k=f(k), v=f(v), v_scale_ref=f(v_ref), scale=scale, mask=mask, rope=rope, qpos=qpos, kpos=kpos, sentinels=sentinels,
                special=special, heavy=heavy)


def reference(c, inp):
    s = logits64(inp["q"], inp["k"], inp["scale"], rope=inp["rope"], qpos=inp["qpos"], kpos=inp["kpos"], mask=inp["mask"], kv_bxor=c.kv_bxor)
    return s, weighted64(s, inp["v"], c.kv_bxor)


def check_margins(c, inp, s):
    """on the float64 logits: every sentinel's key wins its row by MIN_MARGIN (a near-tie row: both keys, NEAR_GAP apart)"""
    assert inp["sentinels"], f"{c.id}: no sentinel row"
    for (b, r, h, t, near) in inp["sentinels"]:
        row = s[b, h, r].clone()
        top = float(row[t])
        row[t] = float("-inf")
        if near >= 0:
            gap = top - float(row[near])
            assert 0.5 * NEAR_GAP <= gap <= 1.5 * NEAR_GAP, (c.id, b, r, h, t, near, gap)
            row[near] = float("-inf")
        assert top - float(row.max()) >= MIN_MARGIN, (c.id, b, r, h, t, top - float(row.max()))
    for (b, r), key in inp["special"].items():
        row = s[b, :, r]
        assert torch.isfinite(row).sum(-1).eq(1).all() and torch.isfinite(row[:, key]).all(), (c.id, b, r, key)


def _x(mode):
    return 1 if mode == "bf16x3" else 0


def _fast(D, mask, splitkv, mode, kh):
    return f"attn_fast_kernel<{D}, {mask}, {splitkv}, {_x(mode)}, {kh}>"


def _staged(D, mode, mask, rope=False):
    return f"attn_kernel<{D}, {0 if mode == 'bf16' else 1}, {_x(mode)}, {mask}, {int(rope and mode != 'bf16x3')}>"


def _pipe(mode, planes=False):
    return f"siu3r_attn_pipe::attn_pipe_kernel<{'true' if mode == 'bf16x3' else 'false'}, {'true' if planes else 'false'}>"


def _cases():
    cs = []
    add = lambda *a, **kw: cs.append(Case(*a, **kw))
    # ---- pipelined kernel: bf16x3 always (D = 64, Nk >= 64), bf16 from 192 128-query workgroups on, pre-split planes
    for (Nq, Nk) in ((128, 64), (129, 65), (130, 127), (257, 129)):
        add("pipe", "bf16x3", 1, 2, Nq, Nk, 64, (_pipe("bf16x3"), 128, 1))
    add("pipe", "bf16x3", 2, 2, 129, 129, 64, (_pipe("bf16x3", True), 128, 1), planes=True)
    add("pipe", "bf16x3", 4, 2, 257, 65, 64, (_pipe("bf16x3", True), 128, 1), planes=True, kv_bxor=1)
    add("pipe", "bf16", 2, 96, 128, 64, 64, (_pipe("bf16"), 128, 1))            # 192 workgroups: the threshold
    add("keyhalf", "bf16", 2, 95, 128, 64, 64, (_fast(64, 0, 0, "bf16", 1), 64, 1))  # 190: one below it
    add("pipe", "bf16", 1, 96, 129, 65, 64, (_pipe("bf16"), 128, 1))            # 192 by ceil(129 / 128) = 2 tiles a problem; runs one, with the side path
    for bx in (1, 3):
        add("pipe", "bf16x3", 4, 2, 130, 65, 64, (_pipe("bf16x3"), 128, 1), kv_bxor=bx)
    # ---- fast kernel, key halves (no mask, Nk >= 64, few workgroups)
    for D, mode in ((32, "bf16"), (64, "bf16"), (32, "bf16x3")):
        for (Nq, Nk) in ((1, 64), (63, 65), (64, 95), (65, 96), (64, 97), (65, 129)):
            add("keyhalf", mode, 2, 2, Nq, Nk, D, (_fast(D, 0, 0, mode, 1), 64, 1))
    for bx in (1, 3):
        add("keyhalf", "bf16", 4, 2, 65, 97, 32, (_fast(32, 0, 0, "bf16", 1), 64, 1), kv_bxor=bx)
    # ---- fast kernel, standard, no mask: Nk < 64 ...
    for D in (32, 64):
        for mode in ("bf16", "bf16x3"):
            for i, Nk in enumerate((1, 7, 8, 31, 32, 33, 63)):
                add("std", mode, 1, 3, (1, 129, 65, 100)[i % 4], Nk, D, (_fast(D, 0, 0, mode, 0), 128, 1))
    # ... and D = 32 at / above the workgroup thresholds (256 bf16, 512 bf16x3), one below them on the key-half kernel
    add("std", "bf16", 4, 64, 100, 70, 32, (_fast(32, 0, 0, "bf16", 0), 128, 1))
    add("keyhalf", "bf16", 3, 85, 100, 70, 32, (_fast(32, 0, 0, "bf16", 1), 64, 1))
    add("std", "bf16x3", 8, 64, 100, 70, 32, (_fast(32, 0, 0, "bf16x3", 0), 128, 1))
    add("keyhalf", "bf16x3", 7, 73, 100, 70, 32, (_fast(32, 0, 0, "bf16x3", 1), 64, 1))
    # ---- fast kernel, masked, unsplit
    for D in (32, 64):
        for mode in ("bf16", "bf16x3"):
            for i, Nk in enumerate((1, 63, 64, 65, 200)):
                for fill in ("ones", "zeros"):
                    add("masked", mode, 2, 2, (130, 100, 129, 65, 130)[i], Nk, D, (_fast(D, 1, 0, mode, 0), 128, 1), mask=fill, ld_extra=64 * ((i + (fill == "zeros")) % 2))
    # ---- fast kernel, key ranges
    for D in (32, 64):
        for mode in ("bf16", "bf16x3"):
            for i, (Nq, Nk, ranges) in enumerate(((1, 1024, 4), (100, 1025, 4), (128, 2100, 8), (100, 4130, 16))):
                add("ranges", mode, 1, 4 if Nq == 1 else 2, Nq, Nk, D, (_fast(D, 0, 1, mode, 0), 128, ranges))
                add("ranges", mode, 2, 4 if Nq == 1 else 2, Nq, Nk, D, (_fast(D, 1, 1, mode, 0), 128, ranges), mask=("zeros", "ones")[i % 2], ld_extra=64 * (i % 2))
    # ---- register-staged kernel: RoPE on load (D = 64), fp32 tensors without split3
    for mode in ("bf16", "f32", "bf16x3"):
        add("staged", mode, 2, 2, 130, 65, 64, (_staged(64, mode, 0, True), 128, 1), rope=True)
        add("staged", mode, 2, 2, 65, 200, 64, (_staged(64, mode, 1, True), 128, 1), rope=True, mask="zeros", ld_extra=64)
    for D in (32, 64):
        add("staged", "f32", 1, 2, 129, 65, D, (_staged(D, "f32", 0), 128, 1))
        add("staged", "f32", 2, 2, 65, 200, D, (_staged(D, "f32", 1), 128, 1), mask="zeros")
    for bx in (1, 3):
        add("staged", "f32", 4, 2, 65, 97, 64, (_staged(64, "f32", 0), 128, 1), kv_bxor=bx)
    # ---- instantiations only an A/B switch reaches
    nf = "SIU3R_ATTN_NO_FAST"
    add("switch", "bf16", 1, 2, 129, 65, 64, (_staged(64, "bf16", 0), 128, 1), env=nf)
    add("switch", "bf16", 2, 2, 65, 200, 32, (_staged(32, "bf16", 1), 128, 1), mask="zeros", env=nf)
    add("switch", "bf16", 1, 2, 33, 63, 32, (_staged(32, "bf16", 0), 128, 1), env=nf)
    add("switch", "bf16", 2, 2, 65, 200, 64, (_staged(64, "bf16", 1), 128, 1), mask="ones", ld_extra=64, env=nf)
    add("switch", "bf16x3", 1, 2, 129, 65, 64, (_staged(64, "bf16x3", 0), 128, 1), env=nf)
    add("switch", "bf16x3", 2, 2, 65, 200, 64, (_staged(64, "bf16x3", 1), 128, 1), mask="zeros", env=nf)
    add("switch", "bf16x3", 1, 2, 129, 65, 32, (_staged(32, "bf16x3", 0), 128, 1), env=nf)
    add("switch", "bf16x3", 2, 2, 65, 200, 32, (_staged(32, "bf16x3", 1), 128, 1), mask="ones", env=nf)
    npipe = "SIU3R_ATTN_NO_PIPE"
    add("switch", "bf16x3", 1, 2, 129, 65, 64, (_fast(64, 0, 0, "bf16x3", 1), 64, 1), env=npipe)
    add("switch", "bf16x3", 2, 2, 65, 129, 64, (_fast(64, 0, 0, "bf16x3", 1), 64, 1), env=npipe)
    add("switch", "bf16x3", 2, 128, 257, 65, 64, (_fast(64, 0, 0, "bf16x3", 0), 128, 1), env=npipe)  # 768 workgroups >= 512
    add("switch", "bf16", 2, 64, 257, 65, 64, (_fast(64, 0, 0, "bf16", 0), 128, 1), env=npipe)      # 384 workgroups >= 256
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = _cases()
DEFAULT_CASES = [c for c in CASES if c.env is None]
SWITCH_CASES = [c for c in CASES if c.env is not None]

# Every kernel siu3r_attention can launch without an environment switch, written out by hand from the dispatch code
# (csrc/attention.hip: attn_route_of; csrc/attention_pipe.hip: siu3r_attn_pipe_ok).
KERNELS_DEFAULT = sorted([
    "siu3r_attn_pipe::attn_pipe_kernel<false, false>",   # bf16, D = 64, Nk >= 64, no mask, >= 192 128-query workgroups
    "siu3r_attn_pipe::attn_pipe_kernel<true, false>",    # bf16x3, D = 64, Nk >= 64, no mask
    "siu3r_attn_pipe::attn_pipe_kernel<true, true>",     # ... on pre-split K / V planes
    # fast kernels <D, MASK, SPLITKV, X3, KH>
    "attn_fast_kernel<32, 0, 0, 0, 0>", "attn_fast_kernel<32, 0, 0, 1, 0>",   # Nk < 64, or at / above 256 / 512 workgroups
    "attn_fast_kernel<64, 0, 0, 0, 0>", "attn_fast_kernel<64, 0, 0, 1, 0>",   # Nk < 64 only (D = 64 with more keys: key halves or pipelined)
    "attn_fast_kernel<32, 0, 0, 0, 1>", "attn_fast_kernel<32, 0, 0, 1, 1>", "attn_fast_kernel<64, 0, 0, 0, 1>",  # key halves (bf16x3 at D = 64 is pipelined)
    "attn_fast_kernel<32, 1, 0, 0, 0>", "attn_fast_kernel<32, 1, 0, 1, 0>", "attn_fast_kernel<64, 1, 0, 0, 0>", "attn_fast_kernel<64, 1, 0, 1, 0>",
    "attn_fast_kernel<32, 0, 1, 0, 0>", "attn_fast_kernel<32, 0, 1, 1, 0>", "attn_fast_kernel<64, 0, 1, 0, 0>", "attn_fast_kernel<64, 0, 1, 1, 0>",
    "attn_fast_kernel<32, 1, 1, 0, 0>", "attn_fast_kernel<32, 1, 1, 1, 0>", "attn_fast_kernel<64, 1, 1, 0, 0>", "attn_fast_kernel<64, 1, 1, 1, 0>",
    # register-staged kernels <D, IN_F32, SPLIT, MASK, QKX>: RoPE on load (D = 64; bf16 operands split the rotated q, k: QKX), fp32 tensors
    # without split3 (both D)
    "attn_kernel<64, 0, 0, 0, 1>", "attn_kernel<64, 0, 0, 1, 1>", "attn_kernel<64, 1, 0, 0, 1>", "attn_kernel<64, 1, 0, 1, 1>",
    "attn_kernel<64, 1, 1, 0, 0>", "attn_kernel<64, 1, 1, 1, 0>",
    "attn_kernel<64, 1, 0, 0, 0>", "attn_kernel<64, 1, 0, 1, 0>", "attn_kernel<32, 1, 0, 0, 0>", "attn_kernel<32, 1, 0, 1, 0>",
])
# ... and the instantiations only a switch reaches
KERNELS_SWITCH_ONLY = sorted([
    "attn_kernel<32, 0, 0, 0, 0>", "attn_kernel<32, 0, 0, 1, 0>", "attn_kernel<32, 1, 1, 0, 0>", "attn_kernel<32, 1, 1, 1, 0>",   # SIU3R_ATTN_NO_FAST
    "attn_kernel<64, 0, 0, 0, 0>", "attn_kernel<64, 0, 0, 1, 0>",                                                             # SIU3R_ATTN_NO_FAST
    "attn_fast_kernel<64, 0, 0, 1, 1>",                                                                                     # SIU3R_ATTN_NO_PIPE
])
