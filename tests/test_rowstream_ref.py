"""CPU checks of tests/dense_rowstream64.py: the float64 restatements against float64 torch; a float32 emulation of each kernel's
arithmetic (A hi by truncation and A lo by round-to-nearest, W hi / lo by round-to-nearest, three products per K step accumulated in
fp32 in the kernel's K order, fp32 coordinates and lerp as the kernel writes them) that must stay within the derived bound at every
case; the wrong answers the kernels can give -- the same emulation with one mutation each -- which must exceed it and are named by
their worst element; the UR / UC window invariant of stem.hip in numpy float32; the launch arithmetic against the properties every case
is there for; and ops.proj_rows_ok against the dispatch of siu3r_proj_rows_x3.  (ops.pack_stem7 / ops.pack_proj refuse CPU tensors:
their round trip is in tests/test_rowstream_gpu.py.)"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_rowstream64 as R  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# the kernel's coordinates, operation by operation, in numpy float32 (stem.hip: ry / rx, yb / xb, fy, y0, y1, ly)
# ------------------------------------------------------------------------------------------------
def coords32(n_out, n_src, tile, align_corners=True):
    """per output row (column) o: (i0, i1, l, origin of o's tile window); `tile` = 8 rows / 16 columns"""
    r = f32(n_src - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    o = np.arange(n_out)
    fo = (r * o.astype(f32)).astype(f32)
    if not align_corners:
        fo = np.maximum((o.astype(f32) + f32(0.5)) * f32(0.5) - f32(0.5), f32(0)).astype(f32)
    i0 = fo.astype(np.int64)                       # (int): truncation, fo >= 0
    i1 = i0 + (i0 < n_src - 1)
    l = (fo - i0.astype(f32)).astype(f32)
    origin = (r * ((o // tile) * tile).astype(f32)).astype(f32).astype(np.int64)
    return i0, i1, l, origin


# ------------------------------------------------------------------------------------------------
# stem: emulation and wrong answers
# ------------------------------------------------------------------------------------------------
STEM_CONV_MUTS = ("transpose", "clamp_border", "drop_lh")
STEM_UP_MUTS = ("stale_up", "no_clamp", "align_off", "origin_off")
DROP_STEP = 6   # ky = 3, kx = 0 .. 3: holds the centre tap
_emu_cache = {}


class StemEmulation:
    def __init__(self, c, inp):
        self.c, self.inp = c, inp

    def conv(self, mut=None):
        """fp32 accumulators [B, G, H, W, 256]: 14 K steps of 16 in the order k = (ky, kx in 0..7, c in 0..3); per step
        A_hi W_hi, A_lo W_hi, A_hi W_lo"""
        c, inp = self.c, self.inp
        if mut is None and _emu_cache.get("shape") == c.shape:
            return _emu_cache["acc"]
        w_hi, w_lo = inp["w_hi"], inp["w_lo"]
        if mut == "transpose":
            w_hi, w_lo = w_hi.transpose(-1, -2), w_lo.transpose(-1, -2)
        whi, wlo = R.stem_weights(w_hi, 8, 4), R.stem_weights(w_lo, 8, 4)
        acc = torch.empty(c.B, c.G, c.H, c.W, R.STEM_C)
        for b in range(c.B):
            for g in range(c.G):
                A = R.stem_patches(inp["img"][b, g], 8, 4, mode="replicate" if mut == "clamp_border" else "constant")
                ahi = R.trunc_bf16(A)
                alo = R.rne_bf16(A - ahi)
                a = torch.zeros(c.H * c.W, R.STEM_C)
                for s in range(R.STEM_KPAD // 16):
                    k = slice(16 * s, 16 * s + 16)
                    a = a + ahi[:, k] @ whi[g][:, k].t()
                    if not (mut == "drop_lh" and s == DROP_STEP):
                        a = a + alo[:, k] @ whi[g][:, k].t()
                    a = a + ahi[:, k] @ wlo[g][:, k].t()
                acc[b, g] = a.view(c.H, c.W, R.STEM_C)
        if mut is None:
            _emu_cache.clear()
            _emu_cache.update(shape=c.shape, acc=acc)
        return acc

    def _tiles(self):
        """tile number of every pixel [B, H, W] and whether a workgroup runs it as a second or later tile"""
        c = self.c
        b, oy, ox = np.arange(c.B)[:, None, None], np.arange(c.H)[None, :, None], np.arange(c.W)[None, None, :]
        t = b * c.per_img + (oy // R.STEM_TH) * (c.W // R.STEM_TW) + ox // R.STEM_TW
        return t, t >= c.nwg

    def upsample(self, mut=None):
        """fp32 [B, G, H, W, 256]: the four corners gathered by flat source-pixel index (an index past the source reads NaN)"""
        c = self.c
        src = self.inp["up"].reshape(c.Z * c.sh * c.sw, R.STEM_C)
        src = torch.cat((src, torch.full((c.sw + 2, R.STEM_C), float("nan"))))
        ac = mut != "align_off"
        y0, y1, ly, yb = coords32(c.H, c.sh, R.STEM_TH, ac)
        x0, x1, lx, xb = coords32(c.W, c.sw, R.STEM_TW, ac)
        if mut == "no_clamp":
            y1, x1 = y0 + 1, x0 + 1
        if mut == "origin_off":
            x0, x1 = np.minimum(x0 + 1, c.sw - 1), np.minimum(x1 + 1, c.sw - 1)
        bs = np.arange(c.B)[:, None, None]
        Y0, Y1, X0, X1 = y0[None, :, None], y1[None, :, None], x0[None, None, :], x1[None, None, :]
        if mut == "stale_up":   # the window in LDS is that of tile t - nwg: its batch item, its origin, its clamp
            t, stale = self._tiles()
            t2 = np.where(stale, t - c.nwg, t)
            tx_n = c.W // R.STEM_TW
            b2, r2 = t2 // c.per_img, t2 % c.per_img
            oyb, oxb = yb[(r2 // tx_n) * R.STEM_TH], xb[(r2 % tx_n) * R.STEM_TW]
            bs = b2
            Y0, Y1 = (np.minimum(oyb + (y - yb)[None, :, None], c.sh - 1) for y in (y0, y1))
            X0, X1 = (np.minimum(oxb + (x - xb)[None, None, :], c.sw - 1) for x in (x0, x1))
        g = np.arange(c.G)[None, :, None, None]

        def corner(Y, X):
            p = ((np.broadcast_to(bs, (c.B, c.H, c.W))[:, None] * c.G + g) * c.sh + np.broadcast_to(Y, (c.B, c.H, c.W))[:, None]) * c.sw \
                + np.broadcast_to(X, (c.B, c.H, c.W))[:, None]
            return src[torch.from_numpy(np.minimum(p, src.shape[0] - 1))]
        ly_, lx_ = torch.from_numpy(ly)[:, None, None], torch.from_numpy(lx)[None, :, None]
        return R.lerp4(corner(Y0, X0), corner(Y0, X1), corner(Y1, X0), corner(Y1, X1), ly_, lx_)

    def run(self, mut=None):
        c = self.c
        acc = self.conv(mut if mut in STEM_CONV_MUTS else None)
        if mut == "stale_raw":   # tile t of a workgroup computed from the patch of its previous tile t - nwg
            ty_n, tx_n = c.H // R.STEM_TH, c.W // R.STEM_TW
            tl = acc.view(c.B, c.G, ty_n, R.STEM_TH, tx_n, R.STEM_TW, R.STEM_C).permute(1, 0, 2, 4, 3, 5, 6).reshape(c.G, c.ntiles, R.STEM_TH, R.STEM_TW, R.STEM_C)
            tl = torch.cat((tl[:, :c.nwg], tl[:, :c.ntiles - c.nwg]), dim=1)
            acc = tl.view(c.G, c.B, ty_n, tx_n, R.STEM_TH, R.STEM_TW, R.STEM_C).permute(1, 0, 2, 4, 3, 5, 6).reshape(c.B, c.G, c.H, c.W, R.STEM_C)
        if c.bias:
            bias = self.inp["bias"]
            if mut == "bias_head":   # head z / G (wrapped into the G sets) in place of z % G
                acc = acc + bias[[b % c.G for b in range(c.B)]][:, None, None, None, :]
            else:
                acc = acc + bias[None, :, None, None, :]
        v = acc.clamp_min(0)
        if c.up:
            v = v + self.upsample(mut if mut in STEM_UP_MUTS else None)
        return v


def stem_mutations(c):
    """the wrong answers that apply to a case (those that recompute the convolution: on the small shapes and the impulse images)"""
    out = []
    small = c.Z * c.H * c.W <= 8192
    if small or c.impulse:
        out += ["transpose", "clamp_border"]
    if c.impulse:
        out += ["drop_lh"]
    if "single" not in c.props:
        out += ["stale_raw"] + (["stale_up"] if c.up else [])
    if c.up:
        out += ["no_clamp", "align_off", "origin_off"]
    if c.bias and c.G > 1 and c.B > 1:
        out += ["bias_head"]
    return out


def _ratio(got, ref, bnd):
    return R.worst_ratio(got, ref["out"], ref["S"], bnd, ref.get("extra"))


STEM_SEEN = {}


@pytest.mark.parametrize("c", R.STEM_CASES, ids=[c.id for c in R.STEM_CASES])
def test_stem_emulation_within_bound_and_wrong_answers_over_it(c):
    per = c.check_props()
    inp = R.stem_inputs(c)
    ref = R.stem_reference(c, inp)
    emu = StemEmulation(c, inp)
    w, idx = _ratio(emu.run(), ref, R.STEM_BOUND)
    print(f"[rowstream] {c.id}: grid {c.nwg} x {c.G}, {c.ntiles} tiles (per workgroup {max(per)} .. {min(per)}); emulation worst {w:.3f} of the bound at {idx}")
    assert w <= 1.0, f"{c.id}: the float32 emulation is {w:.2f} x the bound at (b, g, y, x, n) = {idx}"
    for mut in stem_mutations(c):
        wm, im = _ratio(emu.run(mut), ref, R.STEM_BOUND)
        print(f"[rowstream] {c.id}: {mut}: {wm:.3g} x the bound at (b, g, y, x, n) = {im}")
        assert wm > 1.0, f"{c.id}: wrong answer `{mut}` passes ({wm:.3f} of the bound at {im})"
        STEM_SEEN.setdefault(mut, []).append(c.id)


def test_every_stem_wrong_answer_has_a_case():
    want = set(STEM_CONV_MUTS + STEM_UP_MUTS + ("stale_raw", "bias_head"))
    have = {m for c in R.STEM_CASES for m in stem_mutations(c)}
    assert have == want, (want - have, have - want)
    # the multi-tile wrong answers are caught at the production head count too
    assert any(c.G == 2 and "stale_raw" in stem_mutations(c) for c in R.STEM_CASES)
    assert any(c.G == 2 and "stale_up" in stem_mutations(c) for c in R.STEM_CASES)


def test_stem_reference_is_float64_torch():
    for c in R.STEM_CASES:
        if c.Z * c.H * c.W > 8192 or not (c.up and c.bias):
            continue
        inp = R.stem_inputs(c)
        ref = R.stem_reference(c, inp)["out"]
        w = (inp["w_hi"].double() + inp["w_lo"].double())
        for g in range(c.G):
            x = inp["img"][:, g, :, :, :3].double().permute(0, 3, 1, 2)
            y = F.relu(F.conv2d(x, w[g], inp["bias"][g].double(), padding=3))
            y = y + F.interpolate(inp["up"][:, g].double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
            assert torch.allclose(ref[:, g], y.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12), c.id


def test_stem_impulses_pin_every_tap():
    """every one of the 147 taps is, at some output pixel of the impulse images, the only non-zero product -- in every channel slot"""
    c = next(c for c in R.STEM_CASES if c.impulse)
    inp = R.stem_inputs(c)
    seen = torch.zeros(3, 7, 7, dtype=torch.bool)
    for z in range(c.Z):
        img = inp["img"][z // c.G, z % c.G]
        (y, x, ch), = [tuple(int(v) for v in i) for i in img.nonzero()]
        assert (y, x) in R.impulse_sites(c.H, c.W) and ch < 3
        for ky in range(7):
            for kx in range(7):
                if 0 <= y - ky + 3 < c.H and 0 <= x - kx + 3 < c.W:
                    seen[ch, ky, kx] = True
    assert seen.all()
    S = R.stem_reference(c, inp)["S"]
    assert float(S.max()) <= 0.5 + 0.2 + 1e-6 and float(S.min()) >= 0.25   # one tap (|a| <= 1, |w| <= 0.2) plus the bias


# ------------------------------------------------------------------------------------------------
# proj: emulation and wrong answers
# ------------------------------------------------------------------------------------------------
class ProjEmulation:
    def __init__(self, c, inp):
        self.c, self.inp = c, inp
        self.ahi = R.trunc_bf16(inp["x"])
        self.alo = R.rne_bf16(inp["x"] - self.ahi)

    def acc(self, mut=None, step=None):
        c = self.c
        zi = [((z // c.G) % c.G if mut == "w_of_z_div_g" else z % c.G) for z in range(c.Z)]
        whi, wlo = self.inp["w_hi"][zi], self.inp["w_lo"][zi]
        steps = list(range(c.K // 16))
        if mut == "skip":
            steps.remove(step)
        if mut == "twice":
            steps.insert(step, step)
        a = torch.zeros(c.Z, c.M, c.N)
        mm = lambda x, w, k: torch.einsum("zmk,znk->zmn", x[..., k], w[..., k])
        for s in steps:
            k = slice(16 * s, 16 * s + 16)
            a = a + mm(self.ahi, whi, k)
            if not (mut == "drop_lh" and s == step):
                a = a + mm(self.alo, whi, k)
            a = a + mm(self.ahi, wlo, k)
        return a

    def run(self, mut=None, step=None, base=None):
        c = self.c
        out = base if base is not None else self.acc(mut, step)
        if c.bias:
            b = self.inp["bias"][[z % c.G for z in range(c.Z)]]
            if mut == "bias_shift":   # column blocks 1 and 2 read the bias one column further
                sh = torch.cat((b[:, 1:], torch.zeros(c.Z, 1)), dim=1)
                b = torch.where(torch.arange(c.N)[None, :] >= 32, sh, b)
            out = out + b[:, None, :]
        if mut == "stale":            # tile i + nwg computed from the rows of tile i
            n = c.nwg * c.rows
            out = torch.cat((out[:, :n], out[:, :c.M - n]), dim=1)
        return out


def proj_mutations(c):
    """(kind, where): the K-step wrong answers are placed in the step of the first sentinel column of W (every dense row of x shows it
    there at full scale); those that recompute the accumulation run on the small cases"""
    out = []
    small = c.Z * c.M * c.N <= 600_000
    if small:
        out += [("skip", "w"), ("twice", "w"), ("drop_lh", "w")]
        if c.G > 1 and c.B > 1:
            out += [("w_of_z_div_g", None)]
    if c.ntiles > c.nwg:
        out += [("stale", None)]
    if c.bias and c.N > 33:
        out += [("bias_shift", None)]
    return out


@pytest.mark.parametrize("c", R.PROJ_CASES, ids=[c.id for c in R.PROJ_CASES])
def test_proj_emulation_within_bound_and_wrong_answers_over_it(c):
    per = c.check_props()
    inp = R.proj_inputs(c)
    ref = R.proj_reference(c, inp)
    emu = ProjEmulation(c, inp)
    bnd = R.proj_bound(c)
    base = emu.acc()
    w, idx = _ratio(emu.run(base=base), ref, bnd)
    print(f"[rowstream] {c.id}: grid {c.nwg} x {c.Z}, {c.ntiles} tiles of {c.rows} rows (per workgroup {max(per)} .. {min(per)}); emulation worst {w:.3f} of the bound at {idx}")
    assert w <= 1.0, f"{c.id}: the float32 emulation is {w:.2f} x the bound at (z, m, n) = {idx}"
    wstep = next(s for (kind, _, s) in inp["sentinels"] if kind == ("w" if c.M > 1 else "x"))   # (a single row of x: that row's own step)
    for (mut, where) in proj_mutations(c):
        step = wstep if where == "w" else None
        got = emu.run(mut, step) if mut in ("skip", "twice", "drop_lh", "w_of_z_div_g") else emu.run(mut, base=base)
        wm, im = _ratio(got, ref, bnd)
        print(f"[rowstream] {c.id}: {mut}{'' if step is None else f' (step {step})'}: {wm:.3g} x the bound at (z, m, n) = {im}")
        assert wm > 1.0, f"{c.id}: wrong answer `{mut}` passes ({wm:.3f} of the bound at {im})"


def test_every_proj_wrong_answer_has_a_case():
    have = {m for c in R.PROJ_CASES for (m, _) in proj_mutations(c)}
    assert have == {"skip", "twice", "drop_lh", "w_of_z_div_g", "stale", "bias_shift"}, have
    for K in (128, 256):   # both instantiations meet the stale prefetch; K 256 (three column blocks) the shifted bias
        assert any(c.K == K and ("stale", None) in proj_mutations(c) for c in R.PROJ_CASES)
    steps = {next(s for (kind, _, s) in R.proj_inputs(c)["sentinels"] if kind == "w") for c in R.PROJ_CASES if ("skip", "w") in proj_mutations(c)}
    print(f"[rowstream] K steps the skipped / doubled / dropped wrong answers were placed in: {sorted(steps)}")


def test_proj_reference_is_float64_torch():
    for c in R.PROJ_CASES:
        if c.Z * c.M * c.N > 600_000:
            continue
        inp = R.proj_inputs(c)
        ref = R.proj_reference(c, inp)["out"]
        w = inp["w_hi"].double() + inp["w_lo"].double()
        for z in range(c.Z):
            want = F.linear(inp["x"][z].double(), w[z % c.G], inp["bias"][z % c.G].double() if c.bias else None)
            assert torch.allclose(ref[z], want, rtol=1e-12, atol=1e-12), (c.id, z)


def test_proj_sentinels_cover_first_second_and_last_step():
    for c in R.PROJ_CASES:
        inp = R.proj_inputs(c)
        for kind in ("x", "w"):
            steps = {s for (k, _, s) in inp["sentinels"] if k == kind}
            if (kind == "x" and c.M >= 33) or (kind == "w" and c.N >= 33):
                assert steps == {0, 1, c.K // 16 - 1}, (c.id, kind, steps)
        for (kind, i, s) in inp["sentinels"]:
            row = inp["x"][:, i] if kind == "x" else inp["W"][:, i]
            out = torch.cat((row[..., :16 * s], row[..., 16 * s + 16:]), dim=-1)
            assert not out.any() and row.any(), (c.id, kind, i, s)


# ------------------------------------------------------------------------------------------------
# invariants
# ------------------------------------------------------------------------------------------------
def test_upsample_window_never_exceeds_ur_uc():
    """UR = 6, UC = 10 of stem.hip: over every H (W) = 16 .. 2048 and every tile, the rows (columns) of the x2 source map a 16 x 8 tile
    touches, counted from the tile's window origin yb (xb), are 0 .. 5 (0 .. 9) -- reached exactly, with nothing to spare -- and the
    min(.., sh - 1) clamp of the window fill never changes an index the tile reads"""
    worst = {}
    for (tile, cap, name) in ((R.STEM_TH, 6, "rows"), (R.STEM_TW, 10, "columns")):
        hi = 0
        for n in range(16, 2049, 16):
            ns = n // 2
            i0, i1, _, origin = coords32(n, ns, tile)
            assert (i0 - origin >= 0).all(), (name, n)
            assert (i1 - origin <= cap - 1).all(), (name, n, int((i1 - origin).max()))
            assert (i1 <= ns - 1).all() and (i1 >= i0).all()
            fill = np.minimum(origin[:, None] + np.arange(cap)[None, :], ns - 1)     # the window as the kernel fills it
            o = np.arange(n)
            assert (fill[o, i0 - origin] == i0).all() and (fill[o, i1 - origin] == i1).all(), (name, n)
            hi = max(hi, int((i1 - origin).max()))
        worst[name] = hi
    print(f"[rowstream] largest window index reached over H, W = 16 .. 2048: rows {worst['rows']} (UR - 1 = 5), columns {worst['columns']} (UC - 1 = 9)")
    assert worst == {"rows": 5, "columns": 9}


def test_launch_arithmetic():
    assert R.stem_grid(2, 2, 48, 32) == (24, 24)
    assert R.stem_grid(3, 16, 32, 48) == (16, 36) and R.tiles_per_wg(16, 36) == [3] * 4 + [2] * 12
    assert R.stem_grid(3, 2, 64, 128) == (128, 192) and R.tiles_per_wg(128, 192) == [2] * 64 + [1] * 64
    assert R.stem_grid(5, 2, 64, 128) == (128, 320) and R.tiles_per_wg(128, 320) == [3] * 64 + [2] * 64
    assert R.stem_grid(1, 1, 16, 16) == (2, 2)
    assert R.stem_grid(1, 2, 512, 512) == (128, 2048)              # a production pair
    assert R.proj_grid(32, 1093, 256, 83) == (8, 18, 64) and R.tiles_per_wg(8, 18) == [3, 3] + [2] * 6 and 1093 - 17 * 64 == 5
    assert R.proj_grid(32, 2181, 128, 3) == (8, 18, 128) and 2181 - 17 * 128 == 5
    assert R.proj_grid(258, 70, 256, 83) == (1, 2, 64)
    assert R.proj_grid(4, 1000, 256, 83) == (16, 16, 64) and R.proj_grid(4, 4096, 128, 4) == (32, 32, 128)   # test_kernels_gpu.py: one tile each
    for c in R.STEM_CASES + R.PROJ_CASES:
        c.check_props()
    # what the multi-tile cases are there for, per kernel and at the production head count
    assert any({"multi3", "ragged", "cross"} <= set(c.props) for c in R.STEM_CASES)
    assert any(c.G == 2 and {"multi2", "ragged", "cross"} <= set(c.props) for c in R.STEM_CASES)
    assert any(c.G == 2 and {"multi3", "ragged", "cross"} <= set(c.props) for c in R.STEM_CASES)
    for K in (128, 256):
        assert any(c.K == K and c.G == 2 and {"multi3", "ragged", "zg"} <= set(c.props) for c in R.PROJ_CASES)
        assert any(c.K == K and "clamp" in c.props for c in R.PROJ_CASES)


def test_proj_rows_ok_is_the_dispatch():
    from siu3r_amd import ops

    for K in (64, 128, 256):
        for n in range(1, 129):
            assert bool(ops.proj_rows_ok(K, n)) == R.proj_dispatch(K, n), (K, n)


def test_parity_record_lists_every_case():
    """profiles/rowstream_parity.json (a record of one MI355X run; no bound comes from it) names every case of the GPU module"""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = json.load(open(os.path.join(root, "profiles", "rowstream_parity.json")))["cases"]
    assert set(rec) == {c.id for c in R.STEM_CASES + R.PROJ_CASES}
    assert all(0.0 < r["worst_ratio"] <= 1.0 for r in rec.values())
    for c in R.STEM_CASES + R.PROJ_CASES:
        per = R.tiles_per_wg(c.nwg, c.ntiles)
        assert rec[c.id]["grid"][0] == c.nwg and rec[c.id]["tiles"] == c.ntiles and rec[c.id]["tiles_per_wg"] == [max(per), min(per)], c.id
