"""The rasterizer's three integer stages -- siu3r_raster_sort, siu3r_raster_bin, siu3r_raster_tile_lists (csrc/raster.hip) -- called
directly through the C ABI on crafted keys, counts and rects, and compared bit for bit with tests/raster_stages_ref.py (plain numpy,
itself checked against brute-force loops in tests/test_raster_stages_ref.py).  Every output buffer is carved out of a larger
sentinel-filled tensor: after each call the guard bands, and the tails the contract leaves alone, must still hold the sentinel.

Then the same stages inside real calls at the geometries no render test reaches: frames whose coarse bins are 8 and 16 tiles wide,
more than 16 views in one call, and the state of a multi-view call against the stage references."""
import functools

import numpy as np
import pytest
import torch

import raster_stages_ref as R
from scenes import default_K, look_at_camera, random_scene

pytestmark = pytest.mark.gpu

SENT = -0x5A5A5A5B  # int32 sentinel: negative, so never a Gaussian id, an offset or a count
PAD = 1024          # guard elements on either side of a buffer


class _Guarded:
    """a tensor of `shape` inside a larger one; everything starts as the sentinel"""

    def __init__(self, shape, dtype=torch.int32):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device="cuda")
        self.t = self.whole[PAD:PAD + n].view(shape)

    def guards_intact(self):
        return bool((self.whole[:PAD] == SENT).all()) and bool((self.whole[-PAD:] == SENT).all())

    def untouched(self):
        return bool((self.whole == SENT).all())


def _cams(width, height, V=1):
    """identity pose: the three stages read mode, width and height only"""
    from siu3r_amd import raster

    cam = raster.make_cam_k3(torch.eye(4), 100.0, 100.0, width / 2, height / 2, width, height)
    return raster._cam_array([cam] * V)


def _stats(counts):
    """int64 [V,4], zero except [v][0] = the visible count: the documented precondition of stages 2 and 3"""
    st = _Guarded((len(counts), 4), torch.int64)
    st.t.zero_()
    st.t[:, 0] = torch.tensor(counts, dtype=torch.int64)
    return st


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a, np.int32)


def _up(guarded, a):
    guarded.t.copy_(torch.from_numpy(_i32(a)).view(guarded.t.shape))


def _np(t):
    return t.cpu().numpy()


# ---- sort ----------------------------------------------------------------------------------------------------------------------------
def _check_sort(keys):
    """keys uint32 [V,G] -> runs siu3r_raster_sort and checks keys_a / ids_a [v][0, n) against sort_ref, the tails and the guards"""
    from siu3r_amd import _lib, raster
    from siu3r_amd.ops import _p, _stream

    keys = np.ascontiguousarray(keys, np.uint32)
    V, G = keys.shape
    ref = R.sort_ref(keys)
    nch = raster.geometry(16, 16, G)["nchunks_sort"]
    assert nch == -(-G // 4096)
    ka, kb, ia, ib = (_Guarded((V, G)) for _ in range(4))
    hist, tot = _Guarded((V, 256, nch)), _Guarded((V, 256))
    _up(ka, keys)
    stats = _stats([n for _, _, n in ref])
    stats_before = stats.whole.clone()
    _lib.check(_lib.lib().siu3r_raster_sort(V, G, _p(ka.t), _p(kb.t), _p(ia.t), _p(ib.t), _p(hist.t), _p(tot.t), _p(stats.t), _stream()))
    torch.cuda.synchronize()
    keys_in = torch.from_numpy(_i32(keys)).cuda()
    for v, (want_k, want_i, n) in enumerate(ref):
        got_k, got_i = _np(ka.t[v, :n]).view(np.uint32), _np(ia.t[v, :n])
        assert np.array_equal(got_k, want_k), f"view {v}: sorted keys differ (n = {n})"
        assert np.array_equal(got_i, want_i), f"view {v}: sorted ids differ (n = {n}): the sort is not stable, or lost a key"
        # behind the n visible ones nothing is written: the input keys stay, the other three buffers keep the sentinel
        assert torch.equal(ka.t[v, n:], keys_in[v, n:]), f"view {v}: keys_a written at or behind n = {n}"
        for name, b in (("keys_b", kb), ("ids_a", ia), ("ids_b", ib)):
            assert bool((b.t[v, n:] == SENT).all()), f"view {v}: {name} written at or behind n = {n}"
    for name, b in (("keys_a", ka), ("keys_b", kb), ("ids_a", ia), ("ids_b", ib), ("rs_hist", hist), ("rs_tot", tot)):
        assert b.guards_intact(), f"{name}: written outside the buffer"
    assert torch.equal(stats.whole, stats_before), "the sort takes stats as const"


def _rand_keys(rng, G):
    return rng.integers(0, 2 ** 32, G, dtype=np.uint64).astype(np.uint32)


def _key_pattern(name, G):
    rng = np.random.default_rng(G % 1000 + sum(map(ord, name)))
    k = _rand_keys(rng, G)
    if name == "random46":
        k[rng.random(G) < 0.46] = R.CULLED
    elif name == "none_culled":
        k[k == R.CULLED] = 0xFFFFFFFE
    elif name == "one_visible":
        k[:] = R.CULLED
        k[G // 3] = 0x40490FDB
    elif name == "all_culled":
        k[:] = R.CULLED
    elif name == "all_equal":
        k[:] = 0x3F800000
    elif name == "forty_values":
        k = _rand_keys(rng, 40)[rng.integers(0, 40, G)]
    elif name.startswith("byte"):
        b = int(name[4])
        k = np.uint32(0x12345678 & ~(0xFF << (8 * b))) | (rng.integers(0, 256, G).astype(np.uint32) << np.uint32(8 * b))
    elif name == "ascending":
        k = np.sort(k)
    elif name == "descending":
        k = np.sort(k)[::-1].copy()
    elif name == "extremes":
        k[rng.random(G) < 0.46] = R.CULLED
        for val in (0, 0x7F7FFFFF, 0x80000000, 0xFFFFFFFE):
            k[rng.integers(0, G, max(4, G // 50))] = val  # each many times over: their ties must come out in index order
    else:
        raise KeyError(name)
    return k


_PATTERNS = ["random46", "none_culled", "one_visible", "all_culled", "all_equal", "forty_values", "byte0", "byte1", "byte2", "byte3",
             "ascending", "descending", "extremes"]


@pytest.mark.parametrize("G", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 262144, 262145, 524289])
def test_sort_sizes(G):
    """one key up to two chunks and a key; then 64, 65 and 129 histogram columns: the row scan's carry across one and two 64-column
    blocks (row_scan_kernel), which no render test below 262 145 Gaussians reaches"""
    _check_sort(_key_pattern("random46", G)[None])


@pytest.mark.parametrize("G", [8193, 262145])
@pytest.mark.parametrize("pattern", _PATTERNS)
def test_sort_key_patterns(pattern, G):
    """keys a random scene never has: one digit per pass with full 64-lane groups (all_equal: the per-group counts at their maximum and
    ids ascending), a single varying byte, the top bit set, nothing or one key visible"""
    keys = _key_pattern(pattern, G)
    if pattern == "extremes":
        assert all((keys == val).sum() >= 4 for val in (0, 0x7F7FFFFF, 0x80000000, 0xFFFFFFFE))
    if pattern == "random46":
        assert 0.44 < (keys == R.CULLED).mean() < 0.48
    _check_sort(keys[None])


@pytest.mark.parametrize("G", [4096 + 100, 6000])
def test_sort_all_equal_keys_with_a_ragged_last_chunk(G):
    """all keys equal where the last chunk ends inside a wave: at 8193 and 262 145 every (slice, wave) group of a chunk has 64 keys (or the
    chunk has one key), and a scatter that walks the groups of a digit in the wrong order undoes its own damage over the four passes"""
    _check_sort(np.full((1, G), 0x3F800000, np.uint32))


@pytest.mark.parametrize("visible", ["lane0", "lane63", "odd_waves", "odd_slices", "not_first_chunk", "not_last_chunk"])
def test_sort_culling_aligned_to_the_kernel(visible):
    """culling along the scatter's own structure (64-lane waves, 256-key slices, 4096-key chunks; G = two chunks and a partial one):
    empty ballots, empty slices, a chunk that contributes nothing in pass 0"""
    G = 2 * 4096 + 1500
    i = np.arange(G)
    keep = {"lane0": i % 64 == 0, "lane63": i % 64 == 63, "odd_waves": (i // 64) % 2 == 1, "odd_slices": (i // 256) % 2 == 1,
            "not_first_chunk": i >= 4096, "not_last_chunk": i < 8192}[visible]
    rng = np.random.default_rng(11)
    keys = _rand_keys(rng, 500)[rng.integers(0, 500, G)]  # (ties throughout)
    keys[~keep] = R.CULLED
    _check_sort(keys[None])


def test_sort_views_do_not_affect_each_other():
    G = 8193
    keys = np.stack((_key_pattern("random46", G), _key_pattern("all_culled", G), _key_pattern("all_equal", G)))
    _check_sort(keys)
    _check_sort(keys[::-1])


# ---- binning and tile lists: crafted cases --------------------------------------------------------------------------------------------
def _rand_rects(rng, geo, G, lo, hi):
    """G rects of lo .. hi tiles per side (cut to the frame), anywhere in the frame"""
    w, h = np.minimum(rng.integers(lo, hi + 1, G), geo["gw"]), np.minimum(rng.integers(lo, hi + 1, G), geo["gh"])
    x0, y0 = rng.integers(0, geo["gw"] - w + 1), rng.integers(0, geo["gh"] - h + 1)
    return np.stack((x0, y0, x0 + w, y0 + h), -1).astype(np.int32)


def _prefix(rng, G, n):
    return rng.permutation(G)[:n].astype(np.int32)


def _special_rects(geo):
    """rects of exactly one bin, aligned to it (a clipped x1 / y1 reaches cb), and 2 x 2-tile rects on a corner shared by four bins"""
    cb, out = geo["cb"], []
    for by in range(0, geo["nby"] - 1, max(1, geo["nby"] // 5)):
        for bx in range(0, geo["nbx"] - 1, max(1, geo["nbx"] // 5)):
            out.append((bx * cb, by * cb, bx * cb + cb, by * cb + cb))
            out.append((bx * cb + cb - 1, by * cb + cb - 1, bx * cb + cb + 1, by * cb + cb + 1))
    return np.array(out, np.int32)


def _border_rects(rng, geo):
    """every x range that starts or ends on a bin border, with random y ranges, and the other way round; the four corner tiles"""
    cb, gw, gh = geo["cb"], geo["gw"], geo["gh"]
    xs = [(a, b) for a in range(gw) for b in range(a + 1, gw + 1)]
    ys = [(a, b) for a in range(gh) for b in range(a + 1, gh + 1)]
    out = []
    for on, other, swap in ((xs, ys, False), (ys, xs, True)):
        for a, b in on:
            if a % cb == 0 or b % cb == 0:
                for j in rng.integers(0, len(other), 3):
                    c, d = other[j]
                    out.append((c, a, d, b) if swap else (a, c, b, d))
    out += [(0, 0, 1, 1), (gw - 1, 0, gw, 1), (0, gh - 1, 1, gh), (gw - 1, gh - 1, gw, gh)]
    return np.array(out, np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict(W, H, geo, rect [V,G,4], sorted_ids [per view], bins [per view (bin_start, entries)], lists [per view (tile_start, ids)]);
    the references are computed once and shared by the binning and the tile-list tests (which only read them)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    W, H = 208, 160  # 13 x 10 tiles: ragged bins on both axes
    if name[0] == "n" and name[1:].isdigit():
        n = int(name[1:])
        geo = R.geometry_ref(W, H)
        rect = _rand_rects(rng, geo, n + 50, 1, 2 if n > 100000 else 3)
        ids = [_prefix(rng, n + 50, n)]
    elif name == "full_frame_600":  # every bit-matrix row full in every slice: rank 255 of 256
        geo = R.geometry_ref(W, H)
        rect = np.tile(np.array([0, 0, geo["gw"], geo["gh"]], np.int32), (600, 1))
        ids = [_prefix(rng, 600, 600)]
    elif name == "bin_borders":
        geo = R.geometry_ref(W, H)
        rect = _border_rects(rng, geo)
        ids = [_prefix(rng, len(rect), len(rect))]
    elif name == "one_bin_700":  # 700 entries in bin 0 (three slices of tl_write_kernel's walk), a few dozen of them on any one tile
        geo = R.geometry_ref(W, H)
        x0, y0 = rng.integers(0, 4, 700), rng.integers(0, 4, 700)
        rect = np.stack((x0, y0, x0 + 1, y0 + 1), -1).astype(np.int32)
        ids = [_prefix(rng, 700, 700)]
    elif name == "two_views_one_empty":
        geo = R.geometry_ref(W, H)
        rect = _rand_rects(rng, geo, 350, 1, 3)
        ids = [_prefix(rng, 350, 300), np.zeros(0, np.int32)]
    elif name == "nb1024":  # 32 x 32 bins: thread 255 of bin_scatter_kernel owns bins 1020 .. 1023
        W = H = 2048
        geo = R.geometry_ref(W, H)
        rect = np.concatenate((_rand_rects(rng, geo, 300, 1, 3), np.tile(np.array([0, 0, 128, 128], np.int32), (4, 1))))
        ids = [_prefix(rng, 304, 304)]
    elif name in ("cb8", "cb16"):
        W = H = 2112 if name == "cb8" else 4224
        geo = R.geometry_ref(W, H)
        rect = np.concatenate((_rand_rects(rng, geo, 400, 1, 40), _special_rects(geo)))
        ids = [_prefix(rng, len(rect), len(rect) - 15)]
    elif name in ("t1023", "t1024", "t1025"):
        W, H = {"t1023": (528, 496), "t1024": (512, 512), "t1025": (16400, 16)}[name]
        geo = R.geometry_ref(W, H)
        rect = _rand_rects(rng, geo, 500, 1, 5)
        rect[:3] = (geo["gw"] - 1, geo["gh"] - 1, geo["gw"], geo["gh"])  # the last tile has a list
        ids = [_prefix(rng, 500, 480)]
    else:
        raise KeyError(name)
    V = len(ids)
    used = np.zeros((V, len(rect)), bool)
    for v in range(V):
        used[v, ids[v]] = True
    rect = np.where(used[:, :, None], rect[None], 0).astype(np.int32)  # what projection leaves for a Gaussian outside the view
    bins = [R.bin_ref(geo, ids[v], rect[v]) for v in range(V)]
    lists = [R.tile_lists_ref(geo, *bins[v]) for v in range(V)]
    for v in range(V):  # the two routes to the lists agree, or the reference itself is wrong
        ts, li = R.tile_lists_direct(geo, ids[v], rect[v])
        assert np.array_equal(ts, lists[v][0]) and np.array_equal(li, lists[v][1])
    return dict(W=W, H=H, geo=geo, rect=rect, sorted_ids=ids, bins=bins, lists=lists)


_BIN_CASES = ["n1", "n255", "n256", "n257", "n2047", "n2048", "n2049", "n131073", "full_frame_600", "bin_borders", "one_bin_700",
              "two_views_one_empty", "nb1024", "cb8", "cb16", "t1023", "t1024", "t1025"]


def _geometry(case, G):
    from siu3r_amd import raster

    geo, lib_geo = case["geo"], raster.geometry(case["W"], case["H"], G)
    assert all(lib_geo[k] == geo[k] for k in ("gw", "gh", "T", "cb", "NB")), (lib_geo, geo)
    assert lib_geo["nchunks_bin"] == -(-G // 2048)
    return lib_geo


def _run_bin(case, cap_e):
    """uploads the case, runs siu3r_raster_bin -> (return code, buffers)"""
    from siu3r_amd import _lib
    from siu3r_amd.ops import _p, _stream

    V, G = case["rect"].shape[:2]
    NB = case["geo"]["NB"]
    nch = -(-G // 2048)
    b = dict(keys=_Guarded((V, G)), ids=_Guarded((V, G)), rect=_Guarded((V, G, 4)), hist=_Guarded((V, min(NB, R.NB_MAX), nch)),
             tot=_Guarded((V, min(NB, R.NB_MAX))), bin_start=_Guarded((V, min(NB, R.NB_MAX) + 1)), entries=_Guarded((V, cap_e, 2)),
             stats=_stats([len(i) for i in case["sorted_ids"]]))
    _up(b["rect"], case["rect"])
    for v, ids in enumerate(case["sorted_ids"]):
        b["ids"].t[v, :len(ids)] = torch.from_numpy(ids).cuda()  # behind n: the sentinel (never read: a negative id would index out of the rects)
    rc = _lib.lib().siu3r_raster_bin(_cams(case["W"], case["H"], V), V, G, _p(b["keys"].t), _p(b["ids"].t), _p(b["rect"].t), _p(b["hist"].t),
                                     _p(b["tot"].t), _p(b["bin_start"].t), _p(b["entries"].t), cap_e, _p(b["stats"].t), _stream())
    torch.cuda.synchronize()
    return rc, b


def _check_bin(case, cap_e=None):
    from siu3r_amd import _lib

    V, G = case["rect"].shape[:2]
    _geometry(case, G)
    E = [len(ent) for _, ent in case["bins"]]
    overflow = cap_e is not None
    cap_e = cap_e if overflow else max(E) + 37
    rc, b = _run_bin(case, cap_e)
    _lib.check(rc)
    stats = _np(b["stats"].t)
    for v, (want_start, want_ent) in enumerate(case["bins"]):
        n = len(case["sorted_ids"][v])
        assert np.array_equal(_np(b["bin_start"].t[v]), want_start), f"view {v}: bin_start differs (the true, unclamped starts)"
        m = min(E[v], cap_e)
        assert np.array_equal(_np(b["entries"].t[v, :m]), want_ent[:m]), f"view {v}: entries differ (E = {E[v]}, cap_e = {cap_e})"
        assert stats[v].tolist() == [n, 0, E[v], 1 if E[v] > cap_e else 0], f"view {v}: stats {stats[v].tolist()}"
    for name in ("hist", "tot", "bin_start", "entries", "stats"):
        assert b[name].guards_intact(), f"{name}: written outside the buffer"
    assert b["keys"].untouched(), "the binning does not write the keys"
    assert bool((b["ids"].whole[:PAD] == SENT).all()) and bool((b["ids"].whole[-PAD:] == SENT).all())
    return E


@pytest.mark.parametrize("name", _BIN_CASES)
def test_bin(name):
    """bin_start, entries [0, E), stats[v] = {n, 0, E, 0} against bin_ref.  The counting sort's chunk boundaries (2048 Gaussians) and its
    65-column scan (n131073), ragged bins, a full bit-matrix row, rects on bin borders, NB = 1024, bins of 8 and 16 tiles"""
    case = _case(name)
    E = _check_bin(case)
    if name == "n131073":
        assert -(-(131073 + 50) // 2048) == 65 and max(E) < 600000
    if name in ("cb8", "cb16"):
        cb = case["geo"]["cb"]
        assert cb == (8 if name == "cb8" else 16)
        pr = case["bins"][0][1][:, 1]
        assert (((pr >> 10) & 31) == cb).any() and (((pr >> 15) & 31) == cb).any(), "no clipped field reaches cb"
    if name == "nb1024":
        assert case["geo"]["NB"] == 1024 and np.diff(case["bins"][0][0])[1020:].min() >= 4


def test_bin_entry_overflow():
    """cap_e = E / 2: the first cap_e entries as without a cap, bin_start unclamped, stats[v][2] = E, flag bit 0, nothing behind the buffer"""
    case = _case("n2049")
    E = len(case["bins"][0][1])
    assert E > 2049
    _check_bin(case, cap_e=E // 2)


def test_bin_refuses_a_frame_beyond_the_bin_table():
    """8448 x 8448: 33 x 33 bins even at 16 tiles per bin.  The call returns an error in front of every launch: nothing is written"""
    from siu3r_amd import _lib

    geo = R.geometry_ref(8448, 8448)
    assert geo["NB"] == 1089 and geo["cb"] == 16
    rng = np.random.default_rng(5)
    rect = _rand_rects(rng, geo, 100, 1, 3)[None]
    case = dict(W=8448, H=8448, geo=geo, rect=rect, sorted_ids=[_prefix(rng, 100, 100)])
    rc, b = _run_bin(case, 4096)
    assert rc != 0
    assert "coarse-bin table" in _lib.lib().siu3r_last_error().decode()
    for name in ("hist", "tot", "bin_start", "entries", "keys"):
        assert b[name].untouched(), f"{name} written by a refused call"
    assert _np(b["stats"].t).tolist() == [[100, 0, 0, 0]] and b["stats"].guards_intact()


def _check_lists(case, cap_d=None):
    """uploads the REFERENCE bins of the case (this stage is tested on its own), runs siu3r_raster_tile_lists, checks against the lists"""
    from siu3r_amd import _lib
    from siu3r_amd.ops import _p, _stream

    V, G = case["rect"].shape[:2]
    geo = case["geo"]
    T, NB = geo["T"], geo["NB"]
    _geometry(case, G)
    E, D = [len(ent) for _, ent in case["bins"]], [len(li) for _, li in case["lists"]]
    cap_e = max(E) + 11
    overflow = cap_d is not None
    cap_d = cap_d if overflow else max(D) + 29
    bin_start, entries = _Guarded((V, NB + 1)), _Guarded((V, cap_e, 2))
    tcount, tstart, ids = _Guarded((V, T)), _Guarded((V, T + 2)), _Guarded((V, cap_d))
    for v, (bs, ent) in enumerate(case["bins"]):
        bin_start.t[v] = torch.from_numpy(bs.astype(np.int32)).cuda()
        entries.t[v, :E[v]] = torch.from_numpy(ent).cuda()
    stats = _Guarded((V, 4), torch.int64)
    stats.t.copy_(torch.tensor([[len(case["sorted_ids"][v]), 0, E[v], 0] for v in range(V)], dtype=torch.int64))
    inputs = bin_start.whole.clone(), entries.whole.clone()
    _lib.check(_lib.lib().siu3r_raster_tile_lists(_cams(case["W"], case["H"], V), V, _p(bin_start.t), _p(entries.t), cap_e, _p(tcount.t),
                                                  _p(tstart.t), _p(ids.t), cap_d, _p(stats.t), _stream()))
    torch.cuda.synchronize()
    got_stats = _np(stats.t)
    for v, (want_ts, want_ids) in enumerate(case["lists"]):
        ts = _np(tstart.t[v])
        assert np.array_equal(ts[:T + 1], np.minimum(want_ts, cap_d)), f"view {v}: tile_start differs (D = {D[v]}, cap_d = {cap_d})"
        assert ts[T + 1] == D[v], f"view {v}: tile_start[T + 1] = {ts[T + 1]}, the true pair count is {D[v]}"
        m = min(D[v], cap_d)
        assert np.array_equal(_np(ids.t[v, :m]), want_ids[:m]), f"view {v}: per-tile lists differ"
        assert got_stats[v].tolist() == [len(case["sorted_ids"][v]), 0, E[v], 2 if D[v] > cap_d else 0], f"view {v}: stats {got_stats[v].tolist()}"
    for name, b in (("tile_count", tcount), ("tile_start", tstart), ("ids", ids), ("stats", stats)):
        assert b.guards_intact(), f"{name}: written outside the buffer"
    assert torch.equal(bin_start.whole, inputs[0]) and torch.equal(entries.whole, inputs[1]), "the bins are inputs"
    return D


@pytest.mark.parametrize("name", _BIN_CASES)
def test_tile_lists(name):
    """tile_start [0 .. T], [T + 1] = D and ids [0, D) against tile_lists_ref and tile_lists_direct, from the reference bins of every
    binning case: T = 17 424 and 69 696 on the cb = 8 / 16 frames and T = 1023 / 1024 / 1025 (tl_scan_kernel's 1024-wide loop and its
    carry), a bin of 700 entries walked in three slices, a view with nothing"""
    case = _case(name)
    D = _check_lists(case)
    T = case["geo"]["T"]
    if name in ("cb8", "cb16", "t1023", "t1024", "t1025"):
        assert T == {"cb8": 17424, "cb16": 69696, "t1023": 1023, "t1024": 1024, "t1025": 1025}[name]
        assert np.diff(case["lists"][0][0])[1024:].sum() > 0 or T <= 1024, "no list behind tile 1024"
    if name in ("t1023", "t1024", "t1025"):
        assert np.diff(case["lists"][0][0])[T - 1] > 0, "the last tile has no list"
    if name == "one_bin_700":
        assert len(case["bins"][0][1]) == 700 and 0 < np.diff(case["lists"][0][0])[:4].max() < 256
    if name == "two_views_one_empty":
        assert D[1] == 0 and D[0] > 0


def test_tile_lists_pair_overflow():
    """cap_d = D / 3: tile_start clamped to cap_d, [T + 1] the true total, the first cap_d pairs as without a cap, flag bit 1"""
    case = _case("n2049")
    D = len(case["lists"][0][1])
    assert D > 3 * 2049
    _check_lists(case, cap_d=D // 3)


# ---- the stages inside real calls ------------------------------------------------------------------------------------------------------
def _k2_cam(H, W, seed):
    from siu3r_amd import cuda_splatting as cs, raster

    c2w = look_at_camera(seed)
    fov = cs.get_fov(default_K()[None])
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([1.0]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(c2w)
    return raster.make_cam_k2(w2c, proj @ w2c, float(tan[0]), float(tan[1]), c2w[:3, 3].tolist(), [0.1, 0.2, 0.3], W, H, sh_degree=4, sh_band4=False)


def _k3_cam(H, W, seed, near=0.2, far=1000.0):
    from siu3r_amd import raster

    K = default_K()
    return raster.make_cam_k3(torch.linalg.inv(look_at_camera(seed)), K[0, 0] * W, K[1, 1] * H, K[0, 2] * W, K[1, 2] * H, W, H, near_plane=near, far_plane=far)


def _check_oracle_lists(st, ref, v=0):
    T1 = ref["tile_start"].shape[0]
    assert st.totals(1)[v] == ref["D"]
    assert np.array_equal(_np(st["tile_start_all"][v])[:T1], ref["tile_start"]), "tile ranges differ"
    assert np.array_equal(_np(st["ids_all"][v])[: ref["D"]], ref["ids"]), "per-tile sorted Gaussian lists differ"


_BIG = {"2112": (2112, 8, 3500, (0.003, 0.03)), "4224": (4224, 16, 3500, (0.002, 0.012))}


@pytest.mark.parametrize("family", ["k2", "k3"])
@pytest.mark.parametrize("size", ["2112", "4224"])
def test_render_with_wide_bins_against_the_oracle(size, family):
    """whole renders where make_geo picks bins of 8 and 16 tiles: radii, tiles_touched, lists (and n_touched, K2) exact, maps within the
    bounds of tests/test_raster_gpu.py"""
    from oracle import raster_oracle as RO
    from siu3r_amd import raster

    side, cb, G, scale = _BIG[size]
    assert raster.geometry(side, side, G)["cb"] == cb
    means, cov, opac, sh = random_scene(G, seed=3, scale=scale)
    means[:50, 2] = -1.0    # behind the camera
    means[50:60, 2] = 0.15  # inside the near cull
    cov6 = raster.cov6_from_cov3x3(cov)
    if family == "k2":
        cam = _k2_cam(side, side, seed=1)
        colors = sh.permute(0, 2, 1).contiguous()
        ref = RO.forward(cam, means.numpy(), cov6.numpy(), opac.numpy(), colors.numpy())
        out = raster.rasterize_k2(cam, means.cuda(), cov6.cuda(), colors.cuda(), opac.cuda())
    else:
        cam = _k3_cam(side, side, seed=2, near=0.2)
        colors = torch.rand(G, 3, generator=torch.Generator().manual_seed(9))
        ref = RO.forward(cam, means.numpy(), cov6.numpy(), opac.numpy(), colors.numpy())
        out = raster.rasterize_k3(cam, means.cuda(), cov6.cuda(), opac.cuda(), colors.cuda())
    # what the scene is for: lists far beyond 1024 tiles, Gaussians that straddle several bins, all inside the oracle's id buffer
    assert 30000 < ref["D"] < 64 * G and ref["tiles_touched"].max() > 160, (ref["D"], ref["tiles_touched"].max())
    st = out["state"]
    assert np.array_equal(_np(out["radii"]), ref["radii"]), "radii differ"
    assert np.array_equal(_np(st["tiles_touched"]), ref["tiles_touched"]), "tiles_touched differ"
    _check_oracle_lists(st, ref)
    if family == "k2":
        assert np.array_equal(_np(out["n_touched"]), ref["n_touched"]), "n_touched differs"
        maps = (("image", out["image"], ref["image"]), ("depth", out["depth"], ref["depth"]), ("opacity", out["opacity"], ref["alpha"]))
    else:
        maps = (("colors", out["colors"], ref["image"]), ("alphas", out["alphas"], ref["alpha"]))
    for name, got, want in maps:
        err = float(np.abs(_np(got) - want).max())
        print(f"[parity] {family} {side}^2 {name}: max abs err {err:.2e} (max |ref| {np.abs(want).max():.2e})")
        assert err <= (2e-6 * max(1.0, float(np.abs(want).max())) if family == "k2" else 2e-6)


@pytest.mark.parametrize("family", ["k2", "k3"])
def test_seventeen_views_in_one_call(family):
    """more than PV = 16 views: project_kernel runs a second blockIdx.y chunk with per-view totals of its own.  Every view of the
    17-view call is bit-identical to the same view rendered alone; views 0, 15 and 16 also against the oracle"""
    from oracle import raster_oracle as RO
    from siu3r_amd import raster

    H, W, G, V = 64, 80, 600, 17
    means, cov, opac, sh = random_scene(G, seed=21, depth=(0.8, 6.0))
    means[:20, 2] = -1.0
    cov6 = raster.cov6_from_cov3x3(cov)
    if family == "k2":
        cams = [_k2_cam(H, W, seed=s) for s in range(V)]
        colors = sh.permute(0, 2, 1).contiguous()
        run = lambda cs: raster.rasterize_views_k2(cs, means.cuda(), cov6.cuda(), colors.cuda(), opac.cuda())
        maps = ("image", "depth", "opacity", "n_touched")
    else:
        cams = [_k3_cam(H, W, seed=s, near=1.0, far=5.5) for s in range(V)]
        colors = torch.rand(G, 5, generator=torch.Generator().manual_seed(4))
        run = lambda cs: raster.rasterize_views_k3(cs, means.cuda(), cov6.cuda(), opac.cuda(), colors.cuda())
        maps = ("colors", "alphas")
    out = run(cams)
    st = out["state"]
    stats = st.stats()
    assert stats.shape == (V, 4) and int(stats[:, 0].min()) > 100
    for v in range(V):
        one = run([cams[v]])
        s1 = one["state"]
        assert torch.equal(out["radii"][v], one["radii"][0]), f"view {v}: radii"
        assert torch.equal(st["tiles_touched_all"][v], s1["tiles_touched_all"][0]), f"view {v}: tiles_touched"
        assert torch.equal(stats[v], s1.stats()[0]), f"view {v}: stats {stats[v].tolist()} / alone {s1.stats()[0].tolist()}"
        D = int(stats[v, 1])
        assert torch.equal(st["tile_start_all"][v], s1["tile_start_all"][0]), f"view {v}: tile_start"
        assert torch.equal(st["ids_all"][v, :D], s1["ids_all"][0, :D]), f"view {v}: lists"
        for m in maps:
            assert torch.equal(out[m][v], one[m][0]), f"view {v}: {m}"
    for v in (0, 15, 16):
        ref = RO.forward(cams[v], means.numpy(), cov6.numpy(), opac.numpy(), colors.numpy())
        assert np.array_equal(_np(out["radii"][v]), ref["radii"]) and np.array_equal(_np(st["tiles_touched_all"][v]), ref["tiles_touched"])
        _check_oracle_lists(st, ref, v)
        if family == "k2":
            assert np.array_equal(_np(out["n_touched"][v]), ref["n_touched"])
            for got, want in ((out["image"][v], ref["image"]), (out["depth"][v], ref["depth"]), (out["opacity"][v], ref["alpha"])):
                assert float(np.abs(_np(got) - want).max()) <= 2e-6 * max(1.0, float(np.abs(want).max()))
        else:
            assert float(np.abs(_np(out["colors"][v]) - ref["image"]).max()) <= 2e-6 and float(np.abs(_np(out["alphas"][v]) - ref["alpha"]).max()) <= 2e-6


def test_state_of_a_real_call_obeys_the_stage_references():
    """what projection really emits, through the same references as the crafted inputs: per view, sorted_ids is the stable order of the
    visible Gaussians by depth key, the entries are bin_ref of the state's own sorted_ids and rects, the lists are tile_lists_ref"""
    from siu3r_amd import raster

    H, W, G = 152, 200, 9000
    means, cov, opac, _ = random_scene(G, seed=15, depth=(0.5, 9.0), scale=(0.01, 0.12))
    cams = [_k3_cam(H, W, seed=s, near=1.0, far=8.0) for s in (2, 4, 6)]
    st = raster._project_sort_bin(cams, means.cuda(), raster.cov6_from_cov3x3(cov).cuda(), opac.cuda(), None, 0)
    geo = R.geometry_ref(W, H)
    stats = st.stats()
    rect, touched, depth = _np(st["rect"]), _np(st["tiles_touched_all"]), _np(st["rec"][:, :, 2].contiguous())
    keys = np.where(touched > 0, depth.view(np.uint32), np.uint32(R.CULLED)).astype(np.uint32)  # the key of a visible Gaussian: its depth's bits
    for v, (want_k, want_i, n) in enumerate(R.sort_ref(keys)):
        assert 1000 < n < G and int(stats[v, 0]) == n and int(stats[v, 1]) == int(touched[v].sum())
        sorted_ids = _np(st["sorted_ids"][v, :n])
        assert np.array_equal(sorted_ids, want_i), f"view {v}: sorted_ids"
        assert np.array_equal(_np(st["keys"][v, :n]).view(np.uint32), want_k), f"view {v}: sorted keys"
        bin_start, entries = R.bin_ref(geo, sorted_ids, rect[v])
        assert int(stats[v, 2]) == len(entries) and int(stats[v, 3]) == 0
        assert np.array_equal(_np(st["bin_start"][v]), bin_start), f"view {v}: bin_start"
        assert np.array_equal(_np(st["entries"][v, :len(entries)]), entries), f"view {v}: entries"
        tile_start, ids = R.tile_lists_ref(geo, bin_start, entries)
        ts2, ids2 = R.tile_lists_direct(geo, sorted_ids, rect[v])
        assert np.array_equal(tile_start, ts2) and np.array_equal(ids, ids2)
        assert np.array_equal(_np(st["tile_start_all"][v])[:geo["T"] + 1], tile_start) and int(st["tile_start_all"][v, geo["T"] + 1]) == len(ids)
        assert np.array_equal(_np(st["ids_all"][v, :len(ids)]), ids), f"view {v}: lists"
        assert len(ids) == int(stats[v, 1])
