"""tests/raster_stages_ref.py (the numpy references the GPU stage tests compare against) checked against brute-force Python loops at
tiny sizes, and geometry_ref against values worked out by hand from make_geo (csrc/raster_shared.h).  No GPU."""
import numpy as np
import pytest

import raster_stages_ref as R


# ---- brute force: loops only, no sorting routine of numpy's ------------------------------------------------------------------------
def _sort_loops(keys):
    """insertion sort of (key, index) over the visible keys of one view: stable by construction"""
    out = []
    for i, k in enumerate(int(x) for x in keys):
        if k == R.CULLED:
            continue
        j = len(out)
        while j > 0 and out[j - 1][0] > k:
            j -= 1
        out.insert(j, (k, i))
    return [k for k, _ in out], [i for _, i in out]


def _bins_loops(geo, sorted_ids, rect):
    cb, nbx, NB = geo["cb"], geo["nbx"], geo["NB"]
    bins = [[] for _ in range(NB)]
    for g in (int(x) for x in sorted_ids):
        x0, y0, x1, y1 = (int(x) for x in rect[g])
        for by in range(geo["nby"]):
            for bx in range(nbx):
                ox, oy = bx * cb, by * cb
                # the part of the rect inside this bin, relative to the bin's first tile
                cx0, cy0, cx1, cy1 = max(x0, ox), max(y0, oy), min(x1, ox + cb), min(y1, oy + cb)
                if cx0 < cx1 and cy0 < cy1:
                    bins[by * nbx + bx].append((g, (cx0 - ox) | ((cy0 - oy) << 5) | ((cx1 - ox) << 10) | ((cy1 - oy) << 15)))
    start, ent = [0], []
    for b in bins:
        ent += b
        start.append(len(ent))
    return start, ent


def _lists_loops(geo, sorted_ids, rect):
    start, ids = [0], []
    for ty in range(geo["gh"]):
        for tx in range(geo["gw"]):
            for g in (int(x) for x in sorted_ids):
                x0, y0, x1, y1 = (int(x) for x in rect[g])
                if x0 <= tx < x1 and y0 <= ty < y1:
                    ids.append(g)
            start.append(len(ids))
    return start, ids


def _rects(rng, geo, G, max_side):
    w, h = rng.integers(1, max_side + 1, G), rng.integers(1, max_side + 1, G)
    w, h = np.minimum(w, geo["gw"]), np.minimum(h, geo["gh"])
    x0, y0 = rng.integers(0, geo["gw"] - w + 1), rng.integers(0, geo["gh"] - h + 1)
    return np.stack((x0, y0, x0 + w, y0 + h), -1).astype(np.int32)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side, cb, NB", [(2048, 4, 1024), (2112, 8, 289), (4224, 16, 289), (8448, 16, 1089)])
def test_geometry_ref_square_frames(side, cb, NB):
    """2048 px = 128 tiles = 32 bins of 4 per axis (1024, the table's size exactly); 2112 px = 132 tiles: 33^2 = 1089 bins of 4 are too
    many, 17^2 = 289 of 8 fit; 4224 px = 264 tiles: 66^2, 33^2 too many, 17^2 of 16 fit; 8448 px = 528 tiles: 33^2 = 1089 even at 16,
    where the doubling stops (the binning refuses the frame)"""
    g = R.geometry_ref(side, side)
    assert (g["cb"], g["NB"]) == (cb, NB)
    assert g["gw"] == g["gh"] == side // 16 and g["T"] == (side // 16) ** 2 and g["nbx"] == g["nby"] == -(-(side // 16) // cb)
    assert (g["NB"] > R.NB_MAX) == (side == 8448)


def test_geometry_ref_ragged_frames():
    assert R.geometry_ref(208, 160) == dict(gw=13, gh=10, T=130, cb=4, nbx=4, nby=3, NB=12)
    assert R.geometry_ref(250, 190) == dict(gw=16, gh=12, T=192, cb=4, nbx=4, nby=3, NB=12)  # partial tiles count
    assert R.geometry_ref(1, 1) == dict(gw=1, gh=1, T=1, cb=4, nbx=1, nby=1, NB=1)
    assert R.geometry_ref(16400, 16)["T"] == 1025 and R.geometry_ref(16400, 16)["cb"] == 4
    assert R.geometry_ref(3840, 2160)["cb"] == 8  # 240 x 135 tiles: 60 x 34 = 2040 bins of 4, 30 x 17 = 510 of 8


# ---- sort --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "few_values", "all_equal", "all_culled", "one_visible", "extremes"])
def test_sort_ref_against_insertion_sort(case):
    rng = np.random.default_rng(7)
    G = 300
    keys = rng.integers(0, 2 ** 32, (2, G), dtype=np.uint64).astype(np.uint32)
    keys[rng.random((2, G)) < 0.4] = R.CULLED
    if case == "few_values":
        keys = rng.integers(0, 5, (2, G)).astype(np.uint32) * np.uint32(0x01010101)
        keys[1, ::3] = R.CULLED
    elif case == "all_equal":
        keys[:] = 77
    elif case == "all_culled":
        keys[:] = R.CULLED
    elif case == "one_visible":
        keys[:] = R.CULLED
        keys[0, 123] = 5
        keys[1, 299] = 0
    elif case == "extremes":
        keys[0, :8] = [0xFFFFFFFE, 0x80000000, 0x7F7FFFFF, 0, 0xFFFFFFFE, 0x80000000, 0x7F7FFFFF, 0]
    for v, (sk, ids, n) in enumerate(R.sort_ref(keys)):
        want_k, want_i = _sort_loops(keys[v])
        assert n == len(want_k) == sk.size == ids.size
        assert sk.tolist() == want_k and ids.tolist() == want_i
        assert sk.dtype == np.uint32 and ids.dtype == np.int32


# ---- bins and lists ------------------------------------------------------------------------------------------------------------------
_FRAMES = [(208, 160), (64, 64), (80, 48), (16, 16), (2112 // 8, 2112 // 8)]


def _forced_geo(geo, cb):
    """the same tile grid with a larger bin edge (what make_geo picks for big frames), so that cb = 8 / 16 run at a brute-force size"""
    g = dict(geo, cb=cb)
    g["nbx"], g["nby"] = -(-g["gw"] // cb), -(-g["gh"] // cb)
    g["NB"] = g["nbx"] * g["nby"]
    return g


@pytest.mark.parametrize("cb", [4, 8, 16])
@pytest.mark.parametrize("frame", _FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_bin_and_list_refs_against_loops(frame, cb):
    rng = np.random.default_rng(frame[0] * 31 + cb)
    geo = _forced_geo(R.geometry_ref(*frame), cb)
    G = 120
    rect = _rects(rng, geo, G, max_side=2 * cb + 1)
    rect[0] = (0, 0, geo["gw"], geo["gh"])                         # the whole frame
    rect[1] = (0, 0, min(cb, geo["gw"]), min(cb, geo["gh"]))       # exactly the first bin: clipped x1 / y1 reach cb
    rect[2] = (geo["gw"] - 1, geo["gh"] - 1, geo["gw"], geo["gh"])   # the last tile
    sorted_ids = rng.permutation(G)[:97].astype(np.int32)          # a prefix of a permutation: some Gaussians take no part
    bin_start, entries = R.bin_ref(geo, sorted_ids, rect)
    want_start, want_ent = _bins_loops(geo, sorted_ids, rect)
    assert bin_start.tolist() == want_start
    assert [tuple(e) for e in entries.tolist()] == want_ent
    tile_start, ids = R.tile_lists_ref(geo, bin_start, entries)
    want_ts, want_ids = _lists_loops(geo, sorted_ids, rect)
    assert tile_start.tolist() == want_ts and ids.tolist() == want_ids
    ts2, ids2 = R.tile_lists_direct(geo, sorted_ids, rect)
    assert ts2.tolist() == want_ts and ids2.tolist() == want_ids


def test_refs_with_nothing_visible():
    geo = R.geometry_ref(208, 160)
    rect = np.zeros((5, 4), np.int32)
    none = np.zeros(0, np.int32)
    bin_start, entries = R.bin_ref(geo, none, rect)
    assert bin_start.tolist() == [0] * 13 and entries.shape == (0, 2)
    for ts, ids in (R.tile_lists_ref(geo, bin_start, entries), R.tile_lists_direct(geo, none, rect)):
        assert ts.tolist() == [0] * 131 and ids.size == 0


def test_the_two_list_routes_agree_at_a_larger_size():
    """beyond brute force: 5000 Gaussians on a cb = 8 frame, bins against no bins"""
    rng = np.random.default_rng(3)
    geo = R.geometry_ref(2112, 2112)
    rect = _rects(rng, geo, 5000, max_side=30)
    sorted_ids = rng.permutation(5000)[:4000].astype(np.int32)
    bin_start, entries = R.bin_ref(geo, sorted_ids, rect)
    a, b = R.tile_lists_ref(geo, bin_start, entries), R.tile_lists_direct(geo, sorted_ids, rect)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].size > 500000
