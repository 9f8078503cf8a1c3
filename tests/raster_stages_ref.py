"""Plain numpy restatement of the rasterizer's three integer stages (csrc/raster.hip: siu3r_raster_sort, siu3r_raster_bin,
siu3r_raster_tile_lists), written from their contracts (include/siu3r_hip.h), not from the kernels.  Everything is integer-exact: a
comparison against these is `array_equal`, never a tolerance.  No GPU, no torch.

  sort_ref        keys [V,G] -> per view the visible keys in stable ascending order with their indices
  geometry_ref    frame size -> tile grid, coarse-bin edge cb and bin grid (make_geo, csrc/raster_shared.h)
  bin_ref         depth-ordered ids + tile rects -> bin_start [NB+1], entries [E,2] = (id, rect clipped to the bin, 4 x 5 bits)
  tile_lists_ref  bins -> tile_start [T+1], ids [D]: every tile's Gaussians, front to back
  tile_lists_direct  the same lists WITHOUT the bins: per tile, the sorted Gaussians whose rect contains it (the second route)
"""
import numpy as np

TILE = 16
NB_MAX = 1024          # coarse bins per view the binning accepts
CULLED = 0xFFFFFFFF    # the key of a Gaussian that takes no part in a view


def sort_ref(keys):
    """keys uint32 [V,G] -> [(sorted_keys[:n], ids[:n], n)] per view: the keys != CULLED, ascending, ties in index order"""
    keys = np.asarray(keys)
    assert keys.dtype == np.uint32 and keys.ndim == 2
    out = []
    for k in keys:
        vis = np.flatnonzero(k != np.uint32(CULLED))
        order = np.argsort(k[vis], kind="stable")
        ids = vis[order].astype(np.int32)
        out.append((k[ids], ids, int(ids.size)))
    return out


def geometry_ref(width, height):
    """tiles of 16 x 16 px; bins of cb x cb tiles with cb = 4, doubled (at most to 16) while the frame has more than NB_MAX bins.
    A frame that still has more at cb = 16 keeps cb = 16 and NB > NB_MAX: the binning refuses it."""
    gw, gh = -(-width // TILE), -(-height // TILE)
    cb = 4
    while True:
        nbx, nby = -(-gw // cb), -(-gh // cb)
        if nbx * nby <= NB_MAX or cb >= 16:
            break
        cb *= 2
    return dict(gw=gw, gh=gh, T=gw * gh, cb=cb, nbx=nbx, nby=nby, NB=nbx * nby)


def _expand(x0, y0, x1, y1):
    """boxes [x0, x1) x [y0, y1) (int arrays, all non-empty) -> for every cell of every box, in box order and row-major inside a box:
    (index of the box, x, y)"""
    w, h = x1 - x0, y1 - y0
    assert (w > 0).all() and (h > 0).all(), "empty box"
    cnt = w * h
    src = np.repeat(np.arange(cnt.size), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ws = w[src]
    return src, x0[src] + k % ws, y0[src] + k // ws


def _starts(keys, nkeys):
    """exclusive prefix of the histogram of `keys` over [0, nkeys) -> [nkeys + 1]"""
    return np.concatenate(([0], np.cumsum(np.bincount(keys, minlength=nkeys)))).astype(np.int64)


def bin_ref(geo, sorted_ids, rect):
    """sorted_ids [n]: one view's visible Gaussians front to back; rect [G,4] = (tx0, ty0, tx1, ty1) in tiles, half-open, non-empty for
    every listed id.  Walks the Gaussians in order, each over the bins of its coarse range in (cy, cx) order, and files an entry
    (id, x0 | y0 << 5 | x1 << 10 | y1 << 15) with the rect clipped to the bin and relative to it.  -> bin_start int64 [NB+1],
    entries int32 [E,2], bins ascending, depth order inside a bin"""
    cb, nbx, NB = geo["cb"], geo["nbx"], geo["NB"]
    ids = np.asarray(sorted_ids, np.int64)
    r = np.asarray(rect, np.int64)[ids]
    if ids.size == 0:
        return np.zeros(NB + 1, np.int64), np.zeros((0, 2), np.int32)
    src, cx, cy = _expand(r[:, 0] // cb, r[:, 1] // cb, (r[:, 2] - 1) // cb + 1, (r[:, 3] - 1) // cb + 1)
    ox, oy, rr = cx * cb, cy * cb, r[src]
    x0, y0 = np.maximum(rr[:, 0], ox) - ox, np.maximum(rr[:, 1], oy) - oy
    x1, y1 = np.minimum(rr[:, 2], ox + cb) - ox, np.minimum(rr[:, 3], oy + cb) - oy
    assert (x0 < x1).all() and (y0 < y1).all() and x1.max() <= cb and y1.max() <= cb
    b = cy * nbx + cx
    assert b.min() >= 0 and b.max() < NB
    order = np.argsort(b, kind="stable")  # (a Gaussian meets a bin once: inside a bin the walk's order is the depth order)
    ent = np.stack((ids[src], x0 | (y0 << 5) | (x1 << 10) | (y1 << 15)), -1)[order].astype(np.int32)
    return _starts(b, NB), ent


def tile_lists_ref(geo, bin_start, entries):
    """the bins of bin_ref -> tile_start int64 [T+1], ids int32 [D]: tile t = ty * gw + tx lists the entries of its bin whose clipped
    rect covers it, in the bin's order"""
    cb, nbx, gw, T = geo["cb"], geo["nbx"], geo["gw"], geo["T"]
    ent = np.asarray(entries, np.int64)
    if ent.shape[0] == 0:
        return np.zeros(T + 1, np.int64), np.zeros(0, np.int32)
    b = np.repeat(np.arange(geo["NB"]), np.diff(np.asarray(bin_start, np.int64)))
    pr = ent[:, 1]
    ox, oy = (b % nbx) * cb, (b // nbx) * cb
    src, tx, ty = _expand(ox + (pr & 31), oy + ((pr >> 5) & 31), ox + ((pr >> 10) & 31), oy + ((pr >> 15) & 31))
    assert tx.max() < gw and ty.max() < geo["gh"]
    t = ty * gw + tx
    order = np.argsort(t, kind="stable")  # (a tile lies in one bin, and the bins hold their entries front to back)
    return _starts(t, T), ent[src, 0][order].astype(np.int32)


def tile_lists_direct(geo, sorted_ids, rect):
    """the second route to the lists, without bins, clipping or packing: tile t lists the Gaussians of sorted_ids, in that order,
    whose rect contains it"""
    gw, T = geo["gw"], geo["T"]
    ids = np.asarray(sorted_ids, np.int64)
    if ids.size == 0:
        return np.zeros(T + 1, np.int64), np.zeros(0, np.int32)
    r = np.asarray(rect, np.int64)[ids]
    src, tx, ty = _expand(r[:, 0], r[:, 1], r[:, 2], r[:, 3])
    t = ty * gw + tx
    order = np.argsort(t, kind="stable")
    return _starts(t, T), ids[src][order].astype(np.int32)
