"""Gaussian splat rasterizer front-end: torch tensors -> the C ABI of csrc/raster.hip.

Two conventions behind one tile-binned HIP renderer (include/siu3r_hip.h, siu3r_raster_cam):
  K2 = diff-gaussian-rasterization-w-pose semantics (reference call site src/models/cuda_splatting.py:90-118)
  K3 = gsplat.rasterization semantics (reference call site src/models/gaussian_renderer.py:92-106)
All V views of a call travel through every launch together (the reference loops over views in Python,
cuda_splatting.py:82-121): project -> one stable depth radix sort per view -> depth-ordered coarse bins -> composite.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from ._lib import RasterCam, check
from .ops import _gpu, _p, _stream

TILE = 16
GR_N = 10  # floats per (view, Gaussian) screen-space gradient record (csrc/raster_bwd_shared.h)


def _set(arr, values):
    for i, v in enumerate(values):
        arr[i] = float(v)


def make_cam_k2(w2c, full_proj, tanfovx, tanfovy, campos, bg, width, height, sh_degree=4, sh_band4=False, nt_post_blend=True, near=None,
                far=None) -> RasterCam:
    """sh_degree -1: the colours handed to the rasterizer are precomputed [G,1,3] values, blended as given (no SH, no clamp).
    w2c / full_proj / tanfov / campos None + (near, far): the pose comes from device tensors (`pose_c2w` of the rasterize_* calls,
    siu3r_raster_project_c2w) and only the projection planes travel in the block."""
    c = RasterCam()
    c.mode, c.width, c.height = 0, int(width), int(height)
    if w2c is not None:
        _set(c.w2c, w2c.reshape(-1).tolist())
        _set(c.proj, full_proj.reshape(-1).tolist())
        c.tanfovx, c.tanfovy = float(tanfovx), float(tanfovy)
        _set(c.campos, campos)
    if near is not None:
        c.k2_near, c.k2_far = float(near), float(far)
    _set(c.bg, bg)
    c.sh_degree, c.sh_band4, c.k2_znear_cull = int(sh_degree), int(bool(sh_band4)), 0.2
    c.alpha_min, c.alpha_max, c.t_min, c.dilation = 1.0 / 255.0, 0.99, 1e-4, 0.3
    c.eps2d, c.extent_sigma = 0.3, 3.33
    c.near_plane = 0.2
    c.nt_post_blend = int(bool(nt_post_blend))
    return c


def make_cam_k3(w2c, fx, fy, cx, cy, width, height, near_plane=0.01, far_plane=1e10, eps2d=0.3, radius_clip=0.0,
                opacity_aware_extent=False) -> RasterCam:
    c = RasterCam()
    c.mode, c.width, c.height = 1, int(width), int(height)
    _set(c.w2c, w2c.reshape(-1).tolist())
    c.fx, c.fy, c.cx, c.cy = float(fx), float(fy), float(cx), float(cy)
    c.near_plane, c.far_plane, c.eps2d, c.radius_clip = float(near_plane), float(far_plane), float(eps2d), float(radius_clip)
    c.extent_sigma, c.opacity_aware_extent = 3.33, int(bool(opacity_aware_extent))
    c.alpha_min, c.alpha_max, c.t_min, c.dilation = 1.0 / 255.0, 0.999, 1e-4, 0.3
    c.k2_znear_cull = 0.2
    c.nt_post_blend = 1
    return c


def cov6_from_cov3x3(cov: torch.Tensor) -> torch.Tensor:
    """[G,3,3] -> [G,6] upper-triangular (xx,xy,xz,yy,yz,zz), the order of torch.triu_indices(3,3)
    (reference cuda_splatting.py:107,115).  Pure indexing (layout plumbing)."""
    return torch.stack((cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]), dim=-1).contiguous()


def geometry(width: int, height: int, G: int) -> Dict[str, int]:
    out = (C.c_int32 * 8)()
    check(_lib.lib().siu3r_raster_geometry(int(width), int(height), int(G), out))
    return dict(gw=out[0], gh=out[1], T=out[2], cb=out[3], NB=out[4], nchunks_sort=out[5], nchunks_bin=out[6], cam_bytes=out[7])


def default_entry_capacity(G: int) -> int:
    """Coarse-bin entries per view (8 B each): a Gaussian lands in one 64 x 64 px bin unless it straddles a bin border;
    3 per Gaussian covers the 2 M-Gaussian 1080p stress scene (large splats) with margin.  An overflow is detected after
    the frame (stats) and the call is repeated with the exact count."""
    return int(min(max(3 * G + 65536, 1 << 18), (1 << 31) - 1024))


def default_pair_capacity(G: int) -> int:
    """(tile, Gaussian) pairs per view for the materialised tile lists (4 B each): 8 per Gaussian, at least 1 M."""
    return int(min(max(8 * G, 1 << 20), (1 << 31) - 1024))


# Capacities that a scene of a given size needed before: a caller that renders many frames of similar scenes (an evaluation loop) pays
# the detect-and-repeat of an overflowing bound once, not on every call.  key: (kind, G, V, width, height) -> capacity
_CAPACITY_HINTS: Dict[tuple, int] = {}


def _hinted(kind: str, G: int, V: int, W: int, H: int, default: int) -> int:
    return max(default, _CAPACITY_HINTS.get((kind, G, V, W, H), 0))


def _remember(kind: str, G: int, V: int, W: int, H: int, needed: int):
    _CAPACITY_HINTS[(kind, G, V, W, H)] = int(min(needed + needed // 4 + 1024, (1 << 31) - 1024))


class RasterOverflow(RuntimeError):
    """call_id: sequence number of the deferred call whose views overflowed (None for the synchronous paths)"""

    def __init__(self, msg, call_id=None):
        super().__init__(msg)
        self.call_id = call_id


class RasterState:
    """Buffers of one rasterizer call (V views); __slots__ is everything a call's state can hold (None until set).  The per-tile Gaussian
    lists are not needed to render an RGB view: the properties tile_start_all / ids_all / cap_d (tile_start / ids: view 0) build them on
    first use.  Gv / D / E read the device-side totals of view 0.  state["name"] reads the attribute `name`; nothing is written that way."""
    __slots__ = ("V", "G", "W", "H", "T", "geo", "cams", "cams_dev",  # sizes, geometry(W, H, G), the host RasterCam array and its device blocks
                 "rec", "radii", "rect", "tiles_touched_all", "keys", "keys_b", "sorted_ids", "ids_b",  # per (view, Gaussian)
                 "stats_dev", "bin_start", "entries", "cap_e",  # [V,4] i64 device counters (stats(): their host copy), the coarse bins
                 "pose_dev",  # the two device pose tensors of a "dp" / "c2w" call: like feat_ws kept here because launches read them asynchronously
                 "defer", "cap_d_hint",  # the caller checks for overflow later: nothing synchronises; pair capacity the lists start from
                 "feat_ws", "feat_ws_lists",  # workspace of the N-channel matrix-core composite, and whether it holds the per-quadrant lists
                 "antialiased",  # the projection was the anti-aliased one (siu3r_raster_project_aa): a backward must differentiate that record
                 "_stats_host", "_tl")  # _tl: (tile_start_all [V,T+2], ids_all [V,cap_d], cap_d) once _lists() ran

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.pop(k, None))
        assert not fields, f"not a field of RasterState: {sorted(fields)}"

    def __getitem__(self, k):  # read-only (there is no __setitem__), and only the public fields and properties: _KEYS below
        if k not in self._KEYS:
            raise KeyError(k)
        return getattr(self, k)

    def stats(self) -> torch.Tensor:
        if self._stats_host is None:
            self._stats_host = self.stats_dev.cpu()
        return self._stats_host

    def totals(self, k: int) -> List[int]:
        return [int(x) for x in self.stats()[:, k].tolist()]

    def verify(self):
        """Raise when a capacity-bounded buffer overflowed (only needed by callers that passed check=False)."""
        e_max = int(self.stats()[:, 2].max())
        if e_max > self.cap_e:
            raise RasterOverflow(f"rasterizer coarse-bin entries overflowed: E = {e_max} > entry_capacity {self.cap_e} (pass entry_capacity >= {e_max})")
        # the materialised (tile, Gaussian) pair lists of the N-channel path (tl_scan sets flag bit 1 when a view's pairs exceed
        # pair_capacity: far splats would silently be missing from tiles).  Deferred callers (check_overflow=False) must call verify().
        if self._tl is not None:  # (only when they were built: verify() never builds them)
            tstart, _, cap_d = self._tl
            d_max = int(tstart[:, self.T + 1].max())
            if d_max > cap_d:  # (the sticky flag bit of an earlier, repeated attempt is not consulted: the scan's own total is)
                raise RasterOverflow(f"rasterizer tile-pair lists overflowed: D = {d_max} > pair_capacity {cap_d} (pass pair_capacity >= {d_max})")

    def _lists(self) -> tuple:
        if self._tl is None:
            V, T, dev = self.V, self.T, self.stats_dev.device
            hint_key = ("pairs", self.G, V, self.W, self.H)
            cap_d = self.cap_d_hint or max(1, max(self.totals(1)))
            cap_d = max(cap_d, _CAPACITY_HINTS.get(hint_key, 0))
            while True:
                tcount = torch.empty((V, T), dtype=torch.int32, device=dev)
                tstart = torch.empty((V, T + 2), dtype=torch.int32, device=dev)
                ids = torch.empty((V, cap_d), dtype=torch.int32, device=dev)
                check(_lib.lib().siu3r_raster_tile_lists(self.cams, V, _p(self.bin_start), _p(self.entries), self.cap_e, _p(tcount), _p(tstart), _p(ids),
                                                         cap_d, _p(self.stats_dev), _stream()))
                if self.defer:
                    break
                d_max = int(tstart[:, T + 1].max())
                if d_max <= cap_d:
                    break
                cap_d = d_max  # the bound was too small: repeat with the exact pair count
                _remember(*hint_key, d_max)
            self._tl = (tstart, ids, cap_d)
        return self._tl

    tile_start_all = property(lambda self: self._lists()[0])
    ids_all = property(lambda self: self._lists()[1])
    cap_d = property(lambda self: self._lists()[2])
    tile_start = property(lambda self: self._lists()[0][0])
    ids = property(lambda self: self._lists()[1][0])
    tiles_touched = property(lambda self: self.tiles_touched_all[0])
    Gv = property(lambda self: self.totals(0)[0])
    D = property(lambda self: self.totals(1)[0])
    E = property(lambda self: self.totals(2)[0])
    _KEYS = frozenset(__slots__[:-2] + ("tile_start_all", "ids_all", "cap_d", "tile_start", "ids", "tiles_touched", "Gv", "D", "E"))


def _cam_array(cams: Sequence[RasterCam]):
    arr = (RasterCam * len(cams))()
    for i, c in enumerate(cams):
        C.memmove(C.byref(arr, i * C.sizeof(RasterCam)), C.byref(c), C.sizeof(RasterCam))
    return arr


def _cov_stride(cov: torch.Tensor) -> int:
    """[G,6] upper-triangular or [G,3,3] full covariances (read in place by the projection kernel)."""
    if cov.dim() == 2 and cov.shape[1] == 6:
        return 6
    if cov.dim() == 3 and cov.shape[1:] == (3, 3):
        return 9
    raise RuntimeError(f"covariances must be [G,6] or [G,3,3], got {tuple(cov.shape)}")


def _pose_dev(pose_dev, V, dev):
    """(viewmats [V,4,4], Ks [V,3,3]) device tensors -> contiguous fp32 on `dev` (layout plumbing only; nothing is read back)"""
    vm, Ks = pose_dev
    vm = vm.detach().to(device=dev, dtype=torch.float32).contiguous()
    Ks = Ks.detach().to(device=dev, dtype=torch.float32).contiguous()
    if tuple(vm.shape) != (V, 4, 4) or tuple(Ks.shape) != (V, 3, 3):
        raise RuntimeError(f"device-side poses must be viewmats [V,4,4] and Ks [V,3,3] with V = {V}, got {tuple(vm.shape)} / {tuple(Ks.shape)}")
    return vm, Ks


_Pose = collections.namedtuple("_Pose", "kind a b t_scale")
_HOST_POSE = _Pose("host", None, None, 1.0)


def _pose(V, dev, pose_dev=None, pose_c2w=None) -> _Pose:
    """Where the projection takes a call's pose from, made once at the entry point.  Neither keyword: kind "host", the camera blocks carry it.
    pose_dev = (viewmats [V,4,4] world->camera, Ks [V,3,3] pixel units) as DEVICE tensors (gsplat family): kind "dp", the kernels take the pose
    from a, b (siu3r_raster_project_dp), `cams` only carries frame size, planes and thresholds.  pose_c2w = (extrinsics [V,4,4] camera-to-world,
    normalised intrinsics [V,3,3], t_scale): DEVICE tensors + a float, either family, kind "c2w" (SplattingCUDA.forward; siu3r_raster_project_c2w)."""
    if pose_c2w is not None:
        return _Pose("c2w", *_pose_dev(pose_c2w[:2], V, dev), float(pose_c2w[2]))
    if pose_dev is not None:
        return _Pose("dp", *_pose_dev(pose_dev, V, dev), 1.0)
    return _HOST_POSE


def _project_sort_bin(cams: Sequence[RasterCam], means, cov, opac, colors, channels, entry_capacity=None, check_overflow=True,
                      sh_planar=False, pose: _Pose = _HOST_POSE, antialiased=False) -> RasterState:
    V, G, dev = len(cams), means.shape[0], means.device
    if antialiased and (pose.kind == "dp" or any(c.mode != 0 for c in cams)):
        raise ValueError("antialiased=True covers the 3DGS family (K2 cameras); the gsplat-family (K3) path has no anti-aliased mode")
    arr = _cam_array(cams)
    W, H = cams[0].width, cams[0].height
    geo = geometry(W, H, G)
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    cap_e = int(entry_capacity) if entry_capacity else _hinted("entries", G, V, W, H, default_entry_capacity(G))
    st = RasterState(V=V, G=G, W=W, H=H, T=geo["T"], geo=geo, cams=arr, cams_dev=torch.empty((V * geo["cam_bytes"],), dtype=torch.uint8, device=dev),
                     rec=f(V, G, 12), radii=i32(V, G, 2), rect=i32(V, G, 4), tiles_touched_all=i32(V, G), keys=i32(V, G), keys_b=i32(V, G), sorted_ids=i32(V, G),
                     ids_b=i32(V, G), stats_dev=torch.empty((V, 4), dtype=torch.int64, device=dev), defer=not check_overflow, cap_e=cap_e)
    lib = _lib.lib()
    head = (arr, V, _p(st.cams_dev))
    tail = (G, _p(means), _p(cov), _cov_stride(cov), _p(opac), _p(colors), channels, int(bool(sh_planar)), _p(st.rec), _p(st.radii), _p(st.rect),
            _p(st.tiles_touched_all), _p(st.keys), _p(st.stats_dev), _stream())
    if antialiased:  # the same calls with the compensation in the record's opacity; the factor itself (comp) is not wanted here
        st.antialiased = True
        if pose.kind == "c2w":
            st.pose_dev = (pose.a, pose.b)
            check(lib.siu3r_raster_project_c2w_aa(*head, _p(pose.a), _p(pose.b), pose.t_scale, *tail[:-1], None, tail[-1]))
        else:
            check(lib.siu3r_raster_project_aa(*head, *tail[:-1], None, tail[-1]))
    elif pose.kind == "host":
        check(lib.siu3r_raster_project(*head, *tail))
    else:
        st.pose_dev = (pose.a, pose.b)  # (kept with the state: the launches read them asynchronously)
        if pose.kind == "c2w":
            check(lib.siu3r_raster_project_c2w(*head, _p(pose.a), _p(pose.b), pose.t_scale, *tail))
        else:
            check(lib.siu3r_raster_project_dp(*head, _p(pose.a), _p(pose.b), *tail))
    rs_hist, rs_tot = i32(V, 256, geo["nchunks_sort"]), i32(V, 256)
    check(lib.siu3r_raster_sort(V, G, _p(st.keys), _p(st.keys_b), _p(st.sorted_ids), _p(st.ids_b), _p(rs_hist), _p(rs_tot), _p(st.stats_dev), _stream()))
    bin_hist, bin_tot = i32(V, geo["NB"], geo["nchunks_bin"]), i32(V, geo["NB"])
    st.bin_start = i32(V, geo["NB"] + 1)
    st.entries = torch.empty((V, cap_e, 2), dtype=torch.int32, device=dev)
    check(lib.siu3r_raster_bin(arr, V, G, _p(st.keys), _p(st.sorted_ids), _p(st.rect), _p(bin_hist), _p(bin_tot), _p(st.bin_start), _p(st.entries), cap_e,
                               _p(st.stats_dev), _stream()))
    return st


# ---- deferred overflow checks.  check_overflow=True reads the counters right after the call: a device synchronisation per call, behind
# which the host prepares the next call while the GPU idles (25 % of a 6-view 512^2 frame).  check_overflow="deferred" enqueues an
# asynchronous copy of the counters into pinned memory instead and looks at it when the NEXT deferred call starts (by then the copy has
# long landed) or when check_pending() is called; an overflowing view cannot pass unnoticed meanwhile: the composite kernel fills it
# with NaN.  On detection the needed capacity is remembered (later calls of that scene size are sized right) and RasterOverflow names
# the call that overflowed -- its sequence number (`RasterOverflow.call_id`, returned as out["call_id"] by the deferred call) and its
# scene size -- so that the caller knows WHICH result to discard and repeat; the exception may surface at the start of a LATER deferred
# call (which has not run yet) or at check_pending().  Callers in this repository: bench.py's render legs (check_pending() after the
# timed calls); evaluate.py renders with the synchronous check (check_overflow=True: transparent repeat).
_Pending = collections.namedtuple("_Pending", "event host cap_e key call_id")  # key = (G, V, W, H) of the call
_PENDING: "collections.deque" = collections.deque()
_PINNED_FREE: list = []
_CALL_SEQ = [0]


def _defer_check(st: RasterState):
    stats = st.stats_dev
    i = next((i for i, h in enumerate(_PINNED_FREE) if h.shape == stats.shape), None)
    host = _PINNED_FREE.pop(i) if i is not None else torch.empty(stats.shape, dtype=stats.dtype, pin_memory=True)
    host.copy_(stats, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _CALL_SEQ[0] += 1
    _PENDING.append(_Pending(ev, host, st.cap_e, (st.G, st.V, st.W, st.H), _CALL_SEQ[0]))
    return _CALL_SEQ[0]


def check_pending(block: bool = True):
    """Verify the deferred calls (all of them, waiting for their counters, or with block=False only those whose counters have
    arrived).  Raises RasterOverflow for the first call that overflowed its entry buffers (its views were rendered as NaN)."""
    bad = None
    while _PENDING:
        p = _PENDING[0]
        if not block and not p.event.query():
            break
        p.event.synchronize()
        _PENDING.popleft()
        e_max = int(p.host[:, 2].max())
        if len(_PINNED_FREE) < 8:
            _PINNED_FREE.append(p.host)
        if e_max > p.cap_e:
            _remember("entries", *p.key, e_max)
            bad = bad or (e_max, p)
    if bad:
        e_max, p = bad
        raise RasterOverflow(f"deferred rasterizer call #{p.call_id} (G, V, W, H = {p.key}) overflowed its coarse-bin entries: E = {e_max} > entry_capacity "
                             f"{p.cap_e}; its views were rendered as NaN.  The needed capacity is remembered: repeat that call", call_id=p.call_id)


def _with_retry(run, entry_capacity, check_overflow):
    """run(entry_capacity) -> result dict with "state".  The coarse-bin entries are sized by a bound; when a frame overflows it (the
    kernels drop the excess, flag it and poison the view) the whole call is repeated once with the exact count: the CUDA originals
    resize their buffers behind a device-to-host copy instead.  check_overflow: True = look now (synchronises), "deferred" = look when
    the next deferred call starts / at check_pending(), False = the caller calls state.verify()."""
    if check_overflow == "deferred":
        check_pending(block=False)
        out = run(entry_capacity)
        out["call_id"] = _defer_check(out["state"])
        return out
    out = run(entry_capacity)
    if not check_overflow:
        return out
    st = out["state"]
    e_max = max(st.totals(2))
    if e_max > st.cap_e:
        _remember("entries", st.G, st.V, st.W, st.H, e_max)
        out = run(e_max)
        out["state"].verify()
    return out


def _render(cams, means, cov6, opacities, chan, channels, pose, entry_capacity, check_overflow, composite, sh_planar=False, antialiased=False):
    """The one render path (the entry points have checked the device).  chan: the call's colour block -- `channels` > 0: shs / rgb, which the
    projection reads into the records; 0: feats, which only the composite reads.  composite(st, chan): allocate outputs, launch, return the dict."""
    means, cov6, opacities, chan = (t.contiguous().float() for t in (means, cov6, opacities, chan))

    def run(cap):
        st = _project_sort_bin(cams, means, cov6, opacities, chan if channels else None, channels, cap, check_overflow, sh_planar, pose, antialiased)
        return composite(st, chan)

    return _with_retry(run, entry_capacity, check_overflow)


def _empty(st: RasterState, *shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=st.rec.device)


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _no_deferred(check_overflow):
    if check_overflow == "deferred":
        raise ValueError('check_overflow="deferred" cannot be combined with gradients: the backward reuses the binning of the forward, which '
                         "must be known complete (pass check_overflow=True)")


def _forward(ctx, render, diff, keep, maps, aux):
    """forward of the three autograd functions: render(the first four of the differentiable arguments `diff`, detached; synchronous overflow
    check).  ctx keeps the state and what _grads_out needs of `diff`; saved: `keep` (inputs the backward reads again) and private copies of the
    outputs `maps` (callers may modify the returned ones in place: image.clamp_(0, 1)); the outputs `aux` carry no gradient.  -> maps, aux, state"""
    o = render(*(t.detach() for t in diff[:4]))
    ctx.st = o["state"]
    ctx.shapes = [(t.shape, t.dtype, t.device) if isinstance(t, torch.Tensor) else None for t in diff]
    ctx.save_for_backward(*keep, *(o[k].clone() for k in maps))
    ctx.mark_non_differentiable(*(o[k] for k in aux if o[k] is not None))
    return (*(o[k] for k in maps + aux), ctx.st)


def _backward_start(ctx, inputs, upstream):
    """what the three backwards start from: the state; the saved `inputs` as the kernels read them (fp32, contiguous); the upstream gradients
    of the (output, gradient) pairs likewise, zeros where autograd hands over None; the empty screen-space gradient buffer [V,G,GR_N]"""
    st = ctx.st
    return (st, [t.detach().contiguous().float() for t in inputs],
            [torch.zeros_like(ref) if g is None else g.detach().float().contiguous() for ref, g in upstream], _empty(st, st.V, st.G, GR_N))


def _grads_out(ctx, first, grads):
    """the gradients of the differentiable inputs (index first.. of forward's arguments) in their shapes / dtypes / devices (a pose handed
    over on the host gets its gradient there), None where not needed"""
    out = []
    for i, g in enumerate(grads):
        if g is None or not ctx.needs_input_grad[first + i]:
            out.append(None)
            continue
        shape, dtype, device = ctx.shapes[i]
        out.append(g.reshape(shape).to(device=device, dtype=dtype))
    return out


def rasterize_views_k2(cams: Sequence[RasterCam], means, cov6, shs, opacities, want_n_touched=True, entry_capacity=None,
                       check_overflow=True, sh_planar=False, pose_c2w=None, pose_delta=None, means2d=None, density_stats=None,
                       antialiased=False) -> Dict[str, torch.Tensor]:
    """V views of one Gaussian set.  means [G,3]; cov6 [G,6] (upper triangle) or [G,3,3]; shs [G,ncoef,3], or with sh_planar
    [G,3,25] (Gaussians.harmonics as stored); opacities [G] (fp32, GPU) -> image [V,3,H,W], radii [V,G,2] i32, depth [V,H,W],
    opacity [V,H,W], n_touched [V,G] i32 (None when not wanted) + the call's state.

    Differentiable when grad mode is on and means / cov6 / shs / opacities / pose_delta / means2d requires grad (_RasterizeK2; the
    outputs are the same bits as without grad).  pose_delta [V,6] = (rho, theta): a left se(3) perturbation w2c <- exp(xi^) w2c of each
    view, a gradient holder taken at xi = 0 (the render uses the poses as given).  means2d [G,k>=2]: a gradient holder that receives the
    pixel-space mean gradient summed over the views (the caller scales it).  Every other call runs the plain forward.
    density_stats: a density.DensityStats of G Gaussians; the backward of a differentiable call accumulates the per-view NDC-space mean
    gradient norms (scaled by V: DensityStats.accumulate), the visibility counts and the largest radii into it.  The forward does not
    look at it, and None (the default) leaves the backward exactly as it is without the keyword.  With density_stats.absgrad the composite
    backward is siu3r_raster_composite_rgb_bwd_abs and the norms are those of its abs_mean2d (AbsGS); every returned gradient, means2d's
    included, stays the signed one.
    antialiased=True: the 2-D filter of Mip-Splatting (upstream 3DGS's `antialiasing`): every (view, Gaussian) opacity is multiplied by
    sqrt(max(2.5e-5, det(Sigma2D) / det(Sigma2D + dilation I))) inside the projection (siu3r_raster_project_aa), so the dilation no longer
    brightens a sub-pixel splat; everything behind the projection, n_touched and the backward included, follows the compensated record
    (siu3r_raster_project_bwd_aa differentiates the factor).  False, the default, takes the calls it took without the keyword.  K3 cameras
    with antialiased=True raise ValueError."""
    wants_grad = _wants_grad(means, cov6, shs, opacities, pose_delta, means2d)
    if wants_grad:
        _no_deferred(check_overflow)
        if pose_delta is not None and tuple(pose_delta.shape) != (len(cams), 6):
            raise ValueError(f"pose_delta must be [V, 6] = (rho, theta) per view, got {tuple(pose_delta.shape)}")
        if density_stats is not None and density_stats.G != means.shape[0]:
            raise ValueError(f"density_stats holds {density_stats.G} Gaussians, the render has {means.shape[0]}")
    _gpu(means, cov6, shs, opacities)
    pose = _pose(len(cams), means.device, pose_c2w=pose_c2w)
    if not wants_grad:
        return _rasterize_views_k2(cams, means, cov6, shs, opacities, want_n_touched, entry_capacity, check_overflow, sh_planar, pose, antialiased)
    render = lambda *gaussians: _rasterize_views_k2(cams, *gaussians, want_n_touched, entry_capacity, True, sh_planar, pose, antialiased)
    image, depth, opacity, radii, n_touched, st = _RasterizeK2.apply(render, sh_planar, density_stats, means, cov6, shs, opacities, pose_delta, means2d)
    return dict(image=image, radii=radii, depth=depth, opacity=opacity, n_touched=n_touched, state=st)


class _RasterizeK2(torch.autograd.Function):
    """The K2 forward (unchanged kernels, synchronous overflow check) and its HIP backward (csrc/raster_bwd.hip): composite backward ->
    per-(view, Gaussian) screen-space gradients -> projection backward -> Gaussians, pose (rho, theta) per view, pixel-space means."""

    @staticmethod
    def forward(ctx, render, sh_planar, density_stats, means, cov6, shs, opacities, pose_delta, means2d):
        ctx.sh_planar, ctx.density_stats = sh_planar, density_stats
        gaussians = (means, cov6, shs, opacities)
        return _forward(ctx, render, (*gaussians, pose_delta, means2d), gaussians, maps=("image", "depth", "opacity"), aux=("radii", "n_touched"))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_image, g_depth, g_opacity, _g_radii, _g_nt, _g_st):
        *inputs, image, depth, opacity = ctx.saved_tensors
        st, (means_c, cov_c, shs_c, op_c), (g_image, g_depth, g_opacity), grad = _backward_start(
            ctx, inputs, ((image, g_image), (depth, g_depth), (opacity, g_opacity)))
        lib = _lib.lib()
        V, G, dev = st.V, st.G, image.device
        ncoef = shs_c.shape[2] if ctx.sh_planar else shs_c.shape[1]
        stats = ctx.density_stats
        composite = (st.cams, V, _p(st.cams_dev), G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec), _p(image), _p(depth), _p(opacity), _p(g_image),
                     _p(g_depth), _p(g_opacity), _p(grad))
        abs_m2d = None  # absolute-gradient statistics: the per-pixel |mean terms|, summed by the same launch (the call zeroes them)
        if stats is not None and stats.absgrad:
            abs_m2d = torch.empty((V, G, 2), dtype=torch.float32, device=dev)
            check(lib.siu3r_raster_composite_rgb_bwd_abs(*composite, _p(abs_m2d), _stream()))
        else:
            check(lib.siu3r_raster_composite_rgb_bwd(*composite, _stream()))
        need_pose, need_m2d = ctx.needs_input_grad[7], ctx.needs_input_grad[8]
        g_means, g_cov, g_op, g_sh = torch.empty_like(means_c), torch.empty_like(cov_c), torch.empty_like(op_c), torch.empty_like(shs_c)
        g_m2d = torch.zeros((V, G, 2), dtype=torch.float32, device=dev) if need_m2d else None  # (culled Gaussians: not written)
        if stats is not None and abs_m2d is None and g_m2d is None:
            g_m2d = torch.empty((V, G, 2), dtype=torch.float32, device=dev)  # (the statistics go by the radii, never by an unwritten row)
        rows = int(lib.siu3r_raster_pose_partial_rows(G))
        part = torch.empty((max(rows, 1), V, 6), dtype=torch.float32, device=dev) if need_pose else None
        project_bwd = lib.siu3r_raster_project_bwd_aa if st.antialiased else lib.siu3r_raster_project_bwd
        check(project_bwd(st.cams, V, _p(st.cams_dev), G, _p(means_c), _p(cov_c), _cov_stride(cov_c), _p(op_c), _p(shs_c), ncoef,
                          int(bool(ctx.sh_planar)), _p(st.rect), _p(grad), _p(g_means), _p(g_cov), _p(g_op), _p(g_sh), _p(g_m2d), _p(part), _stream()))
        if stats is not None:
            stats.accumulate(g_m2d if abs_m2d is None else abs_m2d, st.radii, 0.5 * V * st.W, 0.5 * V * st.H)
        g_pose = None
        if need_pose:
            g_pose = torch.empty((V, 6), dtype=torch.float32, device=dev)
            if rows == 0:
                part.zero_()
            check(lib.siu3r_raster_pose_reduce(V, rows, _p(part), _p(g_pose), _stream()))
        g_mean2d = None
        if need_m2d:
            shape, dtype, _ = ctx.shapes[5]
            g_mean2d = torch.zeros(shape, dtype=dtype, device=dev)
            g_mean2d[:, :2] = g_m2d.sum(0).to(dtype)
        return (None, None, None, *_grads_out(ctx, 3, (g_means, g_cov, g_sh, g_op, g_pose)), g_mean2d)


def _rasterize_views_k2(cams, means, cov6, shs, opacities, want_n_touched, entry_capacity, check_overflow, sh_planar, pose,
                        antialiased=False) -> Dict[str, torch.Tensor]:
    def composite(st, _shs):
        V, H, W = st.V, st.H, st.W
        image, depth, alpha = _empty(st, V, 3, H, W), _empty(st, V, H, W), _empty(st, V, H, W)
        n_touched = _empty(st, V, st.G, dtype=torch.int32) if want_n_touched else None
        check(_lib.lib().siu3r_raster_composite_rgb(st.cams, st.V, _p(st.cams_dev), st.G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec),
                                                    _p(image), _p(depth), _p(alpha), _p(n_touched), _stream()))
        return dict(image=image, radii=st.radii, depth=depth, opacity=alpha, n_touched=n_touched, state=st)

    return _render(cams, means, cov6, opacities, shs, shs.shape[2] if sh_planar else shs.shape[1], pose, entry_capacity, check_overflow, composite, sh_planar,
                   antialiased)


def rasterize_k2(cam: RasterCam, means, cov6, shs, opacities, **kw) -> Dict[str, torch.Tensor]:
    """single view: image [3,H,W], radii [G,2], depth [H,W], opacity [H,W], n_touched [G] (+ state).  Keywords (antialiased among them) as
    rasterize_views_k2."""
    o = rasterize_views_k2([cam], means, cov6, shs, opacities, **kw)
    return dict(image=o["image"][0], radii=o["radii"][0], depth=o["depth"][0], opacity=o["opacity"][0],
                n_touched=None if o["n_touched"] is None else o["n_touched"][0], state=o["state"])


def _contributions(cams, means, cov6, opacities, colors, channels, pose, entry_capacity, check_overflow, want_count, want_sum, antialiased=False):
    def composite(st, _chan):
        wmax = _empty(st, st.V, st.G)
        count = _empty(st, st.V, st.G, dtype=torch.int32) if want_count else None
        wsum = _empty(st, st.V, st.G, dtype=torch.int64) if want_sum else None
        check(_lib.lib().siu3r_raster_contrib(st.cams, st.V, _p(st.cams_dev), st.G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec), _p(wmax),
                                              _p(count), _p(wsum), _stream()))
        return dict(wmax=wmax, count=count, wsum=wsum, radii=st.radii, state=st)

    _gpu(means, cov6, opacities)
    means, cov6, opacities = (t.detach() for t in (means, cov6, opacities))
    return _render(cams, means, cov6, opacities, means if colors is None else colors, channels, pose, entry_capacity, check_overflow, composite,
                   antialiased=antialiased)


def contributions_k2(cams: Sequence[RasterCam], means, cov6, opacities, entry_capacity=None, check_overflow=True, pose_c2w=None, want_count=True,
                     want_sum=True, antialiased=False) -> Dict[str, torch.Tensor]:
    """Blend-contribution statistics of V views of one Gaussian set, 3DGS family (siu3r_raster_contrib): with w = alpha * T the very float
    rasterize_views_k2 adds into a pixel, over the pixels of view v that blend Gaussian g -> wmax [V,G] f32 (the largest w; exactly 0 where g
    blends nowhere), count [V,G] i32 (the number of those pixels), wsum [V,G] i64 (the sum of trunc(w * 2^40): fixed point, units of 2^-40),
    radii [V,G,2] i32 + the call's state.  Integer reductions only: two calls give the same bits.  entry_capacity / check_overflow /
    pose_c2w as in rasterize_views_k2 (a view that overflowed an unchecked call has a NaN wmax row and zero count / wsum).  Colours take no
    part: the call projects with sh_degree = -1 on its own copy of the camera blocks and hands the projection `means` as the [G,3] colour
    operand it insists on -- no SH evaluation and no colour tensor.  No autograd: the inputs are detached.  want_count / want_sum = False
    leave that output None.  antialiased=True: the weights of rasterize_views_k2(antialiased=True) (the compensated opacities)."""
    k2 = []
    for c in cams:
        c2 = RasterCam()
        C.memmove(C.byref(c2), C.byref(c), C.sizeof(RasterCam))
        c2.sh_degree, c2.sh_band4 = -1, 0
        k2.append(c2)
    return _contributions(k2, means, cov6, opacities, means.detach().contiguous().float(), 1, _pose(len(cams), means.device, pose_c2w=pose_c2w), entry_capacity,
                          check_overflow, want_count, want_sum, antialiased)


def contributions_k3(cams: Sequence[RasterCam], means, cov6, opacities, entry_capacity=None, check_overflow=True, pose_dev=None, pose_c2w=None,
                     want_count=True, want_sum=True) -> Dict[str, torch.Tensor]:
    """contributions_k2 for the gsplat family (pixel centres at +0.5, saturation nT <= t_min): w is the weight rasterize_views_k3 and
    rasterize_views_k3_rgb give the Gaussian's feature row in that pixel.  The mode-1 projection takes no colour operand at all."""
    return _contributions(cams, means, cov6, opacities, None, 0, _pose(len(cams), means.device, pose_dev, pose_c2w), entry_capacity, check_overflow,
                          want_count, want_sum)


def tune(key: int, value: int) -> None:
    """siu3r_raster_tune: key 0 -- 1 = the 32-channel kernel for every N-channel composite (features that may be non-finite; A/B), 0 = default;
    key 1 -- accumulator blocks per chunk of the matrix-core composite (1 .. 6).  Process-wide, not for concurrent use."""
    check(_lib.lib().siu3r_raster_tune(int(key), int(value)))


def _k3_gate(check_overflow, means, cov6, opacities, chan, pose_dev):
    """the grad gate of both K3 entry points -> (a gradient is wanted, the viewmats of pose_dev: the fifth differentiable argument)"""
    vm = pose_dev[0] if pose_dev is not None else None
    wants_grad = _wants_grad(means, cov6, opacities, chan, vm)
    if wants_grad:
        _no_deferred(check_overflow)
    _gpu(means, cov6, opacities, chan)
    return wants_grad, vm


def _k3_call(function, render, wants_grad, *diff):
    if not wants_grad:
        return render(*diff[:4])
    colors, alphas, radii, st = function.apply(render, *diff)
    return dict(colors=colors, alphas=alphas, radii=radii, state=st)


def rasterize_views_k3(cams: Sequence[RasterCam], means, cov6, opacities, feats, entry_capacity=None, pair_capacity=None,
                       check_overflow=True, pose_dev=None, matrix_form=True, pose_c2w=None) -> Dict[str, torch.Tensor]:
    """feats [G,C] -> colors [V,H,W,C], alphas [V,H,W] (+ state).  gsplat semantics: the per-tile lists are materialised once; for
    C >= 32 they are cut per 8 x 8 quadrant and blended on the matrix cores, all channels at once (identical bits for FINITE features).
    matrix_form=False: the 32-channel kernel, whose pixels only ever see the rows that blend into them -- for features that may hold
    inf / NaN (include/siu3r_hip.h, siu3r_raster_composite_feat_ws).

    Differentiable when grad mode is on and means / cov6 / opacities / feats / the viewmats of pose_dev require grad (_RasterizeK3; the
    outputs are the same bits as without grad).  The gradient is undefined for non-finite features.  Every other call runs the plain forward."""
    wants_grad, vm = _k3_gate(check_overflow, means, cov6, opacities, feats, pose_dev)
    if check_overflow == "deferred":
        raise ValueError('check_overflow="deferred" is only safe on the RGB composites (an overflowing view is NaN-poisoned there); the '
                         "N-channel composite has no such marker: pass True (check now) or False (and call state.verify())")
    pose, check = _pose(len(cams), means.device, pose_dev, pose_c2w), wants_grad or check_overflow
    render = lambda m, c, o, f: _rasterize_views_k3(cams, m, c, o, f, entry_capacity, pair_capacity, check, pose, matrix_form)
    return _k3_call(_RasterizeK3, render, wants_grad, means, cov6, opacities, feats, vm)


def _project_bwd_k3(st, means, cov6, grad, need_pose, g_colors=None):
    """the mode-1 projection backward of a finished composite backward (grad [V,G,GR_N]) -> g_means, g_cov, g_opacities, g_viewmats [V,4,4]"""
    lib = _lib.lib()
    V, G, dev = st.V, st.G, means.device
    g_means, g_cov, g_op = torch.empty_like(means), torch.empty_like(cov6), torch.empty((G,), dtype=torch.float32, device=dev)
    rows = int(lib.siu3r_raster_pose_partial_rows(G))
    part = torch.zeros((max(rows, 1), V, 12), dtype=torch.float32, device=dev) if need_pose else None
    check(lib.siu3r_raster_project_bwd_k3(st.cams, V, _p(st.cams_dev), G, _p(means), _p(cov6), _cov_stride(cov6), _p(st.rect), _p(grad),
                                          _p(g_means), _p(g_cov), _p(g_op), _p(g_colors), _p(part), _stream()))
    g_vm = None
    if need_pose:
        g_vm = torch.empty((V, 4, 4), dtype=torch.float32, device=dev)
        check(lib.siu3r_raster_viewmat_reduce(V, rows, _p(part), _p(g_vm), _stream()))
    return g_means, g_cov, g_op, g_vm


class _RasterizeK3(torch.autograd.Function):
    """The K3 N-channel forward (unchanged kernels, synchronous overflow check) and its HIP backward (csrc/raster_bwd_k3.hip): composite
    backward over the per-quadrant lists (the forward's workspace, or built here) -> per-(view, Gaussian) screen-space gradients and the
    feature gradient -> projection backward -> Gaussians and world->camera matrices."""

    @staticmethod
    def forward(ctx, render, means, cov6, opacities, feats, viewmats):
        return _forward(ctx, render, (means, cov6, opacities, feats, viewmats), (means, cov6, feats), maps=("colors", "alphas"), aux=("radii",))  # (feats: read again)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_colors, g_alphas, _g_radii, _g_st):
        *inputs, colors, alphas = ctx.saved_tensors
        st, (means_c, cov_c, feats_c), (g_colors, g_alphas), grad = _backward_start(ctx, inputs, ((colors, g_colors), (alphas, g_alphas)))
        lib = _lib.lib()
        V, G = st.V, st.G
        tstart, ids_all, cap_d = st.tile_start_all, st.ids_all, st.cap_d
        # the per-quadrant lists: the forward's when its matrix-core form built them, else built now (whichever forward kernel ran -- the
        # 32-channel one below 32 channels, after tune(0, 1) or for scenes past 32-bit offsets -- these lists give the same walk)
        ws = st.feat_ws
        if not st.feat_ws_lists:
            if ws is None:
                ws = torch.empty((int(lib.siu3r_raster_composite_feat_ws_bytes(st.W, st.H, V, cap_d)) // 4,), dtype=torch.int32, device=colors.device)
            check(lib.siu3r_raster_quad_lists(st.cams, V, _p(st.cams_dev), G, _p(tstart), _p(ids_all), cap_d, _p(st.rec), _p(ws), ws.numel() * 4, _stream()))
        g_feats = torch.empty_like(feats_c)
        check(lib.siu3r_raster_composite_feat_bwd(st.cams, V, _p(st.cams_dev), G, _p(tstart), _p(ws), cap_d, _p(st.rec), _p(feats_c), feats_c.shape[1],
                                                  _p(colors), _p(alphas), _p(g_colors), _p(g_alphas), _p(grad), _p(g_feats), _stream()))
        g_means, g_cov, g_op, g_vm = _project_bwd_k3(st, means_c, cov_c, grad, ctx.needs_input_grad[5])
        return (None, *_grads_out(ctx, 1, (g_means, g_cov, g_op, g_feats, g_vm)))


def _rasterize_views_k3(cams, means, cov6, opacities, feats, entry_capacity, pair_capacity, check_overflow, pose, matrix_form) -> Dict[str, torch.Tensor]:
    def composite(st, feats):
        V, G, W, H, Cc = st.V, st.G, st.W, st.H, feats.shape[1]
        st.cap_d_hint = int(pair_capacity) if pair_capacity else default_pair_capacity(G)
        out, alpha = _empty(st, V, H, W, Cc), _empty(st, V, H, W)
        lib = _lib.lib()
        tstart, ids_all, cap_d = st.tile_start_all, st.ids_all, st.cap_d
        # workspace of the per-quadrant lists (C >= 32: every wave of the composite walks its own 8 x 8 quadrant's list)
        ws = _empty(st, int(lib.siu3r_raster_composite_feat_ws_bytes(W, H, V, cap_d)) // 4, dtype=torch.int32) if (Cc >= 32 and matrix_form) else None
        st.feat_ws = ws
        # (whether the forward leaves the per-quadrant lists in ws: a backward reuses them instead of building them again)
        st.feat_ws_lists = ws is not None and bool(lib.siu3r_raster_composite_feat_ws_lists(W, H, V, G, _p(feats), Cc, _p(ws), ws.numel() * 4, cap_d))
        check(lib.siu3r_raster_composite_feat_ws(st.cams, V, _p(st.cams_dev), G, _p(tstart), _p(ids_all), cap_d, _p(st.rec), _p(feats), Cc,
                                                 _p(out), _p(alpha), _p(ws), 0 if ws is None else ws.numel() * 4, _stream()))
        return dict(colors=out, alphas=alpha, radii=st.radii, state=st)

    return _render(cams, means, cov6, opacities, feats, 0, pose, entry_capacity, check_overflow, composite)


def rasterize_views_k3_rgb(cams: Sequence[RasterCam], means, cov6, opacities, rgb, entry_capacity=None, check_overflow=True,
                           pose_dev=None) -> Dict[str, torch.Tensor]:
    """gsplat semantics with THREE precomputed colour channels (rgb [G,3]) -> colors [V,H,W,3], alphas [V,H,W] (+ state), through the
    fused sort-free composite: the colour travels in the per-Gaussian record and no per-tile list is written to HBM (the N-channel
    path materialises the lists because every 32-channel chunk re-walks them).

    Differentiable when grad mode is on and means / cov6 / opacities / rgb / the viewmats of pose_dev require grad (_RasterizeK3RGB)."""
    wants_grad, vm = _k3_gate(check_overflow, means, cov6, opacities, rgb, pose_dev)
    assert rgb.shape[1] == 3
    pose, check = _pose(len(cams), means.device, pose_dev), wants_grad or check_overflow
    render = lambda m, c, o, r: _rasterize_views_k3_rgb(cams, m, c, o, r, entry_capacity, check, pose)
    return _k3_call(_RasterizeK3RGB, render, wants_grad, means, cov6, opacities, rgb, vm)


class _RasterizeK3RGB(torch.autograd.Function):
    """The K3 three-channel fused forward and its HIP backward: composite_rgb_bwd_kernel<K3> (csrc/raster_bwd.hip) re-walks the coarse
    bins like the forward, then the mode-1 projection backward (csrc/raster_bwd_k3.hip) takes the record colours' gradient to rgb."""

    @staticmethod
    def forward(ctx, render, means, cov6, opacities, rgb, viewmats):
        return _forward(ctx, render, (means, cov6, opacities, rgb, viewmats), (means, cov6), maps=("colors", "alphas"), aux=("radii",))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_colors, g_alphas, _g_radii, _g_st):
        *inputs, colors, alphas = ctx.saved_tensors
        st, (means_c, cov_c), (g_colors, g_alphas), grad = _backward_start(ctx, inputs, ((colors, g_colors), (alphas, g_alphas)))
        check(_lib.lib().siu3r_raster_composite_rgb_bwd_k3(st.cams, st.V, _p(st.cams_dev), st.G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec),
                                                           _p(colors), _p(alphas), _p(g_colors), _p(g_alphas), _p(grad), _stream()))
        g_rgb = torch.empty((st.G, 3), dtype=torch.float32, device=colors.device)
        g_means, g_cov, g_op, g_vm = _project_bwd_k3(st, means_c, cov_c, grad, ctx.needs_input_grad[5], g_colors=g_rgb)
        return (None, *_grads_out(ctx, 1, (g_means, g_cov, g_op, g_rgb, g_vm)))


def _rasterize_views_k3_rgb(cams, means, cov6, opacities, rgb, entry_capacity, check_overflow, pose) -> Dict[str, torch.Tensor]:
    def composite(st, _rgb):
        out, alpha = _empty(st, st.V, st.H, st.W, 3), _empty(st, st.V, st.H, st.W)
        check(_lib.lib().siu3r_raster_composite_rgb(st.cams, st.V, _p(st.cams_dev), st.G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec),
                                                    _p(out), None, _p(alpha), None, _stream()))
        return dict(colors=out, alphas=alpha, radii=st.radii, state=st)

    return _render(cams, means, cov6, opacities, rgb, 3, pose, entry_capacity, check_overflow, composite)


def rasterize_k3(cam: RasterCam, means, cov6, opacities, feats, **kw) -> Dict[str, torch.Tensor]:
    o = rasterize_views_k3([cam], means, cov6, opacities, feats, **kw)
    return dict(colors=o["colors"][0], alphas=o["alphas"][0], radii=o["radii"][0], state=o["state"])


def scale_inplace_(x: torch.Tensor, s: float):
    _gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    check(_lib.lib().siu3r_scale_inplace(_p(x), x.numel(), float(s), _stream()))
    return x


def quat_scale_to_cov6(quats_wxyz: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """[G,4] (w,x,y,z) + [G,3] -> [G,6] (gsplat's quat_scale_to_covar, upper triangle).  Differentiable (through the normalisation)."""
    if _wants_grad(quats_wxyz, scales):
        return _QuatScaleCov6.apply(quats_wxyz, scales)
    return _quat_scale_to_cov6(quats_wxyz, scales)


def _quat_scale_to_cov6(quats_wxyz, scales):
    _gpu(quats_wxyz, scales)
    q, sc = quats_wxyz.contiguous().float(), scales.contiguous().float()
    out = torch.empty((q.shape[0], 6), dtype=torch.float32, device=q.device)
    check(_lib.lib().siu3r_quat_scale_to_cov6(_p(q), _p(sc), _p(out), q.shape[0], _stream()))
    return out


class _QuatScaleCov6(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quats, scales):
        ctx.save_for_backward(quats, scales)
        return _quat_scale_to_cov6(quats.detach(), scales.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cov6):
        quats, scales = ctx.saved_tensors
        q, sc = quats.detach().contiguous().float(), scales.detach().contiguous().float()
        gq, gs = torch.empty_like(q), torch.empty_like(sc)
        check(_lib.lib().siu3r_quat_scale_to_cov6_bwd(_p(q), _p(sc), _p(g_cov6.detach().float().contiguous()), _p(gq), _p(gs), q.shape[0], _stream()))
        return (gq.to(quats.dtype) if ctx.needs_input_grad[0] else None, gs.to(scales.dtype) if ctx.needs_input_grad[1] else None)


def sh_eval(means: torch.Tensor, campos, sh: torch.Tensor, degree: int) -> torch.Tensor:
    """means [G,3], campos (3 floats on the host, or a DEVICE tensor of 3 floats: no read-back), sh [G,ncoef,3] -> rgb [G,3] =
    max(SH . coeffs + 0.5, 0).  Differentiable w.r.t. means, sh and a device campos (zero gradient where a colour was clamped at 0)."""
    cp_t = campos if isinstance(campos, torch.Tensor) else None
    if _wants_grad(means, sh, cp_t):
        if cp_t is None:
            cp_t = torch.tensor([float(v) for v in campos], dtype=torch.float32, device=means.device)
        elif not cp_t.is_cuda:  # (a differentiable copy: a host campos that requires grad gets its gradient back on the host)
            cp_t = cp_t.to(device=means.device, dtype=torch.float32)
        return _ShEval.apply(means, cp_t, sh, int(degree))
    return _sh_eval(means, campos, sh, degree)


def _sh_eval(means, campos, sh, degree):
    _gpu(means, sh)
    means, sh = means.contiguous().float(), sh.contiguous().float()
    out = torch.empty((means.shape[0], 3), dtype=torch.float32, device=means.device)
    if isinstance(campos, torch.Tensor) and campos.is_cuda:
        cp = campos.detach().float().contiguous()
        assert cp.numel() == 3
        check(_lib.lib().siu3r_sh_eval_dp(_p(means), _p(cp), _p(sh), sh.shape[1], int(degree), _p(out), means.shape[0], _stream()))
        return out
    cam = (C.c_float * 3)(*[float(v) for v in campos])
    check(_lib.lib().siu3r_sh_eval(_p(means), C.cast(cam, C.c_void_p), _p(sh), sh.shape[1], int(degree), _p(out), means.shape[0], _stream()))
    return out


class _ShEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, campos, sh, degree):
        ctx.save_for_backward(means, campos, sh)
        ctx.degree = degree
        return _sh_eval(means.detach(), campos.detach(), sh.detach(), degree)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb):
        means, campos, sh = ctx.saved_tensors
        m, cp, s = (t.detach().contiguous().float() for t in (means, campos, sh))
        g_m, g_sh, g_cp = torch.empty_like(m), torch.empty_like(s), torch.empty((3,), dtype=torch.float32, device=m.device)
        check(_lib.lib().siu3r_sh_eval_bwd(_p(m), _p(cp), _p(s), s.shape[1], ctx.degree, _p(g_rgb.detach().float().contiguous()), _p(g_sh), _p(g_m),
                                           _p(g_cp), m.shape[0], _stream()))
        need = ctx.needs_input_grad
        return (g_m.to(means.dtype) if need[0] else None, g_cp.reshape(campos.shape).to(campos.dtype) if need[1] else None,
                g_sh.to(sh.dtype) if need[2] else None, None)


def blend_background_(colors: torch.Tensor, alphas: torch.Tensor, bg) -> torch.Tensor:
    """colors [H,W,C] += (1 - alphas[H,W]) * bg, in place.  bg: C <= 3 floats on the host, or a DEVICE tensor of C floats (any C, no read-back)."""
    _gpu(colors, alphas)
    assert colors.is_contiguous() and alphas.is_contiguous() and colors.dtype == torch.float32
    if isinstance(bg, torch.Tensor) and bg.is_cuda:
        b = bg.detach().float().contiguous()
        assert b.numel() == colors.shape[-1], (tuple(b.shape), tuple(colors.shape))
        check(_lib.lib().siu3r_blend_background_dp(_p(colors), _p(alphas), _p(b), colors.shape[-1], alphas.numel(), _stream()))
        return colors
    b = (C.c_float * 3)(*([float(v) for v in bg] + [0.0] * (3 - len(bg))))
    check(_lib.lib().siu3r_blend_background(_p(colors), _p(alphas), C.cast(b, C.c_void_p), colors.shape[-1], alphas.numel(), _stream()))
    return colors


def blend_background(colors: torch.Tensor, alphas: torch.Tensor, bg: torch.Tensor) -> torch.Tensor:
    """Out-of-place, differentiable form of blend_background_ (the same kernel on a copy: the same bits): colors [...,C] + (1 - alphas[...])
    * bg [C] (a device tensor).  Gradients reach colors, alphas and bg."""
    return _BlendBackground.apply(colors, alphas, bg)


class _BlendBackground(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, alphas, bg):
        ctx.save_for_backward(alphas, bg)
        out = colors.detach().float().contiguous().clone()
        return blend_background_(out, alphas.detach().float().contiguous(), bg.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        # d out / d colors = 1, d out / d alphas = -bg, d out / d bg = 1 - alphas: elementwise products and sums over the pixels
        alphas, bg = ctx.saved_tensors
        b = bg.detach().float().reshape(-1)
        g_al = -(g * b).sum(-1) if ctx.needs_input_grad[1] else None
        g_bg = (g * (1.0 - alphas.detach().float())[..., None]).reshape(-1, b.numel()).sum(0).reshape(bg.shape).to(bg.dtype) if ctx.needs_input_grad[2] else None
        return g, g_al, g_bg


def algorithmic_bytes(G: int, G_v: int, D: int, P: int, channels: Optional[int] = None) -> int:
    """Algorithmic HBM bytes of one rendered view: RGB path 348 G + 48 G_v + 88 D + 20 P;
    C-channel path (44+4C) G + 36 G_v + (76+4C) D + (4C+4) P."""
    if channels is None:
        return 348 * G + 48 * G_v + 88 * D + 20 * P
    return (44 + 4 * channels) * G + 36 * G_v + (76 + 4 * channels) * D + (4 * channels + 4) * P
