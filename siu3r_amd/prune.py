"""Contribution pruning: drop the Gaussians that never reach a meaningful blending weight in any training view (RadSplat, Niemeyer et al.
2024: the largest alpha * T over all rays; the sum of the weights is the significance score of LightGaussian and the sampling weight of
Mini-Splatting).  The statistics come from one kernel next to the K2 composite (csrc/contrib.hip, raster.contributions_k2): the walk of
the forward without colours, reduced per Gaussian with integer operations only, so every number here is bit-reproducible and any
chunking of the views gives identical bits."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import raster
from .density import FIELDS, _check_params, event_iterations

WSUM_UNIT = 2.0 ** -40  # one unit of the fixed-point weight sums


class ContributionStats:
    """The blend contributions of G Gaussians over the views seen so far: wmax [G] f32 (the largest blending weight alpha * T in any pixel
    of any view), wsum [G] i64 (the sum of the weights over all pixels and views, fixed point in units of 2^-40), count [G] i64 (pixels
    that blend the Gaussian), views [G] i32 (views in which at least one pixel does)."""

    def __init__(self, G: int, device):
        self.G = int(G)
        self.wmax = torch.zeros(self.G, dtype=torch.float32, device=device)
        self.wsum = torch.zeros(self.G, dtype=torch.int64, device=device)
        self.count = torch.zeros(self.G, dtype=torch.int64, device=device)
        self.views = torch.zeros(self.G, dtype=torch.int32, device=device)

    def accumulate(self, out: Dict[str, torch.Tensor]):
        """fold the [V,G] outputs of one raster.contributions_k2 / _k3 call in: wmax takes the maximum (a NaN row -- a view that overflowed
        an unchecked call -- stays NaN), wsum, count and views add.  Integer sums and a maximum: the order of the calls does not matter."""
        wmax, wsum, count = out["wmax"], out["wsum"], out["count"]
        if wsum is None or count is None:
            raise ValueError("ContributionStats needs all three statistics (want_count / want_sum)")
        if wmax.dim() != 2 or wmax.shape[1] != self.G or wsum.shape != wmax.shape or count.shape != wmax.shape:
            raise ValueError(f"contribution statistics of {self.G} Gaussians: the outputs must be [V, {self.G}], got {tuple(wmax.shape)}")
        if wmax.shape[0] == 0 or self.G == 0:
            return
        self.wmax = torch.maximum(self.wmax, wmax.amax(0))
        self.wsum += wsum.sum(0)
        self.count += count.sum(0, dtype=torch.int64)
        self.views += (count > 0).sum(0, dtype=torch.int32)

    def weight_sum(self) -> torch.Tensor:
        """the summed blending weights as float64 (wsum * 2^-40: exact up to 2^53 units)"""
        return self.wsum.to(torch.float64) * WSUM_UNIT


def gaussian_contributions(means, scales, rotations, opacities, c2w, Kn, near, far, image_shape, view_chunk: int = 8,
                           translation_scale: float = 1.0, antialiased: bool = False) -> ContributionStats:
    """The contributions of one Gaussian set to V posed views, in the conventions of cuda_splatting.render_cuda and refine.refine_gaussians:
    means [G,3], scales [G,3], rotations [G,4] raw (x, y, z, w) quaternions, opacities [G] (all in their natural form, on the GPU); c2w
    [V,4,4] camera-to-world, Kn [V,3,3] (or [3,3]) normalised intrinsics, near / far floats (or [V]), image_shape (H, W).  The poses are
    consumed on the device.  `view_chunk` views go through the rasterizer per call (it bounds the [V,G] temporaries).  antialiased: the
    weights of the anti-aliased render (raster.contributions_k2)."""
    if int(view_chunk) <= 0:
        raise ValueError(f"view_chunk must be positive, got {view_chunk}")
    dev = means.device
    H, W = (int(s) for s in image_shape)
    c2w = c2w.detach().float().to(dev)
    V = c2w.shape[0]
    Kn = Kn.detach().float().to(dev)
    Kn = (Kn[None].expand(V, 3, 3) if Kn.dim() == 2 else Kn).contiguous()
    as_v = lambda x: x.detach().float().cpu().reshape(-1).expand(V).tolist() if isinstance(x, torch.Tensor) else [float(x)] * V
    near_v, far_v = as_v(near), as_v(far)
    with torch.no_grad():
        cov6 = raster.quat_scale_to_cov6(torch.roll(rotations.detach(), 1, dims=-1), scales.detach())
        stats = ContributionStats(means.shape[0], dev)
        for v0 in range(0, V, int(view_chunk)):
            v1 = min(V, v0 + int(view_chunk))
            cams = [raster.make_cam_k2(None, None, None, None, None, (0.0, 0.0, 0.0), W, H, sh_degree=-1, near=near_v[v], far=far_v[v]) for v in range(v0, v1)]
            stats.accumulate(raster.contributions_k2(cams, means, cov6, opacities, pose_c2w=(c2w[v0:v1], Kn[v0:v1], float(translation_scale)),
                                                     **(dict(antialiased=True) if antialiased else {})))
    return stats


def prune_by_contribution(params: Dict[str, torch.Tensor], stats: ContributionStats, min_weight: float = 0.01, min_views: int = 1,
                          keep_at_most: Optional[int] = None, moments: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None):
    """params: the five FIELDS (any parametrisation: rows are only selected); moments: {field: (exp_avg, exp_avg_sq)} of the fields Adam
    moves.  A row is kept when stats.wmax >= min_weight (compared in float32) and stats.views >= min_views; keep_at_most = N then keeps
    only the N of those with the largest wsum (ties go to the lower index).  The compaction preserves the order and copies the kept rows
    of every field and moment bit for bit.  A NaN wmax (a view of an unchecked call overflowed) raises.  One host read.
    Returns (new params, new moments, info = {"rows_in", "rows_out", "pruned", "never_blended"})."""
    moments = moments or {}
    G = _check_params(params, moments, stats.G)
    if keep_at_most is not None and int(keep_at_most) < 0:
        raise ValueError(f"keep_at_most must be >= 0 (or None), got {keep_at_most}")
    thr = torch.tensor(float(min_weight), dtype=torch.float32, device=stats.wmax.device)
    keep = (stats.wmax >= thr) & (stats.views >= int(min_views))
    if keep_at_most is not None:
        score = torch.where(keep, stats.wsum, torch.full_like(stats.wsum, -1))
        order = torch.sort(score, descending=True, stable=True).indices[: int(keep_at_most)]
        top = torch.zeros_like(keep)
        top[order] = True
        keep = keep & top
    idx = torch.nonzero(keep).reshape(-1)
    nan, never, rows_out = (int(x) for x in torch.stack((torch.isnan(stats.wmax).sum(), (stats.count == 0).sum(), keep.sum())).tolist())
    if nan:
        raise RuntimeError(f"contribution statistics hold {nan} NaN rows: a view overflowed its coarse-bin entries in an unchecked call")
    new_p = {k: params[k].index_select(0, idx) for k in FIELDS}
    new_m = {k: (m[0].index_select(0, idx), m[1].index_select(0, idx)) for k, m in moments.items()}
    return new_p, new_m, dict(rows_in=G, rows_out=rows_out, pruned=G - rows_out, never_blended=never)


@dataclass
class ContributionPrune:
    """When and how refine.refine_gaussians prunes by contribution (its `prune=` keyword).  min_weight / min_views / keep_at_most are
    prune_by_contribution's; RadSplat uses min_weight 0.01 during training and up to 0.25 for light models.  The schedule is
    density.event_iterations': events before the renders of start, start + every, ... up to and including stop (None: iters - every),
    never iteration 0.  final = True runs one more event after the last iteration, so that the returned set is pruned."""
    min_weight: float = 0.01
    min_views: int = 1
    keep_at_most: Optional[int] = None
    start: int = 100
    every: int = 100
    stop: Optional[int] = None
    final: bool = False

    def events(self, iters: int) -> List[int]:
        return event_iterations(self.start, self.every, self.stop, iters, "ContributionPrune")
