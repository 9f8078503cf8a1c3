"""Instance-aware depth smoothness in per-scene refinement: the control refine.refine_gaussians' `smooth=` takes.  The term itself is
losses.depth_smoothness (csrc/depth_smooth.hip): differences of the rendered depth of the training views, switched off
wherever neighbouring pixels belong to different panoptic segments or are void, so that depth may jump at object boundaries and is pulled
flat (order 1) or planar (order 2) inside one instance.  The segment maps are what SIU3RModel.forward returns for its context views."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple, Union

from .losses import SMOOTH_ORDERS, SMOOTH_SPACES


@dataclass
class DepthSmoothness:
    """What refine.refine_gaussians' `smooth=` switches on: iteration t's objective gains weight_t * losses.depth_smoothness(render depth,
    render opacity, segments, order, space, min_opacity) on the iteration's own render.  weight: a float, or a (start, end) pair of positive
    numbers decayed exponentially over the iterations (refine.depth_weight_schedule).  order, space, min_opacity: depth_smoothness's."""
    weight: Union[float, Tuple[float, float]] = 1.0
    order: int = 1
    space: str = "render"
    min_opacity: float = 0.5

    def validate(self):
        if isinstance(self.order, bool) or self.order not in SMOOTH_ORDERS:
            raise ValueError(f"DepthSmoothness: order must be one of {SMOOTH_ORDERS}, got {self.order!r}")
        if self.space not in SMOOTH_SPACES:
            raise ValueError(f"DepthSmoothness: space must be one of {tuple(SMOOTH_SPACES)}, got {self.space!r}")
        if not 0.0 <= float(self.min_opacity) < math.inf:
            raise ValueError(f"DepthSmoothness: min_opacity must be finite and >= 0, got {self.min_opacity}")
        if isinstance(self.weight, (tuple, list)):
            if len(self.weight) != 2 or not all(0.0 < float(w) < math.inf for w in self.weight):
                raise ValueError(f"DepthSmoothness: a (start, end) weight must be two positive finite numbers, got {self.weight!r}")
        elif not 0.0 < float(self.weight) < math.inf:
            raise ValueError(f"DepthSmoothness: weight must be positive and finite (a weight of 0 everywhere is smooth=None), got {self.weight!r}")

    def weights(self, iters: int) -> List[float]:
        """the weight of the term at every iteration: the schedule of the depth term, reused"""
        from .refine import depth_weight_schedule

        return depth_weight_schedule(self.weight, iters)
