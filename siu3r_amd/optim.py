"""The optimiser of splat refinement on the GPU: Adam over all Gaussian fields as ONE fused HIP launch per step (csrc/gaussian_adam.hip,
DESIGN.md section 12), which leaves alone the Gaussians that no view of the iteration's render saw, and the learning-rate rules of the
3DGS training recipe (Kerbl et al. 2023): the higher SH bands at a fraction of the DC rate, a log-linear decay of the position rate.

The arithmetic of a visible row is torch.optim.Adam's (amsgrad off, no weight decay) in float32; the bias corrections use the optimiser's
GLOBAL step count, also for a row that earlier steps skipped.  There is no CPU path and nothing here synchronises with the host.

TorchAdam puts torch.optim.Adam behind the same surface (moments / rebind / zero_moments / zero_grad / step), so that refine.refine_gaussians
drives either optimiser with one set of statements."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _gpu, _p, _stream

MAX_FIELDS = 8  # SIU3R_ADAM_MAX_FIELDS
SH_FIELD = "harmonics"  # [G,3,n]: the field whose first coefficient per colour steps at lr and the others at lr * sh_rest_lr_scale


def log_linear(a: float, b: float, n: int) -> List[float]:
    """n values from a to b (both positive), v_t = a * (b / a) ** (t / (n - 1)) with both endpoints exact; n <= 1 gives [a] * n"""
    if n <= 1:
        return [a] * n
    return [a] + [a * (b / a) ** (t / (n - 1)) for t in range(1, n - 1)] + [b]


def means_lr_schedule(lr_init: float, lr_final: float, iters: int) -> List[float]:
    """The position learning rate at every iteration: log-linear interpolation lr_t = lr_init * (lr_final / lr_init) ** (t / (iters - 1))
    with both endpoints exact (the decay of the 3DGS recipe, without its delay); iters == 1 gives [lr_init]."""
    n = max(int(iters), 0)
    a, b = float(lr_init), float(lr_final)
    if not (0.0 < a < math.inf and 0.0 < b < math.inf):
        raise ValueError(f"means_lr_schedule: lr_init and lr_final must both be positive and finite, got {lr_init!r}, {lr_final!r}")
    return log_linear(a, b, n)


def _rate(name: str, v) -> float:
    v = float(v)
    if not 0.0 <= v < math.inf:
        raise ValueError(f"learning rate of {name!r} must be finite and >= 0, got {v}")
    return v


class GaussianAdam:
    """Adam over named fields of G Gaussians.  params: {field: float32 GPU leaf tensor [G, ...], contiguous}, at most 8 fields, one G;
    lrs: {field: rate} for every field of params.  A field called "harmonics" ([G,3,n]) steps its DC coefficients at its rate and the
    other coefficients at rate * sh_rest_lr_scale (3DGS: 0.05)."""

    def __init__(self, params: Dict[str, torch.Tensor], lrs: Dict[str, float], betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-15,
                 sh_rest_lr_scale: float = 1.0):
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
        if not 0.0 <= float(eps) < math.inf:
            raise ValueError(f"eps must be finite and >= 0, got {eps}")
        if not 0.0 <= float(sh_rest_lr_scale) < math.inf:
            raise ValueError(f"sh_rest_lr_scale must be finite and >= 0, got {sh_rest_lr_scale}")
        self.betas, self.eps, self.sh_rest_lr_scale = (b1, b2), float(eps), float(sh_rest_lr_scale)
        self.step_count = 0
        self._ws = None
        self._bind(params)
        self.lrs = self._rates(lrs, dict.fromkeys(self.params))
        missing = [k for k in self.params if self.lrs[k] is None]
        if missing:
            raise ValueError(f"lrs: no learning rate for {missing}")
        self._moments = {k: (torch.zeros_like(p, memory_format=torch.contiguous_format), torch.zeros_like(p, memory_format=torch.contiguous_format))
                         for k, p in self.params.items()}

    # ---- validation ------------------------------------------------------------------------------------------------------------------------
    def _rates(self, lrs, base):
        out = dict(base)
        for k, v in (lrs or {}).items():
            if k not in self.params:
                raise ValueError(f"lrs: unknown field {k!r} (one of {tuple(self.params)})")
            out[k] = _rate(k, v)
        return out

    @staticmethod
    def _check_like(name, t, like):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _gpu(t)
        if t.dtype != torch.float32 or t.shape != like.shape or t.device != like.device or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor {tuple(like.shape)} on {like.device}, got {tuple(t.shape)} {t.dtype} on {t.device}"
                             f"{'' if t.is_contiguous() else ', not contiguous'}")

    def _bind(self, params):
        if not isinstance(params, dict) or not 1 <= len(params) <= MAX_FIELDS:
            raise ValueError(f"params must be a dict of 1 .. {MAX_FIELDS} fields, got {len(params) if isinstance(params, dict) else type(params).__name__}")
        first = None
        for k, p in params.items():
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"params[{k!r}] must be a tensor, got {type(p).__name__}")
            _gpu(p)
            first = p if first is None else first
            if p.dtype != torch.float32 or p.dim() < 1 or p.numel() == 0 or not p.is_contiguous():
                raise ValueError(f"params[{k!r}] must be a non-empty contiguous float32 tensor [G, ...], got {tuple(p.shape)} {p.dtype}")
            if p.shape[0] != first.shape[0] or p.device != first.device:
                raise ValueError(f"params[{k!r}] has {p.shape[0]} rows on {p.device}, the first field {first.shape[0]} on {first.device}")
            if k == SH_FIELD and p.dim() != 3:
                raise ValueError(f"params[{k!r}] must be [G, 3, n], got {tuple(p.shape)}")
        self.params = dict(params)
        self.G = int(first.shape[0])
        self.device = first.device

    # ---- state -----------------------------------------------------------------------------------------------------------------------------
    @property
    def moments(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """{field: (exp_avg, exp_avg_sq)}: the tensors the kernel updates, the form density.densify_and_prune takes"""
        return dict(self._moments)

    def rebind(self, params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]]):
        """new leaves and their moments after a density event (another row count is fine); the step count and the rates are kept"""
        if set(params) != set(self.params) or set(moments) != set(self.params):
            raise ValueError(f"rebind: the fields must stay {tuple(self.params)}, got params {tuple(params)} and moments {tuple(moments)}")
        old = (self.params, self.G, self.device)
        order = list(self.params)
        self._bind({k: params[k] for k in order})
        try:
            for k in order:
                self._check_like(f"moments[{k!r}][0]", moments[k][0], self.params[k])
                self._check_like(f"moments[{k!r}][1]", moments[k][1], self.params[k])
        except Exception:
            self.params, self.G, self.device = old
            raise
        self._moments = {k: (moments[k][0], moments[k][1]) for k in order}

    def zero_moments(self, field: str):
        if field not in self._moments:
            raise ValueError(f"zero_moments: unknown field {field!r} (one of {tuple(self.params)})")
        for m in self._moments[field]:
            m.zero_()

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params.values():
            if set_to_none or p.grad is None:
                p.grad = None
            else:
                p.grad.zero_()

    # ---- the step --------------------------------------------------------------------------------------------------------------------------
    def _visibility(self, visible):
        """(radii, V, R, mask) of siu3r_gaussian_adam"""
        if visible is None:
            return None, 0, 0, None
        if not isinstance(visible, torch.Tensor):
            raise TypeError(f"visible must be a tensor or None, got {type(visible).__name__}")
        _gpu(visible)
        if visible.device != self.device or not visible.is_contiguous():
            raise ValueError(f"visible must be contiguous and on {self.device}, got {'a' if visible.is_contiguous() else 'a non-contiguous'} tensor on {visible.device}")
        if visible.dtype == torch.int32:
            if visible.dim() != 3 or visible.shape[1] != self.G or visible.shape[0] == 0 or visible.shape[2] == 0:
                raise ValueError(f"visible (int32 radii) must be [V, {self.G}, R], got {tuple(visible.shape)}")
            return visible, int(visible.shape[0]), int(visible.shape[2]), None
        if visible.dtype in (torch.bool, torch.uint8):
            if tuple(visible.shape) != (self.G,):
                raise ValueError(f"visible (mask) must be [{self.G}], got {tuple(visible.shape)}")
            return None, 0, 0, visible.view(torch.uint8)
        raise ValueError(f"visible must be int32 radii [V,G,R] or a bool / uint8 mask [G], got {visible.dtype}")

    def step(self, visible: Optional[torch.Tensor] = None, lrs: Optional[Dict[str, float]] = None):
        """One Adam step of every field from its `.grad`.  visible: the render's int32 radii [V,G,R] (a Gaussian is visible iff any entry is
        > 0), a bool / uint8 mask [G], or None (all visible); an invisible Gaussian keeps the bits of its parameters and moments, and its
        gradient is not read.  lrs: per-field rates for THIS step only (a schedule's value)."""
        rates = self._rates(lrs, self.lrs)
        radii, V, R, mask = self._visibility(visible)
        table = (_lib.AdamField * len(self.params))()
        for i, (k, p) in enumerate(self.params.items()):
            if p.grad is None:
                raise RuntimeError(f"GaussianAdam.step: field {k!r} has no gradient (backward did not reach it)")
            self._check_like(f"{k}.grad", p.grad, p)
            m, v = self._moments[k]
            sh = k == SH_FIELD
            table[i] = _lib.AdamField(_p(p), _p(p.grad), _p(m), _p(v), p.numel() // self.G, p.shape[-1] if sh else 0, rates[k],
                                      rates[k] * self.sh_rest_lr_scale if sh else rates[k])
        lib = _lib.lib()
        if radii is not None and (self._ws is None or self._ws.numel() < self.G or self._ws.device != self.device):
            self._ws = torch.empty(int(lib.siu3r_gaussian_adam_ws(self.G)), dtype=torch.uint8, device=self.device)
        t = self.step_count + 1
        b1, b2 = self.betas
        with torch.cuda.device(self.device):
            check(lib.siu3r_gaussian_adam(table, len(self.params), self.G, b1, b2, self.eps, 1.0 - b1 ** t, 1.0 - b2 ** t, _p(radii), V, R, _p(mask),
                                          _p(self._ws) if radii is not None else None, _stream()))
        self.step_count = t


class TorchAdam:
    """torch.optim.Adam (fused, one parameter group per field) behind the part of GaussianAdam's surface that refine.refine_gaussians uses, so
    that the loop never sees torch's optimiser-state format.  It steps every row at its constant rate: no visibility, no schedule."""

    def __init__(self, params: Dict[str, torch.Tensor], lrs: Dict[str, float], eps: float = 1e-15):
        self.lrs, self.eps = {k: lrs[k] for k in params}, eps
        self._bind(params)

    def _bind(self, params):
        self.params = dict(params)
        self._opt = torch.optim.Adam([{"params": [p], "lr": self.lrs[k]} for k, p in self.params.items()], eps=self.eps, fused=True)

    @property
    def moments(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """{field: (exp_avg, exp_avg_sq)} of the optimiser's state (there from the first step on)"""
        state = {k: self._opt.state[p] for k, p in self.params.items()}
        return {k: (state[k]["exp_avg"], state[k]["exp_avg_sq"]) for k in state}

    def rebind(self, params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]]):
        """a new torch.optim.Adam on the new leaves after a density event, with each field's step count (fused Adam: a device tensor per
        parameter) and the given moments as its state"""
        steps = {k: self._opt.state[p]["step"] for k, p in self.params.items()}
        self._bind({k: params[k] for k in self.params})
        for k, p in self.params.items():
            self._opt.state[p] = {"step": steps[k], "exp_avg": moments[k][0], "exp_avg_sq": moments[k][1]}

    def zero_moments(self, field: str):
        state = self._opt.state[self.params[field]]
        for m in ("exp_avg", "exp_avg_sq"):
            if m in state:  # (before the first step there is nothing to zero)
                state[m].zero_()

    def zero_grad(self, set_to_none: bool = True):
        self._opt.zero_grad(set_to_none=set_to_none)

    def step(self, visible=None, lrs=None):
        if visible is not None or lrs is not None:
            raise ValueError("TorchAdam.step takes neither `visible` nor `lrs`: only GaussianAdam implements them")
        self._opt.step()
