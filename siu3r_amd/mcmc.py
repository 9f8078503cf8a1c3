"""MCMC densification of per-scene refinement (Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo"; the
MCMCStrategy of gsplat) on top of csrc/mcmc.hip: the set has a fixed budget of rows (`cap_max`), nothing is ever deleted and reallocated.
At an event the dead Gaussians (opacity <= min_opacity) are RELOCATED onto live ones drawn in proportion to their opacity, with an
opacity / scale correction that leaves the render nearly unchanged, and the set GROWS by a fixed share up to the cap, the new rows again
being corrected copies of drawn ones.  Every iteration a regulariser pulls opacities and scales down (so that unused Gaussians die) and
covariance-shaped noise moves the means of the transparent ones.  No gradient statistics are needed.

The draws are integer arithmetic on 24-bit weights and the caller's random words: a pure function of both.

Everything here works on the UNCONSTRAINED parameters refine.refine_gaussians optimises, as density.py does: means [G,3], "scales" =
log-scales [G,3], "rotations" = raw (x, y, z, w) quaternions [G,4], "opacities" = logit opacities [G], harmonics [G,3,n]."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .density import FIELDS, _check_params, _f32, _rows, event_iterations
from .ops import _gpu, _p, _stream

GATE_OPACITY = 0.005  # the noise gate's centre: gsplat's op_sigmoid(1 - o, k = 100, x0 = 0.995)
N_MAX = 51            # the relocation update's largest N = count + 1
W_ONE = 1 << 24       # the sampling weight of opacity 1


@dataclass
class MCMCControl:
    """When and how refine.refine_gaussians relocates and grows the set.  cap_max: the budget of rows, never exceeded (and not below the
    starting count).  grow_factor, min_opacity, noise_lr, opacity_reg and scale_reg are gsplat's MCMCStrategy defaults; the schedule
    (start, every, stop) follows density.DensityControl: an event at iteration i runs BEFORE the render of iteration i, stop = None means
    iters - every, iteration 0 is never an event.  seed: of the generator that draws the random words and the noise."""
    cap_max: int
    grow_factor: float = 1.05
    min_opacity: float = 0.005
    noise_lr: float = 5e5
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    start: int = 100
    every: int = 100
    stop: Optional[int] = None
    seed: int = 0

    def validate(self, G: Optional[int] = None):
        """host-side validation, before any device work: ValueError for a field that is not finite, negative, or out of its range, and for
        a cap below the row count G"""
        if isinstance(self.cap_max, bool) or not isinstance(self.cap_max, int) or self.cap_max <= 0:
            raise ValueError(f"MCMCControl.cap_max must be a positive int, got {self.cap_max!r}")
        for name in ("grow_factor", "min_opacity", "noise_lr", "opacity_reg", "scale_reg"):
            v = float(getattr(self, name))
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"MCMCControl.{name} must be finite and >= 0, got {getattr(self, name)!r}")
        if float(self.grow_factor) < 1.0:
            raise ValueError(f"MCMCControl.grow_factor must be >= 1, got {self.grow_factor!r}")
        if not 0.0 < float(self.min_opacity) < 1.0:
            raise ValueError(f"MCMCControl.min_opacity must lie inside (0, 1), got {self.min_opacity!r}")
        self.events(0)  # (every <= 0 raises there)
        if int(self.start) < 0 or (self.stop is not None and int(self.stop) < 0):
            raise ValueError(f"MCMCControl.start / stop must be >= 0, got {self.start!r} / {self.stop!r}")
        if G is not None and self.cap_max < int(G):
            raise ValueError(f"MCMCControl.cap_max = {self.cap_max} is below the {int(G)} Gaussians the run starts from (nothing is ever deleted)")

    def events(self, iters: int) -> List[int]:
        """the iterations of a run of `iters` iterations that relocate and grow: the schedule of density.event_iterations"""
        return event_iterations(self.start, self.every, self.stop, iters, "MCMCControl")

    def n_new(self, G: int) -> int:
        """how many rows an event adds to G: up to int(grow_factor * G), never past cap_max"""
        return max(0, min(int(self.cap_max), int(float(self.grow_factor) * int(G))) - int(G))

    @property
    def logit_min_opacity(self) -> float:
        """the float32 number the kernel compares the logit opacities against (computed once, on the host)"""
        return _f32(math.log(float(self.min_opacity) / (1.0 - float(self.min_opacity))))


# ---- the kernels, one wrapper each ---------------------------------------------------------------------------------------------------------
def _ints(t: torch.Tensor, n: int, dtype, name: str) -> torch.Tensor:
    if tuple(t.shape) != (n,) or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor [{n}], got {tuple(t.shape)} {t.dtype}")
    return t


def _ws(G: int, device) -> torch.Tensor:
    return torch.empty(max(int(_lib.lib().siu3r_mcmc_ws(G)) // 8, 1), dtype=torch.int64, device=device)


def weights(logit_opacity: torch.Tensor, logit_min_opacity: float, relocate: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """siu3r_mcmc_weights -> (w [G] int32 = rint(sigmoid(a) 2^24), dead [G] bool = a <= logit_min_opacity); relocate=True gives the dead
    rows the weight 0"""
    _gpu(logit_opacity)
    G = logit_opacity.shape[0]
    _rows(logit_opacity, G, "logit_opacity")
    if logit_opacity.dim() != 1 or G == 0:
        raise ValueError(f"logit_opacity must be [G] with G > 0, got {tuple(logit_opacity.shape)}")
    w = torch.empty(G, dtype=torch.int32, device=logit_opacity.device)
    dead = torch.empty(G, dtype=torch.uint8, device=logit_opacity.device)
    check(_lib.lib().siu3r_mcmc_weights(_p(logit_opacity), G, float(logit_min_opacity), int(bool(relocate)), _p(w), _p(dead), _stream()))
    return w, dead.view(torch.bool)


def scan(w: torch.Tensor, dead: Optional[torch.Tensor] = None):
    """siu3r_mcmc_scan -> (cum [G] int64: the inclusive scan of w, dead_idx [G] int32: the dead rows in memory order in its first n_dead
    entries, n_dead [1] int32), all on the device; without `dead` the last two are None"""
    _gpu(w, dead)
    G = w.shape[0]
    if G == 0:
        raise ValueError("scan: no rows")
    _ints(w, G, torch.int32, "w")
    cum = torch.empty(G, dtype=torch.int64, device=w.device)
    dead_idx = n_dead = None
    if dead is not None:
        _ints(dead, G, torch.bool, "dead")
        dead_idx = torch.empty(G, dtype=torch.int32, device=w.device)
        n_dead = torch.empty(1, dtype=torch.int32, device=w.device)
    check(_lib.lib().siu3r_mcmc_scan(_p(w), _p(dead), G, _p(cum), _p(dead_idx), _p(n_dead), _p(_ws(G, w.device)), _stream()))
    return cum, dead_idx, n_dead


def sample(cum: torch.Tensor, rbits: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """siu3r_mcmc_sample: rbits [n] int64 random words in [0, 2^32) -> (sampled [n] int32: the smallest g with cum[g] > (rbits * total) >> 32,
    count [G] int32); a total of 0 makes every draw row 0"""
    _gpu(cum, rbits)
    G, n = cum.shape[0], rbits.shape[0]
    _ints(cum, G, torch.int64, "cum"), _ints(rbits, n, torch.int64, "rbits")
    if G == 0:
        raise ValueError("sample: no rows")
    sampled = torch.empty(n, dtype=torch.int32, device=cum.device)
    count = torch.empty(G, dtype=torch.int32, device=cum.device)
    check(_lib.lib().siu3r_mcmc_sample(_p(cum), G, _p(rbits), n, _p(sampled), _p(count), _stream()))
    return sampled, count


def relocation_update(log_scales: torch.Tensor, logit_opacity: torch.Tensor, count: torch.Tensor, min_opacity: float):
    """siu3r_mcmc_relocate, in place: the opacity / scale correction of every row with count > 0 (drawn count times)"""
    _gpu(log_scales, logit_opacity, count)
    G = logit_opacity.shape[0]
    _rows(log_scales, G, "log_scales"), _rows(logit_opacity, G, "logit_opacity"), _ints(count, G, torch.int32, "count")
    if tuple(log_scales.shape) != (G, 3) or G == 0:
        raise ValueError(f"log_scales must be [G, 3] with G > 0, got {tuple(log_scales.shape)}")
    check(_lib.lib().siu3r_mcmc_relocate(_p(log_scales), _p(logit_opacity), _p(count), G, float(min_opacity), _stream()))


def copy_rows(field: torch.Tensor, moments: Optional[Tuple[torch.Tensor, torch.Tensor]], src: torch.Tensor, dst: Optional[torch.Tensor] = None,
              G0: int = 0):
    """siu3r_mcmc_copy_rows, in place: field[dst[j]] = field[src[j]] (dst None: row G0 + j); rows dst[j] and src[j] of both moments become
    zero.  src / dst: int32 [n]; sources and destinations must be disjoint."""
    _gpu(field, src, dst)
    rows, n = field.shape[0], src.shape[0]
    _rows(field, rows, "field"), _ints(src, n, torch.int32, "src")
    if rows == 0:
        raise ValueError("copy_rows: an empty field")
    if dst is not None:
        _ints(dst, n, torch.int32, "dst")
    elif not 0 <= int(G0) <= rows - n:
        raise ValueError(f"copy_rows: rows {G0} .. {int(G0) + n} lie outside the field's {rows}")
    if moments is not None:
        for m in moments:
            _gpu(m)
            if m.shape != field.shape or m.dtype != torch.float32 or not m.is_contiguous():
                raise ValueError(f"copy_rows: a moment must be a contiguous float32 tensor {tuple(field.shape)}, got {tuple(m.shape)} {m.dtype}")
    check(_lib.lib().siu3r_mcmc_copy_rows(_p(field), _p(moments[0]) if moments else None, _p(moments[1]) if moments else None, field[0].numel(), rows,
                                          _p(src), _p(dst), int(G0), n, _stream()))


def inject_noise(means: torch.Tensor, log_scales: torch.Tensor, quats: torch.Tensor, logit_opacity: torch.Tensor, scaler: float, noise: torch.Tensor):
    """siu3r_mcmc_noise, in place on means: means += Sigma (noise * gate * scaler) with Sigma = R(q / |q|) diag(exp(2 s)) R^T and
    gate = 1 / (1 + exp(-100 (0.005 - sigmoid(logit_opacity)))): opaque Gaussians stay, transparent ones explore.  noise [G,3]: unit normals."""
    _gpu(means, log_scales, quats, logit_opacity, noise)
    G = means.shape[0]
    for name, t, shape in (("means", means, (G, 3)), ("log_scales", log_scales, (G, 3)), ("quats", quats, (G, 4)), ("logit_opacity", logit_opacity, (G,)),
                           ("noise", noise, (G, 3))):
        if tuple(t.shape) != shape or G == 0:
            raise ValueError(f"{name} must be {list(shape)} with G > 0, got {tuple(t.shape)}")
        _rows(t, G, name)
    if not math.isfinite(float(scaler)):
        raise ValueError(f"scaler must be finite, got {scaler!r}")
    check(_lib.lib().siu3r_mcmc_noise(_p(means), _p(log_scales), _p(quats), _p(logit_opacity), _p(noise), G, GATE_OPACITY, float(scaler), _stream()))


def regularize(logit_opacity: torch.Tensor, log_scales: torch.Tensor, opacity_reg: float, scale_reg: float, grad_opacity: Optional[torch.Tensor] = None,
               grad_scales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """siu3r_mcmc_regularize: adds the gradient of opacity_reg * mean(sigmoid(logit_opacity)) into grad_opacity [G] and that of
    scale_reg * mean(exp(log_scales)) into grad_scales [G,3] (None: that field is frozen) -> the two values, [2] float32 on the device"""
    _gpu(logit_opacity, log_scales, grad_opacity, grad_scales)
    G = logit_opacity.shape[0]
    if tuple(logit_opacity.shape) != (G,) or tuple(log_scales.shape) != (G, 3) or G == 0:
        raise ValueError(f"logit_opacity must be [G] and log_scales [G, 3] with G > 0, got {tuple(logit_opacity.shape)} and {tuple(log_scales.shape)}")
    _rows(logit_opacity, G, "logit_opacity"), _rows(log_scales, G, "log_scales")
    for name, g, like in (("grad_opacity", grad_opacity, logit_opacity), ("grad_scales", grad_scales, log_scales)):
        if g is not None and (g.shape != like.shape or g.dtype != torch.float32 or not g.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 tensor {tuple(like.shape)}, got {tuple(g.shape)} {g.dtype}")
    for name, v in (("opacity_reg", opacity_reg), ("scale_reg", scale_reg)):
        if not math.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
    value = torch.empty(2, dtype=torch.float32, device=logit_opacity.device)
    check(_lib.lib().siu3r_mcmc_regularize(_p(logit_opacity), _p(log_scales), G, float(opacity_reg), float(scale_reg), _p(grad_opacity), _p(grad_scales),
                                           _p(_ws(G, logit_opacity.device)), _p(value), _stream()))
    return value


# ---- the two halves of an event, and the event -----------------------------------------------------------------------------------------------
def _words(n: int, control: MCMCControl, rbits, generator, device) -> torch.Tensor:
    """n random words in [0, 2^32) as int64: the first n of the caller's, or drawn from `generator` (None: one seeded by control.seed)"""
    if rbits is not None:
        if rbits.dim() != 1 or rbits.shape[0] < n or rbits.dtype != torch.int64:
            raise ValueError(f"rbits must be an int64 tensor of at least {n} words, got {tuple(rbits.shape)} {rbits.dtype}")
        return rbits[:n].contiguous()
    if generator is None:
        generator = torch.Generator(device=device).manual_seed(int(control.seed))
    return torch.randint(0, 1 << 32, (n,), generator=generator, device=device, dtype=torch.int64)


def relocate(params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]], control: MCMCControl,
             rbits: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> dict:
    """Moves every dead Gaussian (logit opacity <= logit(min_opacity)) onto a live one, IN PLACE.  params: the five FIELDS in unconstrained
    form, free or frozen alike; moments: {field: (exp_avg, exp_avg_sq)} of the fields Adam moves.  One draw per dead row, in proportion to
    the live rows' opacities; every drawn row gets the relocation update (as if split into count + 1 equal parts), the dead rows become
    copies of the updated rows, and the Adam moments of both become zero.  rbits: at least n_dead int64 random words in [0, 2^32), of
    which the first n_dead are used (None: drawn from `generator`, or from one seeded by control.seed).
    ONE host read, the number of dead rows; none dead: nothing happens; all dead: RuntimeError.  -> {"rows_in", "rows_out", "relocated"}."""
    control.validate()
    G = _check_params(params, moments)
    w, dead = weights(params["opacities"], control.logit_min_opacity, relocate=True)
    cum, dead_idx, n_dead = scan(w, dead)
    n = int(n_dead)
    if n == G:
        raise RuntimeError(f"MCMC relocation: all {G} Gaussians are dead (opacity <= {control.min_opacity}): there is nothing to relocate onto")
    if n > 0:
        sampled, count = sample(cum, _words(n, control, rbits, generator, w.device))
        relocation_update(params["scales"], params["opacities"], count, control.min_opacity)
        for k in FIELDS:
            copy_rows(params[k], moments.get(k), sampled, dead_idx[:n])
    return dict(rows_in=G, rows_out=G, relocated=n)


def grow(params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]], control: MCMCControl,
         rbits: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
    """Adds control.n_new(G) rows (known on the host: no read): as many draws in proportion to the opacities of ALL rows, the relocation
    update on the drawn rows (in place on `params`), and the new rows G .. G + n_new - 1 are copies of the updated ones with zero moments
    (the drawn rows' moments become zero too).  -> (new params, new moments, {"rows_in", "rows_out", "added"}); nothing to add returns the
    inputs themselves."""
    control.validate()
    G = _check_params(params, moments)
    n = control.n_new(G)
    info = dict(rows_in=G, rows_out=G + n, added=n)
    if n == 0:
        return params, moments, info
    w, _ = weights(params["opacities"], control.logit_min_opacity, relocate=False)
    cum, _, _ = scan(w)
    sampled, count = sample(cum, _words(n, control, rbits, generator, w.device))
    relocation_update(params["scales"], params["opacities"], count, control.min_opacity)
    new_p, new_m = {}, {}

    def grown(t):
        out = torch.empty((G + n, *t.shape[1:]), dtype=torch.float32, device=t.device)
        out[:G].copy_(t)
        return out

    for k in FIELDS:
        new_p[k] = grown(params[k])
        if k in moments:
            new_m[k] = (grown(moments[k][0]), grown(moments[k][1]))
        copy_rows(new_p[k], new_m.get(k), sampled, None, G0=G)
    return new_p, new_m, info


def event(params: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]], control: MCMCControl,
          rbits: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
    """One MCMC event, in density.densify_and_prune's return shape: relocate (in place on `params`), then grow.  The random words are those
    of relocate followed by those of grow: of `rbits` the first n_dead and the next n_new, else drawn in that order from `generator` (None:
    each half seeds its own).  -> (new params, new moments, {"rows_in", "rows_out", "relocated", "added"}); nothing to add: the inputs."""
    moved = relocate(params, moments, control, rbits, generator)
    new_p, new_m, info = grow(params, moments, control, None if rbits is None else rbits[moved["relocated"]:], generator)
    return new_p, new_m, dict(info, relocated=moved["relocated"])
