"""Dense restatement of MCMC densification (Kheradmand et al. 2024; gsplat's MCMCStrategy) from the rules, not from csrc/mcmc.hip: the
sampling weights and the relocation update in float64 / Python floats, the multinomial draw in Python integers, the noise and the
regulariser in plain torch (float64 by default; `dtype=torch.float32` gives the same restatement in float32, the yardstick of the float32
error bars).  Runs on any device."""
import bisect
import itertools
import math

import torch

from dense_density64 import rotation

W_ONE = 1 << 24                 # the weight of opacity 1
N_MAX = 51                      # the largest N = count + 1 of the relocation update
O_MAX = 1.0 - 1.1920929e-07
GATE_OPACITY = 0.005            # op_sigmoid(1 - o, k = 100, x0 = 0.995)


def f32(x):
    """x rounded to float32, as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


# ---- (a) weights ------------------------------------------------------------------------------------------------------------------------
def weights(logit_opacity, logit_min_opacity, relocate):
    """logit_opacity [G] float32 -> (w [G] int64 = rint(sigmoid(a) 2^24) with the sigmoid in float64, dead [G] bool = a <= the threshold
    as float32 numbers); relocate: the dead rows get w = 0"""
    a = logit_opacity.float()
    o = 1.0 / (1.0 + torch.exp(-a.double()))
    w = torch.round(o * W_ONE).long()  # (torch.round rounds halves to even, as rint does)
    dead = a <= torch.tensor(logit_min_opacity, dtype=torch.float64).float()
    if relocate:
        w = torch.where(dead, torch.zeros_like(w), w)
    return w, dead


# ---- (b), (c) the integer sampler ---------------------------------------------------------------------------------------------------------
def scan(w):
    """the inclusive scan of integer weights (int64 is exact: G <= 2^30 weights of at most 2^24)"""
    return torch.cumsum(w.long(), 0)


def multinomial(w, rbits):
    """w: integer weights, rbits: random words in [0, 2^32); in Python integers: t = (r * total) >> 32, the draw is the smallest g with
    cum[g] > t (row 0 when no row has a weight) -> (sampled: list, count: list)"""
    cum = list(itertools.accumulate(int(v) for v in w))
    total = cum[-1]
    sampled, count = [], [0] * len(cum)
    for r in rbits:
        r = int(r)
        assert 0 <= r < (1 << 32)
        g = bisect.bisect_right(cum, (r * total) >> 32) if total > 0 else 0
        sampled.append(g)
        count[g] += 1
    return sampled, count


def dead_list(dead):
    """the indices of the dead rows in memory order"""
    return [g for g, d in enumerate(dead.tolist()) if d]


# ---- (d) the relocation update ------------------------------------------------------------------------------------------------------------
def denominator(o_new, N):
    """sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1), written as the double sum it is; the binomials are exact
    integers, the terms are summed without intermediate rounding (math.fsum)"""
    terms = []
    for i in range(1, N + 1):
        for k in range(i):
            terms.append(math.comb(i - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1))
    return math.fsum(terms)


def denominator_hockey_stick(o_new, N):
    """the same number with the sum over i done first: sum_i C(i-1, k) = C(N, k+1)"""
    return math.fsum(math.comb(N, k + 1) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1) for k in range(N))


def relocated_row(a, s, count, min_opacity, denom=denominator):
    """one row: a (logit opacity), s (three log-scales), drawn `count` >= 0 times -> (new a, new s), Python floats (float64)"""
    N = min(int(count) + 1, N_MAX)
    o = 1.0 / (1.0 + math.exp(-a))
    o_new = 1.0 - (1.0 - o) ** (1.0 / N)
    shift = math.log(o / denom(o_new, N))
    oc = min(max(o_new, min_opacity), O_MAX)  # the clamp comes after the denominator, as in gsplat
    return math.log(oc / (1.0 - oc)), [v + shift for v in s]


def relocation(logit_opacity, log_scales, count, min_opacity):
    """[G] / [G,3] float32 and integer counts -> float64 tensors (a, s); rows with count == 0 are the inputs upcast"""
    a, s = logit_opacity.double().clone(), log_scales.double().clone()
    for g, c in enumerate(count.tolist()):
        if c > 0:
            na, ns = relocated_row(float(a[g]), s[g].tolist(), c, min_opacity)
            a[g] = na
            s[g] = torch.tensor(ns, dtype=torch.float64)
    return a, s


# ---- (e) the row copy ---------------------------------------------------------------------------------------------------------------------
def copy_rows(field, moments, src, dst=None, G0=0):
    """field[dst[j]] = field[src[j]] (dst None: row G0 + j); rows dst[j] and src[j] of both moments become zero -> new tensors"""
    src = torch.as_tensor(src).long()
    dst = G0 + torch.arange(src.shape[0]) if dst is None else torch.as_tensor(dst).long()
    out = field.clone()
    out[dst] = field[src]
    ms = None
    if moments is not None:
        ms = tuple(m.clone() for m in moments)
        for m in ms:
            m[dst] = 0
            m[src] = 0
    return out, ms


# ---- (f) noise, (g) regulariser -----------------------------------------------------------------------------------------------------------
def noise(means, log_scales, quats_xyzw, logit_opacity, unit_normals, scaler, gate_opacity=GATE_OPACITY, dtype=torch.float64):
    """-> (means + Sigma (noise * gate * scaler), that displacement) in `dtype`; gate = 1 / (1 + exp(-100 (gate_opacity - o))),
    Sigma = R(q / |q|) diag(exp(2 s)) R^T"""
    t = lambda x: torch.as_tensor(x, dtype=torch.float64).to(dtype)
    o = 1.0 / (1.0 + torch.exp(-t(logit_opacity)))
    gate = 1.0 / (1.0 + torch.exp(-100.0 * (t(gate_opacity) - o)))
    R = rotation(t(quats_xyzw))
    sigma = R @ torch.diag_embed(torch.exp(2.0 * t(log_scales))) @ R.transpose(-1, -2)
    delta = torch.einsum("gij,gj->gi", sigma, t(unit_normals) * (gate * t(scaler))[:, None])
    return t(means) + delta, delta


def regularize(logit_opacity, log_scales, opacity_reg, scale_reg, grad_opacity=None, grad_scales=None, dtype=torch.float64):
    """-> (grad_opacity + opacity_reg o (1 - o) / G, grad_scales + scale_reg exp(s) / (3 G), (opacity_reg mean o, scale_reg mean exp(s))
    [2]) in `dtype`; a gradient that is None stays None"""
    t = lambda x: torch.as_tensor(x, dtype=torch.float64).to(dtype)
    G = logit_opacity.shape[0]
    o = 1.0 / (1.0 + torch.exp(-t(logit_opacity)))
    e = torch.exp(t(log_scales))
    ga = None if grad_opacity is None else t(grad_opacity) + t(opacity_reg) * o * (1.0 - o) / G
    gs = None if grad_scales is None else t(grad_scales) + t(scale_reg) * e / (3 * G)
    return ga, gs, torch.stack((t(opacity_reg) * o.mean(), t(scale_reg) * e.mean()))
