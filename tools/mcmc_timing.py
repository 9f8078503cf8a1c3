"""Time MCMC densification (siu3r_amd/mcmc.py, csrc/mcmc.hip) against the same steps written in torch ops on the GPU
(float32; torch.multinomial for the draw):
  per iteration   mcmc.inject_noise + mcmc.regularize, device events around blocks of steps, the candidates alternating so that a drift of
                  the board hits both; the time per step is the median over the blocks;
  per event       mcmc.relocate + mcmc.grow on a fresh copy of a set with `--dead` dead rows (the copy is not timed; the event's one host
                  read is), one event per block, the median over the blocks.
Needs a GPU; writes one JSON file.

    python tools/mcmc_timing.py --out profiles/mcmc_timing.json [--gaussians 1000000] [--sh 16]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("means", "scales", "rotations", "opacities", "harmonics")
N_MAX = 51


def board_uuid():
    uuid = getattr(torch.cuda.get_device_properties(0), "uuid", None)
    if uuid is not None:
        return str(uuid)
    try:
        out = subprocess.run(["rocm-smi", "--showuniqueid"], capture_output=True, text=True, timeout=60).stdout
        ids = [l.split(":")[-1].strip() for l in out.splitlines() if "Unique ID" in l]
        return ids[0] if ids else "unknown"
    except Exception:
        return "unknown"


# ---- the same steps in torch ops (float32) ---------------------------------------------------------------------------------------------
def torch_noise(means, log_scales, quats, logit_opacity, scaler, noise):
    o = torch.sigmoid(logit_opacity)
    gate = 1.0 / (1.0 + torch.exp(-100.0 * (0.005 - o)))
    q = quats / quats.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).view(-1, 3, 3)
    v = noise * (gate * scaler)[:, None]
    # (3 x 3 products as broadcast multiplies: written with torch.einsum, a batched GEMM over a million 3 x 3 matrices, this step took 21 ms)
    u = torch.exp(2.0 * log_scales) * (R * v[:, :, None]).sum(1)
    means.add_((R * u[:, None, :]).sum(2))


def torch_regularize(logit_opacity, log_scales, lam_o, lam_s, grad_o, grad_s):
    G = logit_opacity.shape[0]
    o = torch.sigmoid(logit_opacity)
    e = torch.exp(log_scales)
    grad_o.add_(o * (1.0 - o), alpha=lam_o / G)
    grad_s.add_(e, alpha=lam_s / (3 * G))
    return torch.stack((lam_o * o.mean(), lam_s * e.mean()))


def _torch_update(p, idx, count, binom, min_opacity):
    """the relocation update of the drawn rows `idx` (unique), float32, the inner index summed by the hockey-stick identity"""
    N = (count[idx] + 1).clamp(max=N_MAX)
    o = torch.sigmoid(p["opacities"][idx])
    o_new = 1.0 - torch.pow(1.0 - o, 1.0 / N.float())
    k = torch.arange(N_MAX, device=o.device)
    terms = binom[N] * torch.pow(o_new[:, None], (k + 1).float()) / torch.sqrt((k + 1).float()) * (1.0 - 2.0 * (k % 2).float())
    denom = torch.where(k[None, :] < N[:, None], terms, torch.zeros_like(terms)).sum(-1)
    p["scales"][idx] += torch.log(o / denom)[:, None]
    p["opacities"][idx] = torch.logit(o_new.clamp(min_opacity, 1.0 - 1.1920929e-07))


def torch_event(p, m, n_new, binom, min_opacity, logit_min):
    """relocate + grow in torch ops -> (new params, new moments)"""
    G = p["opacities"].shape[0]
    dead = p["opacities"] <= logit_min
    dead_idx = torch.nonzero(dead).flatten()  # (the host read: the number of dead rows)
    if dead_idx.numel() > 0:
        probs = torch.where(dead, torch.zeros_like(p["opacities"]), torch.sigmoid(p["opacities"]))
        sampled = torch.multinomial(probs, dead_idx.numel(), replacement=True)
        count = torch.bincount(sampled, minlength=G)
        _torch_update(p, torch.nonzero(count).flatten(), count, binom, min_opacity)
        for k in FIELDS:
            p[k][dead_idx] = p[k][sampled]
            for t in m[k]:
                t[dead_idx] = 0
                t[sampled] = 0
    sampled = torch.multinomial(torch.sigmoid(p["opacities"]), n_new, replacement=True)
    count = torch.bincount(sampled, minlength=G)
    _torch_update(p, torch.nonzero(count).flatten(), count, binom, min_opacity)
    new_p, new_m = {}, {}
    for k in FIELDS:
        new_p[k] = torch.cat((p[k], p[k][sampled]))
        for t in m[k]:
            t[sampled] = 0
        new_m[k] = tuple(torch.cat((t, torch.zeros((n_new, *t.shape[1:]), device=t.device))) for t in m[k])
    return new_p, new_m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=16)
    ap.add_argument("--dead", type=int, default=10_000, help="dead rows of the timed event")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20, help="iterations per timed block")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_timing needs a GPU: a CPU run says nothing about it")
    from siu3r_amd import mcmc

    G, dev = a.gaussians, "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=gen, device=dev)
    base = dict(means=rnd(G, 3), scales=torch.log(0.01 + 0.1 * torch.rand((G, 3), generator=gen, device=dev)), rotations=rnd(G, 4),
                opacities=torch.logit(0.01 + 0.98 * torch.rand(G, generator=gen, device=dev)), harmonics=rnd(G, 3, a.sh))
    base["opacities"][torch.randperm(G, generator=gen, device=dev)[:a.dead]] = -9.0
    base_m = {k: (rnd(*v.shape) * 1e-3, torch.rand(v.shape, generator=gen, device=dev) * 1e-6) for k, v in base.items()}
    control = mcmc.MCMCControl(cap_max=2 * G)
    n_new = control.n_new(G)
    binom = torch.tensor([[math.comb(n, k + 1) for k in range(N_MAX)] for n in range(N_MAX + 1)], dtype=torch.float32, device=dev)

    # ---- per iteration: noise + regulariser ----
    noise = rnd(G, 3)
    scaler = control.noise_lr * 1.6e-4
    state = {name: dict(means=base["means"].clone(), grad_o=torch.zeros(G, device=dev), grad_s=torch.zeros(G, 3, device=dev)) for name in ("hip", "torch")}

    def hip_step():
        s = state["hip"]
        mcmc.regularize(base["opacities"], base["scales"], control.opacity_reg, control.scale_reg, s["grad_o"], s["grad_s"])
        mcmc.inject_noise(s["means"], base["scales"], base["rotations"], base["opacities"], scaler, noise)

    def torch_step():
        s = state["torch"]
        torch_regularize(base["opacities"], base["scales"], control.opacity_reg, control.scale_reg, s["grad_o"], s["grad_s"])
        torch_noise(s["means"], base["scales"], base["rotations"], base["opacities"], scaler, noise)

    steps = {"hip_noise_regularize": hip_step, "torch_noise_regularize": torch_step}
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(a.blocks):
        for name, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)

    # ---- per event: relocate + grow on a fresh copy ----
    fresh = lambda: ({k: v.clone() for k, v in base.items()}, {k: (v[0].clone(), v[1].clone()) for k, v in base_m.items()})
    rows = {}

    def hip_event(p, m):
        info = mcmc.relocate(p, m, control, generator=gen)
        new_p, _, grown = mcmc.grow(p, m, control, generator=gen)
        rows["hip"] = (info["relocated"], grown["added"], new_p["means"].shape[0])

    def torch_ev(p, m):
        new_p, _ = torch_event(p, m, n_new, binom, control.min_opacity, control.logit_min_opacity)
        rows["torch"] = new_p["means"].shape[0]

    events = {"hip_relocate_grow": hip_event, "torch_relocate_grow": torch_ev}
    for name, fn in events.items():
        times[name] = []
    for block in range(a.blocks + 2):  # (two warm-up events each)
        for name, fn in events.items():
            p, m = fresh()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(p, m)
            e1.record()
            e1.synchronize()
            if block >= 2:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert rows["hip"] == (a.dead, n_new, G + n_new) and rows["torch"] == G + n_new, rows

    result = {"gaussians": G, "sh_coefficients": a.sh, "dead_rows": a.dead, "rows_added": n_new, "steps_per_block": a.steps, "blocks": a.blocks,
              "warmup_steps": a.warmup, "device": torch.cuda.get_device_name(0), "board_uuid": board_uuid(), "torch": torch.__version__, "candidates": {}}
    for name, ts in times.items():
        us = statistics.median(ts)
        unit = "step" if name in steps else "event"
        result["candidates"][name] = {f"us_per_{unit}_median": us, f"us_per_{unit}_min": min(ts), f"us_per_{unit}_max": max(ts)}
        print(f"{name:>24}: {us:10.1f} us / {unit} (min {min(ts):.1f}, max {max(ts):.1f})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": a.out, "board_uuid": result["board_uuid"]}))


if __name__ == "__main__":
    main()
