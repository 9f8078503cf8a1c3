"""Time optim.GaussianAdam.step (csrc/gaussian_adam.hip) against torch.optim.Adam(fused=True).step on the same five Gaussian fields
(DESIGN.md section 12).  Device events around blocks of steps after a warm-up, the candidates alternating so that a drift of the board hits
all of them; the per-step time is the median over the blocks.  Bytes: the dense update moves 7 x 4 bytes per element (read p, g, m, v;
write p, m, v).  Needs a GPU; writes one JSON file.

    python tools/adam_step_timing.py --out profiles/adam_step_timing.json [--gaussians 1000000] [--sh 16]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = {"means": (3,), "scales": (3,), "rotations": (4,), "opacities": (), "harmonics": None}
LRS = {"means": 1.6e-4, "scales": 5e-3, "rotations": 1e-3, "opacities": 5e-2, "harmonics": 2.5e-3}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=16)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_timing needs a GPU: a CPU run says nothing about it")
    from siu3r_amd.optim import GaussianAdam

    G, dev = a.gaussians, "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = {k: (G, *(s if s is not None else (3, a.sh))) for k, s in FIELDS.items()}
    grads = {k: torch.randn(s, generator=gen, device=dev) * 1e-3 for k, s in shapes.items()}
    make = lambda: {k: torch.randn(s, generator=gen, device=dev).requires_grad_(True) for k, s in shapes.items()}
    elements = sum(g.numel() for g in grads.values())
    half = torch.rand(G, generator=gen, device=dev) < 0.5
    radii = torch.zeros((a.views, G, 2), dtype=torch.int32, device=dev)
    radii[0, :, 0] = half.to(torch.int32) * 5

    p_hip, p_torch = make(), make()
    for p in (p_hip, p_torch):
        for k in p:
            p[k].grad = grads[k]
    hip = GaussianAdam(p_hip, LRS, sh_rest_lr_scale=0.05)
    ref = torch.optim.Adam([{"params": [p_torch[k]], "lr": LRS[k]} for k in p_torch], eps=1e-15, fused=True)
    candidates = {
        "torch_fused_dense": ref.step,
        "hip_dense": hip.step,
        "hip_half_visible_mask": lambda: hip.step(visible=half),
        "hip_half_visible_radii": lambda: hip.step(visible=radii),
    }
    for _ in range(a.warmup):
        for fn in candidates.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in candidates}
    for _ in range(a.blocks):
        for name, fn in candidates.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    dense_bytes = 7 * 4 * elements
    result = {"gaussians": G, "sh_coefficients": a.sh, "elements": elements, "dense_bytes_per_step": dense_bytes, "views_of_radii": a.views,
              "visible_share": float(half.float().mean()), "steps_per_block": a.steps, "blocks": a.blocks, "warmup_steps": a.warmup,
              "device": torch.cuda.get_device_name(0), "board_uuid": board_uuid(), "torch": torch.__version__, "candidates": {}}
    for name, ts in times.items():
        us = statistics.median(ts)
        result["candidates"][name] = {"us_per_step_median": us, "us_per_step_min": min(ts), "us_per_step_max": max(ts),
                                      "dense_bytes_over_time_TBps": dense_bytes / (us * 1e-6) / 1e12}
        print(f"{name:>24}: {us:9.1f} us / step (min {min(ts):.1f}, max {max(ts):.1f}); 7 x 4 B x {elements} elements over that = "
              f"{dense_bytes / (us * 1e-6) / 1e12:.2f} TB/s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": a.out, "board_uuid": result["board_uuid"]}))


if __name__ == "__main__":
    main()
