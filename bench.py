#!/usr/bin/env python
"""SIU3R hot-path benchmark (driver contract: one JSON line on rank 0).

A "step" is one pass of the hot path (SIU3RModel.forward incl. the on-device panoptic post-process with a NON-EMPTY result and
the query-class-logit lifting inputs) over one batch of synthetic image pairs at 2 x 512 x 512 (BASELINE.json configs[1]: single
pair, ViT-L encoder/decoder + DPT 3DGS heads + ViT-Adapter/Mask2Former), with seeded synthetic weights of the reference
architecture (no checkpoint is available offline) and inputs already resident in HBM.  value = image-pairs/s over all ranks (weak
scaling: each rank runs its own pairs).

The timed mode is the one that meets the north-star parity bar (<= 1e-3 max-norm on the Gaussian fields against the fp32 oracle):
precision "bf16x3" = fp32 activations, bf16 MFMA with the hi/lo operand split (3 passes).

A plain run sets up, warms up, times `--steps` steps and prints the line.  Everything else it measures runs only with `--full`: the
plain-bf16 mode (bf16 operands, ~2e-2 .. 1e-1 on the fields, tests/test_model_gpu.py) timed the same way right after and reported as
`second_mode`, the `roofline` object of the dominant kernel, the render legs and the CPU baselines (the `--no-*` options drop single
ones of them).  `--dump-outputs DIR` writes what the timed path returned in its last step as DIR/<name>.npy (float32 / float64;
arrays above the size budget as a fixed, seeded sample; DIR/manifest.json says which), for comparing two builds output for output.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
"""
import argparse
import collections
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOPS_PER_PAIR_512 = 4059.0e9  # algorithmic 2*MAC of one pair @512^2 (torch flop counter on the reference)
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 peak, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0


def _latest_profile(suffix):
    """newest committed round of a counter summary (profiles/rNN_<suffix>)"""
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    return found[-1] if found else os.path.join(ROOT, "profiles", "r00_" + suffix)


PMC_FILE = _latest_profile("pmc_summary.json")
BUSY_FILE = _latest_profile("mfma_busy.json")
PMC_NAME = "profiles/" + os.path.basename(PMC_FILE)
# the exact statement tests/test_model_gpu.py::test_parity_sweep asserts on seven shapes / seeds (-m gpu, driver-run)
PARITY = {"bf16x3": "vs the pinned fp32 oracle, max-normalised: every Gaussian field <= 1e-3 (measured <= 8e-5); Mask2Former class / mask logits "
                    "<= 5e-3 (<= 1e-3 on most inputs; 1-3e-3 when a thresholded attention mask flips a borderline pixel between fp32 evaluation "
                    "orders); label maps agree >= 0.995; graph replay bit-identical to eager (tests/test_model_gpu.py::test_parity_sweep)",
          "bf16": "bf16 operand rounding: 2e-2 .. 1e-1 on the fields (covariances worst), label agreement 0.85-0.93"}


def _family(name):
    """source-level kernel of an instantiation: `ns::kernel<args>` -> `ns::kernel`"""
    return name.split("<")[0].strip()


def pmc_bytes(section, family):
    """HBM-side bytes per launch of one source-level kernel (all its template instantiations) from the committed counter passes
    (tools/pmc_cmd.sh: separate FETCH_SIZE / WRITE_SIZE runs, both in KiB; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for
    gfx950): sum over the instantiations / their launches."""
    if not os.path.exists(PMC_FILE):
        return None, None
    sec = json.load(open(PMC_FILE)).get(section)
    if not sec:
        return None, None
    rows = [e for n, e in sec.items() if _family(n) == family and "FETCH_SIZE" in e and "WRITE_SIZE" in e]
    launches = sum(e["FETCH_SIZE"]["launches"] for e in rows)
    if not launches:
        return None, None
    total = sum(2.0 * e["FETCH_SIZE"]["total"] + e["WRITE_SIZE"]["total"] for e in rows) * 1024.0
    return total / launches, f"{PMC_NAME}[{section}] (all instantiations of {family}: {launches} launches)"


def pmc_frame_bytes(section, views_per_call):
    """HBM-side bytes of one rendered frame: every kernel the profiled rasterizer command launched (project, sort passes, binning,
    composite, buffer clears), summed, over the frames it rendered (= composite launches x views per call)."""
    if not os.path.exists(PMC_FILE):
        return None, None
    sec = json.load(open(PMC_FILE)).get(section)
    if not sec:
        return None, None
    comp = [e for n, e in sec.items() if n.startswith("composite_rgb_kernel")]
    if not comp or "FETCH_SIZE" not in comp[0]:
        return None, None
    frames = sum(e["FETCH_SIZE"]["launches"] for e in comp) * views_per_call
    tot = sum(2.0 * e.get("FETCH_SIZE", {}).get("total", 0.0) + e.get("WRITE_SIZE", {}).get("total", 0.0) for e in sec.values()) * 1024.0
    return tot / frames, f"{PMC_NAME}[{section}] (all kernels of the command / {frames} frames)"


def timed_steps(run, steps, D, dev):
    """the contract's timed region: barrier + synchronize on both sides, max over ranks.  run(steps) does exactly `steps` steps and
    returns the last one's result."""
    torch.cuda.synchronize()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(steps)
    torch.cuda.synchronize()
    D.barrier()
    torch.cuda.synchronize()
    return D.max_over_ranks(time.perf_counter() - t0, device=dev), out


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _board_id() -> str:
    """UUID of the GPU this rank runs on (HIP device properties), for comparing runs: the same tree measured 52.3 / 54.6 / 56.0 pairs/s on three boards"""
    try:
        return str(torch.cuda.get_device_properties(torch.cuda.current_device()).uuid)
    except Exception:
        return "unknown"


DUMP_BYTES = 60 << 20  # --dump-outputs writes at most this much (the limit is 64 MB)


def dump_outputs(out, directory):
    """What the timed path returned in its last step, (gaussians, segmentation output, seg masks, segments_info, query scores), as
    DIR/<name>.npy: floating tensors as float32 (float64 stays float64), integer / bool tensors and the segment lists as float64.
    Every array keeps at most `cap` elements: larger ones are a sample at sorted indices drawn from a generator seeded with the crc32 of
    the name (the same indices in every run of the same shapes).  cap starts at 2^21 and halves until the whole dump fits DUMP_BYTES."""
    import zlib
    import numpy as np

    gauss, seg, masks, infos = out[:4]
    qs = out[4] if len(out) > 4 else None
    arrays = []  # (name, tensor or numpy array)
    for k, v in vars(gauss).items():
        if torch.is_tensor(v):
            arrays.append((f"gaussians_{k}", v))
        elif isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) for t in v):
            arrays += [(f"gaussians_{k}_{b}", t) for b, t in enumerate(v)]
    arrays += [(f"seg_{k}", v) for k, v in seg.items() if torch.is_tensor(v) and not k.startswith("_")]
    arrays += [(f"seg_masks_{b}", m) for b, m in enumerate(masks) if torch.is_tensor(m)]
    arrays += [(f"segments_{b}", np.array([[s["id"], s["label_id"], float(s["was_fused"]), s["score"]] for s in segs], dtype=np.float64).reshape(-1, 4))
               for b, segs in enumerate(infos)]
    if qs is not None:
        arrays += [(f"query_scores_{b}", q.detach().double().reshape(-1) if torch.is_tensor(q) else np.asarray(q, dtype=np.float64).reshape(-1))
                   for b, q in enumerate(qs)]

    def itemsize(v):
        is_f32 = (v.is_floating_point() and v.dtype != torch.float64) if torch.is_tensor(v) else v.dtype == np.float32
        return 4 if is_f32 else 8

    numel = lambda v: v.numel() if torch.is_tensor(v) else v.size
    cap = 1 << 21
    while cap > 1 and sum(min(numel(v), cap) * itemsize(v) for _, v in arrays) > DUMP_BYTES:
        cap //= 2
    os.makedirs(directory, exist_ok=True)
    manifest = {"cap_elements": cap, "arrays": {}}
    for name, v in arrays:
        entry = {"shape": list(v.shape), "source_dtype": str(v.dtype)}
        if torch.is_tensor(v):
            flat = v.detach().reshape(-1)
            if flat.numel() > cap:
                g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
                idx = torch.randint(0, flat.numel(), (cap,), generator=g).sort().values
                flat = flat[idx.to(flat.device)]
                entry["sample"] = {"elements": cap, "indices": "sorted torch.randint(0, numel, (elements,)) of torch.Generator().manual_seed(crc32(name)), flat order"}
            else:
                flat = flat.reshape(tuple(v.shape))
            a = flat.to(torch.float32 if itemsize(v) == 4 else torch.float64).cpu().numpy()
        else:
            a = v
        entry["dtype"] = str(a.dtype)
        np.save(os.path.join(directory, f"{name}.npy"), a)
        manifest["arrays"][name] = entry
    with open(os.path.join(directory, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1, help="image pairs per step per GPU (configs[1] = 1)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3"], help="the timed mode (default: the 1e-3 parity mode)")
    ap.add_argument("--depth", type=int, default=1, help="steps in flight: 1 = one synchronous forward() per step (default); 2 = SIU3RModel.forward_async, "
                    "step n+1 is enqueued before step n's segment table is picked up on the host (measured: no gain, profiles/r04_pipeline_probe.txt)")
    ap.add_argument("--full", action="store_true", help="also the second precision mode, the roofline, the render legs and the CPU baselines")
    ap.add_argument("--no-second-mode", action="store_true", help="(with --full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full)")
    ap.add_argument("--no-roofline", action="store_true", help="(with --full)")
    ap.add_argument("--no-render", action="store_true", help="(with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become the launcher (one rank per GPU, the contract's own command line)
        # instead of silently timing one rank and printing n_gpus = 1
        if torch.cuda.device_count() < args.gpus:
            raise RuntimeError(f"--gpus {args.gpus} but this node shows {torch.cuda.device_count()} GPU(s)")
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.run(cmd, env=env).returncode)

    from siu3r_amd import distributed as D
    from siu3r_amd import ops
    from siu3r_amd.model import SIU3RModel
    from siu3r_amd import synthetic_weights as OW  # shared synthetic-weight generator (no checkpoint offline)

    rank, local, world = D.init_from_env()
    if world != args.gpus:
        raise RuntimeError(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus} (or without a launcher: bench.py spawns the ranks itself)")
    local = local % torch.cuda.device_count()  # (lets a gloo dry run put two ranks on one GPU; one GPU per rank otherwise)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    H = W = args.size
    B = args.batch

    sd = OW.make_weights(0)
    g = torch.Generator().manual_seed(1234 + rank)
    images = torch.rand(B, 2, 3, H, W, generator=g).to(dev)
    K = torch.tensor([[318 / 256, 0, 0.5], [0, 318 / 256, 0.5], [0, 0, 1]])[None, None].repeat(B, 2, 1, 1).to(dev)

    def run_mode(precision):
        model = SIU3RModel(sd, image_size=(H, W), precision=precision, device=dev)

        model.pipeline_depth = depth = max(1, args.depth)

        def step():
            with torch.no_grad():
                return model(images, K, enable_query_class_logit_lift=True)

        def run(n):
            """n steps, every one complete (network body, panoptic post-process, host-side segment lists); with depth > 1 step i+1
            is enqueued before step i's result is picked up, so that consecutive steps overlap on the GPU"""
            if depth == 1:
                out = None
                for _ in range(n):
                    out = step()
                return out
            pend, out = collections.deque(), None
            with torch.no_grad():
                for _ in range(n):
                    pend.append(model.forward_async(images, K, enable_query_class_logit_lift=True))
                    if len(pend) >= depth:
                        out = pend.popleft().result()
                while pend:
                    out = pend.popleft().result()
            return out

        # untimed warm-up: at least 3 passes whatever W is (1st packs the weights eagerly, 2nd captures the HIP graphs, 3rd replays);
        # one more round per extra pipeline slot (each slot captures its own graphs on first use)
        run(max(3, args.warmup) + 2 * (depth - 1))
        model.release_source_weights()
        dt, out = timed_steps(run, args.steps, D, dev)
        return model, step, dt, out

    model, step, dt, out = run_mode(args.precision)
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs)

    # the path's single collective: per-rank additive statistics
    gauss = out[0]
    stats = dict(n_pairs=B * args.steps, n_images=2 * B * args.steps, n_gaussians=gauss.means.shape[1] * B,
                 n_segments=sum(len(i) for i in out[3]), label_checksum=float(gauss.instance_labels.sum().item()))
    total = D.reduce_stats(D.all_gather_stats(D.pack_stats(stats), device=dev))

    second, m2, step2 = None, None, None
    if args.full and not args.no_second_mode:
        other = "bf16" if args.precision == "bf16x3" else "bf16x3"
        m2, step2, dt2, out2 = run_mode(other)
        second = {"precision": other, "value": B * args.steps * world / dt2, "unit": "image-pairs/s", "ms_per_step": dt2 / args.steps * 1e3,
                  "n_segments_per_step": sum(len(i) for i in out2[3]), "parity": PARITY[other]}
        del out2
    del sd

    if rank != 0:
        return
    pairs = total["n_pairs"]
    value = pairs / dt
    x3 = args.precision == "bf16x3"
    result = {
        "metric": "image-pairs/sec @2x512^2 (SIU3R network forward incl. panoptic post-process)",
        "value": value, "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16x3 (fp32 activations, bf16 MFMA with hi/lo operand split; meets the 1e-3 parity bar)" if x3 else "bf16",
        "data": "synthetic (seeded uniform images, seeded synthetic weights of the reference architecture, shaped so that the panoptic result is non-empty)",
        "config": {"workload": f"configs[1]: single pair 2x{H}x{W} per step" if B == 1 else f"{B} pairs 2x{H}x{W} per step",
                   "pairs_per_step_per_gpu": B, "image_size": [H, W], "precision": args.precision, "parity": PARITY[args.precision],
                   "parallelism": f"dp{world} (independent pairs, one all-gather of metric statistics)",
                   "launch": "per-chain HIP graphs on 4 streams (encoder+decoder+pts3d heads | ViT-Adapter+Mask2Former | Gaussian head 1 | Gaussian head 2)" if (model.use_graph and model._ctx.concurrent) else "eager",
                   "steps_in_flight": max(1, args.depth),
                   "pipelining": ("forward_async: step n+1 is enqueued (own buffers, graphs and streams) before step n's segment table is read on the host; "
                                  "every step is complete and inside the timed region; results bit-identical to forward()") if args.depth > 1 else "none (synchronous forward per step)",
                   "n_segments_per_step": total["n_segments"] / max(1, world), "n_gaussians_per_step": total["n_gaussians"] / max(1, world),
                   "board": _board_id()},  # boards of this pool differ by +-3.5 % on the same tree (README): a number is tied to the one it ran on
        "network_tflops_algorithmic": value * FLOPS_PER_PAIR_512 * (H * W / (512 * 512)) / 1e12,
    }
    if second:
        result["second_mode"] = second

    if args.full and not args.no_roofline:
        result["roofline"] = gemm_roofline(model, step, args.precision, B, H, W)
        if second and m2 is not None:
            second["roofline"] = gemm_roofline(m2, step2, second["precision"], B, H, W)

    if args.full and not args.no_render:
        result.update(render_legs(gauss, B, H, W, dev, world, step=step))

    if args.full and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baselines(images, K, H, W)
    print(json.dumps(result))


def _profile_kernel_stats(which="step_kernels.txt"):
    """newest committed rocprofv3 summary of this command, steady state: {kernel name: (launches per step, average ns per launch)} from
    profiles/rNN_step_kernels.txt (the difference of a 25-step and a 5-step `rocprofv3 --kernel-trace --stats` profile: 20 replayed steps,
    no warm-up / capture / weight-packing launches in it; the chains run CONCURRENTLY there, kernels share the chip) or
    rNN_eager_step_kernels.txt (the same for eager single-stream steps: every kernel alone, the regime of this file's HIP-event leg);
    falls back to rNN_bench_kernel_stats.csv (every launch of the whole command)"""
    import csv
    import re
    path = _latest_profile(which)
    if os.path.exists(path):
        rows = {}
        for line in open(path):
            m = re.match(r"\s*([0-9.]+) us/step\s+([0-9.]+) launches/step\s+(.*)$", line)
            if m and float(m.group(2)) > 0:
                rows[m.group(3).strip()] = (float(m.group(2)), float(m.group(1)) * 1e3 / float(m.group(2)))
        if rows:
            return "profiles/" + os.path.basename(path), rows
    path = _latest_profile("bench_kernel_stats.csv")
    if not os.path.exists(path):
        return None, {}
    rows = {}
    for r in csv.DictReader(open(path)):
        try:
            rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]) / max(1, int(r["Calls"])))
        except (KeyError, ValueError):
            pass
    return "profiles/" + os.path.basename(path), rows


def gemm_roofline(model, step, precision, B, H, W, passes=3):
    """roofline object of the mode's dominant kernel, MEASURED in this run: HIP events around every GEMM launch (on the launch stream)
    of eager single-stream steps, each queued behind a sleep kernel so that the event pairs time the kernels back to back.  One
    UNTIMED eager pass first (the eager path's own buffers, split-K workspaces and lazily packed operands are touched for the first
    time there: round 4's single un-warmed pass read 4-9x too slow on two instantiations), then `passes` timed passes; every
    instantiation's time is the MEDIAN over the passes of its summed launch time in a pass.  "Kernel" = the source-level kernel (a
    function template: rocprofv3 lists each instantiation -- tile shape, A-operand mode, fused LayerNorm -- as its own row, and the
    ping-pong GEMM runs as a dozen of them); the dominant one is the one with the largest summed launch time.  achieved = its
    launches' 2 M N K / their summed (median) durations; `instantiations` lists the rows it is made of.  `traffic` and
    `mfma_busy_counter_frac` need hardware counters (rocprofv3 --pmc: not collectable from inside the process): they are read from the
    newest committed counter pass and say so (`traffic_live` / `mfma_busy_live` = false)."""
    import statistics
    from siu3r_amd import ops

    conc, model._ctx.concurrent = model._ctx.concurrent, False  # one stream: every launch between its own two events

    def eager_pass(timed):
        timer = ops.KernelTimer() if timed else None
        ops.set_kernel_timer(timer)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(int(2.0e8))  # ~0.1 s: the whole step is enqueued before it runs
        e0.record()
        step()
        e1.record()
        ops.set_kernel_timer(None)
        torch.cuda.synchronize()
        return (timer.summary() if timed else None), e0.elapsed_time(e1)

    try:
        eager_pass(False)
        runs = [eager_pass(True) for _ in range(max(3, passes))]
    finally:
        model._ctx.concurrent = conc
        ops.set_kernel_timer(None)
    eager_step_ms = statistics.median(r[1] for r in runs)
    # what an event pair adds to a launch: pairs around a 64-float kernel, queued behind a sleep kernel like the passes above (the pair's own
    # barrier packets and the kernel boundary; the trivial kernel itself is ~1.5 us of it).  Reported, NOT subtracted from anything.
    pair_floor_us = None
    try:
        from siu3r_amd import raster as _r
        x64 = torch.zeros(64, device="cuda")
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(64)]
        torch.cuda._sleep(int(2.0e7))
        for a_, b_ in evs:
            a_.record(); _r.scale_inplace_(x64, 1.0); b_.record()
        torch.cuda.synchronize()
        pair_floor_us = statistics.median(a_.elapsed_time(b_) for a_, b_ in evs) * 1e3
    except Exception:
        pass
    summ = {}
    for k in runs[0][0]:
        per = [r[0][k] for r in runs if k in r[0]]
        summ[k] = dict(launches=per[0]["launches"], flops=per[0]["flops"], ms=statistics.median(p_["ms"] for p_ in per),
                       ms_min=min(p_["ms"] for p_ in per), ms_max=max(p_["ms"] for p_ in per))
    fams = {}
    for k, v in summ.items():
        f = fams.setdefault(_family(k), dict(launches=0, flops=0.0, ms=0.0))
        for key in f:
            f[key] += v[key]
    name, d = max(fams.items(), key=lambda kv: kv[1]["ms"])
    achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
    npass = 3 if precision == "bf16x3" else 1
    traffic, traffic_src = (None, None)
    if B == 1 and (H, W) == (512, 512):
        traffic, traffic_src = pmc_bytes(f"bench_{precision}", name)
    busy = None
    if os.path.exists(BUSY_FILE):
        rows = [v for n, v in json.load(open(BUSY_FILE)).get(f"bench_{precision}", {}).get("kernels", {}).items() if _family(n) == name]
        act = sum(v["GRBM_GUI_ACTIVE"] for v in rows)
        if act > 0:
            busy = sum(v["SQ_VALU_MFMA_BUSY_CYCLES"] for v in rows) / (act / 8.0 * 1024.0)
    variants = lambda pred: {k: {"launches": v["launches"], "ms": v["ms"], "avg_launch_us": v["ms"] * 1e3 / v["launches"],
                                 "avg_launch_us_min_max_over_passes": [v["ms_min"] * 1e3 / v["launches"], v["ms_max"] * 1e3 / v["launches"]],
                                 "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12} for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]) if pred(k)}
    # consistency: (i) the kernels of one serial step cannot take longer than the step; (ii) the committed rocprofv3 summary of the SAME
    # regime (eager, one stream: profiles/rNN_eager_step_kernels.txt) must agree on the dominant kernel's average launch duration; and,
    # for the record, (iii) the same kernel inside the replayed multi-stream step (profiles/rNN_step_kernels.txt): there its launches share
    # the chip with the other chains and take longer -- `in_step` is that figure, from the committed profile, not measured in this run
    gemm_ms = sum(v["ms"] for v in summ.values())
    avg_us = d["ms"] * 1e3 / d["launches"]

    def prof_avg(which):
        pn, prof = _profile_kernel_stats(which)
        prow = [(c, ns) for n, (c, ns) in prof.items() if _family(n.replace("void ", "")) == name and (("<true" in n) == (precision == "bf16x3"))]
        return pn, (sum(c * ns for c, ns in prow) / max(1e-9, sum(c for c, _ in prow)) / 1e3 if prow else None)

    prof_name, prof_avg_us = prof_avg("eager_step_kernels.txt")
    same_regime = prof_name is not None and prof_name.endswith("eager_step_kernels.txt") and B == 1 and (H, W) == (512, 512)  # (the committed profiles are one pair per step)
    step_name, step_avg_us = prof_avg("step_kernels.txt")
    check = {"dominant_ms_le_eager_step": bool(d["ms"] <= eager_step_ms), "gemm_ms_le_eager_step": bool(gemm_ms <= eager_step_ms),
             "eager_single_stream_step_ms": eager_step_ms, "profile": prof_name, "profile_is_same_regime": same_regime,
             "profile_avg_launch_us": prof_avg_us, "ratio_to_profile": (avg_us / prof_avg_us) if prof_avg_us else None,
             "agrees_with_profile_within_10pct": bool(abs(avg_us / prof_avg_us - 1.0) <= 0.10) if (prof_avg_us and same_regime) else None}
    # (boards of the pool sustain clocks +-3.5 % apart on one tree -- DESIGN.md section 5, round 6 item 12 -- and the event pairs include
    # the launch gap, +5-8 %: on a slower board than the committed profile's the ratio passes 1.10; the line says which board the profile is from)
    try:
        pb = open(os.path.join(ROOT, "profiles", os.path.basename(prof_name or "").split("_")[0] + "_profile_board.txt")).read().strip()  # (written by tools/evidence_round.sh)
    except Exception:
        pb = None
    check["profile_board"], check["same_board_as_profile"] = pb, (pb == _board_id()) if pb else None
    in_step = None
    if step_avg_us and step_name.endswith("step_kernels.txt") and not step_name.endswith("eager_step_kernels.txt"):
        in_step = {"source": step_name + " (replayed multi-stream step under rocprofv3 --kernel-trace: the chains run beside each other)", "live": False,
                   "avg_launch_us": step_avg_us, "achieved": d["flops"] / d["launches"] / (step_avg_us * 1e-6) / 1e12,
                   "frac": d["flops"] / d["launches"] / (step_avg_us * 1e-6) / 1e12 / MFMA_BF16_PEAK_TFLOPS}
    if not check["gemm_ms_le_eager_step"] or check["agrees_with_profile_within_10pct"] is False:
        print(f"bench.py: roofline consistency check: {check}", file=sys.stderr)
    return {
        "kernel": name,
        "bound": "mfma", "achieved": achieved, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
        "frac": achieved / MFMA_BF16_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_src, "traffic_live": False,
        "timing": f"HIP events per launch on the launch stream, {len(runs)} warm eager single-stream passes after one untimed pass, median per instantiation",
        "mfma_passes_per_product": npass, "mfma_issue_frac": achieved * npass / MFMA_BF16_PEAK_TFLOPS,
        "mfma_busy_counter_frac": busy, "mfma_busy_live": False,
        "mfma_busy_source": "profiles/" + os.path.basename(BUSY_FILE) + " (SQ_VALU_MFMA_BUSY_CYCLES pass, all instantiations)" if busy is not None else None,
        "launches_per_step": d["launches"], "avg_launch_us": avg_us,
        "event_pair_around_a_64_float_kernel_us": pair_floor_us,  # what the timing method adds to every launch (the profile's per-kernel durations do not carry it)
        "algorithmic_flops_per_launch_avg": d["flops"] / d["launches"],
        "share_of_gemm_time": d["ms"] / gemm_ms,
        "gemm_time_ms_per_step": gemm_ms,
        "gemm_tflops_all_kernels": sum(v["flops"] for v in summ.values()) / (gemm_ms * 1e-3) / 1e12,
        "consistency": check,
        "in_step": in_step,
        "instantiations": variants(lambda k: _family(k) == name),
        "other_gemm_kernels": variants(lambda k: _family(k) != name),
    }


def render_legs(gauss, B, H, W, dev, world, step=None):
    """render ms/frame (the metric's second half) through the product path, K2 semantics (SplattingCUDA.forward: colour + depth):
      render             the network's own Gaussians (synthetic weights: few of them land in view)
      render_pair_scene  a pixel-aligned 2 x H x W Gaussian set as a trained network emits for an indoor pair (>= 50 % in view)
      render_stress      BASELINE.json configs[4] shape: 2 097 152 Gaussians, one 1920 x 1080 frame"""
    from siu3r_amd import cuda_splatting as cs, raster, synthetic
    from siu3r_amd.gaussian_renderer import SplattingCUDA
    from siu3r_amd.gaussians_types import Gaussians

    out = {}
    nv = 6
    ext1 = synthetic.target_views(nv)
    Kt1 = synthetic.default_intrinsics()[None].repeat(nv, 1, 1)
    rend = SplattingCUDA(deferred_overflow_check=True)  # no device synchronisation per call; rend.check_pending() below is the barrier

    def leg(means, cov, sh, opac, label):
        """means [b,G,3] ... on the device; forward rescales means / covariances in place, hence the fresh copies"""
        b = means.shape[0]
        ext, Kt = ext1[None].repeat(b, 1, 1, 1).to(dev), Kt1[None].repeat(b, 1, 1, 1).to(dev)  # camera tensors on the device, as the pipeline holds them
        fresh = lambda: Gaussians(means=means.clone(), covariances=cov.clone(), harmonics=sh, opacities=opac)
        rend.forward(fresh(), ext, Kt, (H, W), render_color=True)  # warm-up
        reps = 6
        gs = [fresh() for _ in range(reps)]
        it = iter(gs)
        ms_frame = event_ms(lambda: rend.forward(next(it), ext, Kt, (H, W), render_color=True), reps) / (b * nv)
        rend.check_pending()  # (raises if a timed frame overflowed its buffers and was rendered as NaN)
        # data-dependent sizes of the views of item 0 (visible Gaussians, (Gaussian, tile) pairs) for the algorithmic byte count
        e = ext1.clone()
        e[:, :3, 3] *= 10.0
        _, _, aux = cs.render_cuda(e, Kt1, torch.full((nv,), 1.0), torch.full((nv,), 1000.0), (H, W), torch.zeros(nv, 3), (means[0] * 10.0)[None].expand(nv, -1, -1),
                                   (cov[0] * 100.0)[None].expand(nv, -1, -1, -1), sh[0][None].expand(nv, -1, -1, -1), opac[0][None].expand(nv, -1), return_aux=True)
        st = aux[0]["state"]
        G = means.shape[1]
        Gv, Dp = st.totals(0), st.totals(1)
        bytes_alg = sum(raster.algorithmic_bytes(G, gv, d, H * W) for gv, d in zip(Gv, Dp)) / nv
        ach = bytes_alg / (ms_frame * 1e-3) / 1e9
        return {"ms_per_frame": ms_frame, "views": nv, "resolution": [H, W], "gaussians": G, "visible_mean": sum(Gv) / nv, "visible_frac": sum(Gv) / nv / G,
                "tile_pairs_mean": sum(Dp) / nv, "scene": label,
                "semantics": "K2 (diff-gaussian-rasterization family): SH deg 4 -> RGB + depth, all views of an item in one rasterizer call",
                "overflow_check": "deferred (SplattingCUDA(deferred_overflow_check=True): no device synchronisation per call; verified after the timed calls)",
                "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                             "algorithmic_bytes_per_view": bytes_alg, "traffic": None,
                             "note": "whole per-frame pipeline (camera preparation on the device, project, per-view radix sort, coarse binning, composite)"}}

    out["render"] = leg(gauss.means, gauss.covariances, gauss.harmonics, gauss.opacities, "the network's own output (synthetic weights)")

    if step is not None:
        # SURVEY 8(d) config 2, second figure: network + 6-view colour render per pair, every step complete (forward incl. its host
        # pick-up of the segment table, then SplattingCUDA.forward on that step's own Gaussians: in-place x10 rescale as in the reference)
        ext_b, Kt_b = ext1[None].repeat(B, 1, 1, 1).to(dev), Kt1[None].repeat(B, 1, 1, 1).to(dev)

        def both():
            g_ = step()[0]
            return rend.forward(g_, ext_b, Kt_b, (H, W), render_color=True)

        both()
        torch.cuda.synchronize()
        n_it = 10
        t0 = time.perf_counter()
        for _ in range(n_it):
            both()
        torch.cuda.synchronize()
        dt_b = (time.perf_counter() - t0) / n_it
        rend.check_pending()
        out["network_plus_render"] = {"value": B / dt_b, "unit": "image-pairs/s", "ms_per_step": dt_b * 1e3, "views_rendered_per_pair": nv,
                                      "resolution": [H, W], "what": "forward (as in the timed region) + SplattingCUDA.forward colour + depth of 6 target views per pair, "
                                      f"wall clock over {n_it} steps on this rank"}
    pm, pc, po, ps = (t.to(dev) for t in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
    out["render_pair_scene"] = leg(pm[None], pc[None], ps[None], po[None], "siu3r_amd.synthetic.pixel_aligned_scene(seed=0): 2 views x H x W pixel-aligned Gaussians of an indoor pair")
    if (H, W) == (512, 512):
        t, src = pmc_frame_bytes("raster_pair", nv)
        out["render_pair_scene"]["roofline"]["traffic"], out["render_pair_scene"]["roofline"]["traffic_source"] = t, src
    out["render_qc_logits"] = logit_leg(pm, pc, po, ext1, Kt1, H, W, nv, q=8, classes=21)
    del pm, pc, po, ps

    if world == 1:
        Gs, Ws, Hs = 2_097_152, 1920, 1080
        m_, cov_, op_, sh_ = (t.to(dev) for t in synthetic.random_scene(Gs, seed=1, spread=3.0, depth=(2.0, 9.0), scale=(0.004, 0.03)))
        c2w = synthetic.perturbed_camera(0, jitter=0.1)
        w2c = torch.linalg.inv(c2w)
        fx = 0.9 * Ws
        fovx, fovy = 2 * math.atan(Ws / (2 * fx)), 2 * math.atan(Hs / (2 * fx))
        proj = cs.get_projection_matrix(torch.tensor([0.1]), torch.tensor([100.0]), torch.tensor([fovx]), torch.tensor([fovy]))[0]
        cam2 = raster.make_cam_k2(w2c=w2c, full_proj=proj @ w2c, tanfovx=math.tan(fovx / 2), tanfovy=math.tan(fovy / 2), campos=c2w[:3, 3],
                                  bg=torch.zeros(3), width=Ws, height=Hs, sh_degree=4)
        run = lambda: raster.rasterize_views_k2([cam2], m_, cov_, sh_, op_, want_n_touched=True, sh_planar=True, check_overflow="deferred")
        for _ in range(2):
            o = run()
        ms_s = event_ms(run, 5)
        raster.check_pending()
        o = run()
        raster.check_pending()
        st = o["state"]
        Gv_s, D_s = st.totals(0)[0], st.totals(1)[0]
        b_s = raster.algorithmic_bytes(Gs, Gv_s, D_s, Hs * Ws)
        t, src = pmc_frame_bytes("raster_stress", 1)
        out["render_stress"] = {"ms_per_frame": ms_s, "resolution": [Ws, Hs], "gaussians": Gs, "visible": Gv_s, "visible_frac": Gv_s / Gs, "tile_pairs": D_s,
                                "scene": "siu3r_amd.synthetic.random_scene(seed=1): configs[4] shape (8 views x 512^2 worth of Gaussians, 1080p), RGB + depth + n_touched",
                                "roofline": {"bound": "hbm", "achieved": b_s / (ms_s * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                             "frac": b_s / (ms_s * 1e-3) / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_view": b_s, "traffic": t, "traffic_source": src}}
        del m_, cov_, op_, sh_, o
    return out


def logit_leg(means, cov, opac, ext, Kt, H, W, nv, q=8, classes=21):
    """SURVEY 8(d) config 5, C-channel variant: the query x class logit render of the evaluation loop (reference
    src/models/gaussian_renderer.py:81-110: gsplat semantics, C = q * 21 feature channels per Gaussian, rendered in 32-channel chunks
    over one set of materialised per-tile lists), q = 8 kept queries -> 168 channels, the pixel-aligned pair scene, 6 views in one
    call.  Algorithmic bytes per view: (44 + 4C) G + 36 G_v + (76 + 4C) D + (4C + 4) P."""
    from siu3r_amd import raster

    dev = means.device
    G, Cc = means.shape[0], q * classes
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(G, Cc, generator=gen).to(dev)
    e = ext.clone()
    e[:, :3, 3] *= 10.0  # SplattingCUDA.forward's scene rescale (x10 means, x100 covariances, near = 1, far = 1000)
    m10, c100 = (means * 10.0).contiguous(), (cov * 100.0).contiguous()
    cams = []
    for j in range(nv):
        Kp = Kt[j].clone()
        Kp[0, :] *= W
        Kp[1, :] *= H
        cams.append(raster.make_cam_k3(torch.linalg.inv(e[j]), Kp[0, 0], Kp[1, 1], Kp[0, 2], Kp[1, 2], W, H, near_plane=1.0, far_plane=1000.0))
    run = lambda: raster.rasterize_views_k3(cams, m10, c100, opac, feats)
    o = run()
    o = run()  # (pair-list capacity remembered by the first call)
    st = o["state"]
    Gv, Dp = st.totals(0), st.totals(1)
    ms_frame = event_ms(run, 5) / nv
    bytes_alg = sum(raster.algorithmic_bytes(G, gv, d, H * W, channels=Cc) for gv, d in zip(Gv, Dp)) / nv
    ach = bytes_alg / (ms_frame * 1e-3) / 1e9
    return {"ms_per_frame": ms_frame, "views": nv, "resolution": [H, W], "gaussians": G, "channels": Cc, "kept_queries": q, "visible_mean": sum(Gv) / nv,
            "tile_pairs_mean": sum(Dp) / nv, "scene": "siu3r_amd.synthetic.pixel_aligned_scene(seed=0) with seeded normal features [G, q*21]",
            "semantics": "K3 (gsplat.rasterization family): N-channel features, per-tile lists materialised once, all channels composited in one pass as "
                         "rank-2 v_mfma_f32_32x32x2_f32 updates (exact f32, bit-identical to the 32-channel-chunk kernel); overflow counters read after "
                         "every call (one device synchronisation per call, as the evaluation loop runs it)",
            "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                         "algorithmic_bytes_per_view": bytes_alg, "formula": "(44+4C) G + 36 G_v + (76+4C) D + (4C+4) P", "traffic": None}}


def cpu_baselines(images, K, H, W):
    """Bounded CPU samples on the host cores: the fp32 oracle forward (the metric's unit) and the OpenMP reference rasterizer
    (oracle/raster_ref.c) on one frame of the pair scene.  Test infrastructure used as the thing to compare against, never shipped."""
    from oracle import siu3r_oracle as O
    from oracle import raster_oracle as RO
    from siu3r_amd import cuda_splatting as cs, raster, synthetic
    from siu3r_amd import synthetic_weights as OW

    # 16 threads (256 oversubscribed threads made one forward take 830 s on the GPU box); a quarter-size pair first, and the
    # full-size pair only if it is predicted to stay within ~40 s
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd_cpu = OW.make_weights(0)
    K_c = K[:1].cpu()
    img_q = torch.nn.functional.interpolate(images[0].cpu(), size=(H // 2, W // 2), mode="bilinear")[None]
    t1 = time.perf_counter()
    with torch.no_grad():
        O.model_forward(sd_cpu, img_q, K_c, keep_intermediates=False)
    t_q = time.perf_counter() - t1
    if t_q * 4.4 <= 40.0:
        t1 = time.perf_counter()
        with torch.no_grad():
            O.model_forward(sd_cpu, images[:1].cpu(), K_c, keep_intermediates=False)
        t_cpu = time.perf_counter() - t1
        sample = f"1 pair 2x{H}x{W}, one fp32 forward = {t_cpu:.1f} s"
    else:
        t_cpu = t_q * 4.27  # FLOP ratio 4059.0 / 950.7 GFLOP between 512^2 and 256^2
        sample = f"1 pair 2x{H//2}x{W//2} = {t_q:.1f} s, scaled x4.27 (FLOP ratio) to 2x{H}x{W}"
    base = {"value": 1.0 / t_cpu, "unit": "image-pairs/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": sample + "; oracle/siu3r_oracle.py = parity-pinned fp32 port of the reference forward"}

    # rasterizer: one 512^2 frame of the pixel-aligned pair scene (524 288 Gaussians) through oracle/raster_ref.c, OpenMP over tiles
    threads = min(32, os.cpu_count() or 1)
    os.environ["OMP_NUM_THREADS"] = str(threads)  # read when libgomp starts its first team (the library is loaded below)
    means, cov, opac, sh = synthetic.pixel_aligned_scene(H, W, 2, seed=0)
    e = synthetic.target_views(2)[1].clone()
    e[:3, 3] *= 10.0
    Kt = synthetic.default_intrinsics()
    fov = cs.get_fov(Kt[None])
    tan = (0.5 * fov).tan()[0]
    proj = cs.get_projection_matrix(torch.tensor([1.0]), torch.tensor([1000.0]), fov[:, 0], fov[:, 1])[0]
    w2c = torch.linalg.inv(e)
    cam = raster.make_cam_k2(w2c, proj @ w2c, float(tan[0]), float(tan[1]), e[:3, 3].tolist(), [0, 0, 0], W, H, sh_degree=4)
    a = ((means * 10.0).numpy(), raster.cov6_from_cov3x3(cov * 100.0).numpy(), opac.numpy(), sh.permute(0, 2, 1).contiguous().numpy())
    RO.forward(cam, *a, want_lists=False)  # warm-up (page faults, thread team start)
    t1 = time.perf_counter()
    n = 0
    while n < 3 or (time.perf_counter() - t1 < 5.0 and n < 20):
        ref = RO.forward(cam, *a, want_lists=False)
        n += 1
    t_r = (time.perf_counter() - t1) / n
    base["raster"] = {"value": 1.0 / t_r, "unit": "frames/s", "ms_per_frame": t_r * 1e3, "cores": threads, "kind": "port",
                      "sample": f"{n} x one {H}x{W} frame of the pair scene ({means.shape[0]} Gaussians, {int((ref['tiles_touched'] > 0).sum())} visible, "
                                f"{ref['D']} tile pairs), whole pipeline; oracle/raster_ref.c (-O2 -fopenmp, tiles in parallel; projection and sort serial)"}
    return base


if __name__ == "__main__":
    main()
