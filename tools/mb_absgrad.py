"""What the absolute-gradient (AbsGS) densification statistics cost, written to profiles/absgrad_timing.json:
  composite backward   microseconds per call of siu3r_raster_composite_rgb_bwd (plain) and siu3r_raster_composite_rgb_bwd_abs on
                       synthetic.pixel_aligned_scene (2 x 512^2 = 524,288 Gaussians, SH degree 4) seen from six 512 x 512 views, on the state
                       of one forward: device events around 20 calls, five turns per contender, the contenders alternating inside every turn
                       of ONE process, the best turn and every turn.  With --parent the parent commit's library is loaded next to this tree's
                       and its plain entry point takes part in the same turns on the same buffers (`parent_plain`).
  refine iteration     milliseconds of one refine_gaussians iteration of the tests/refine_scenes.py family (20,000 Gaussians, 4 views at
                       128 x 128, scales / opacities / harmonics free, as tools/mb_bilagrid.py times it) with DensityControl(absgrad=False /
                       True) whose first event lies beyond the run (the statistics are kept, the set does not change): host clock around 30
                       iterations ending in a synchronise, five alternating turns in one process.  With --parent the plain iteration of the
                       parent commit (`parent_plain`) and of this tree (`plain_child_process`) also run in fresh child processes, one turn
                       each, five times in alternation: two libraries of one package cannot share a process, and a child process and a
                       process that has already run other work do not time alike, so the parent condition compares child with child.
  first event          (not a timing) on the scene of tests/test_refine_density_gpu.py::test_growth_from_half_the_gaussians, 60 iterations,
                       events at 20 and 40: the rows the first event adds and the held-out PSNR at the end, with the signed statistics at the
                       3DGS threshold 2e-4 and the absolute ones at gsplat's 8e-4.
  python tools/mb_absgrad.py [--parent PATH] [--out FILE]     PATH: a built checkout of the parent commit
The parent condition the record states: the plain path's best turn on this tree does not exceed the parent's worst turn (the margin is
the parent's own turn-to-turn spread).  The cost of the abs form is reported, not bounded."""
import ctypes, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
CHILD = "--refine-only" in args  # a child process: the plain refinement turns of the tree at --root, printed as a JSON line
root = os.path.abspath(args[args.index("--root") + 1]) if "--root" in args else ROOT
parent = os.path.abspath(args[args.index("--parent") + 1]) if "--parent" in args else None
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from refine_scenes import BG, FAR, FIELDS, NEAR, _cams, _psnr, _render, _truth
from siu3r_amd import refine
from siu3r_amd.density import DensityControl

assert torch.cuda.is_available(), "mb_absgrad.py measures on the GPU"
NEVER = 10 ** 6  # an event schedule that starts beyond every run here


def refine_turns(variants, turns, iters=30):
    """{name: [ms per iteration, one per turn]}; the variants take turns"""
    s = _truth()
    c2w, K = _cams([0, 1, 2, 3])
    targets = _render(c2w, K, s["means"], refine.covariances_from(s["rotations"], s["scales"]), s["harmonics"], s["opacities"])[0]

    def run(n, kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refine.refine_gaussians(*(s[k] for k in FIELDS), targets, c2w, K, NEAR, FAR, BG, iters=n, params=("scales", "opacities", "harmonics"), log_every=0, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for kw in variants.values():
        run(5, kw)
    ms = {k: [] for k in variants}
    for _ in range(turns):
        for k, kw in variants.items():
            ms[k].append(run(iters, kw))
    return ms


if CHILD:
    n = int(args[args.index("--turns") + 1])
    print(json.dumps(refine_turns({"plain": dict(density=DensityControl(start=NEVER))}, n)["plain"]))
    sys.exit(0)

from siu3r_amd import _lib, cuda_splatting as cs, raster, synthetic
from siu3r_amd.ops import _p, _stream

props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} {props.uuid}")
record = {"device": props.name, "gpu_uuid": str(props.uuid)}

# ---- the composite backward on the state of one forward ------------------------------------------------------------------------------------
V, H, W = 6, 512, 512
means, cov, opac, sh = (t.cuda() for t in synthetic.pixel_aligned_scene(H, W, 2, seed=0))
G = means.shape[0]
ext = synthetic.target_views(V)
Kn = synthetic.default_intrinsics()[None].repeat(V, 1, 1)
fov = cs.get_fov(Kn)
tan = (0.5 * fov).tan()
proj = cs.get_projection_matrix(torch.full((V,), 1.0), torch.full((V,), 1000.0), fov[:, 0], fov[:, 1])
cams = []
for v in range(V):
    e = ext[v].clone()
    e[:3, 3] *= 10.0
    w2c = torch.linalg.inv(e)
    cams.append(raster.make_cam_k2(w2c, proj[v] @ w2c, float(tan[v, 0]), float(tan[v, 1]), e[:3, 3].tolist(), [0, 0, 0], W, H, sh_degree=4))
with torch.no_grad():
    o = raster.rasterize_views_k2(cams, means * 10.0, cov * 100.0, sh, opac, sh_planar=sh.dim() == 3 and sh.shape[1] == 3 and sh.shape[-1] == 25)
st = o["state"]
gen = torch.Generator(device="cuda").manual_seed(0)
gi, gd, go = (torch.randn(t.shape, generator=gen, device="cuda") for t in (o["image"], o["depth"], o["opacity"]))
grads = {k: torch.empty((V, G, 10), device="cuda") for k in ("plain", "abs", "parent_plain")}
abs_m = torch.empty((V, G, 2), device="cuda")
common = lambda grad: (st.cams, V, _p(st.cams_dev), G, _p(st.bin_start), _p(st.entries), st.cap_e, _p(st.rec), _p(o["image"]), _p(o["depth"]), _p(o["opacity"]),
                       _p(gi), _p(gd), _p(go), _p(grad))
lib = _lib.lib()
contenders = {"plain": lambda: _lib.check(lib.siu3r_raster_composite_rgb_bwd(*common(grads["plain"]), _stream())),
              "abs": lambda: _lib.check(lib.siu3r_raster_composite_rgb_bwd_abs(*common(grads["abs"]), _p(abs_m), _stream()))}
if parent:
    plib = ctypes.CDLL(os.path.join(parent, "siu3r_amd", "libsiu3r_hip.so"))
    assert not hasattr(plib, "siu3r_raster_composite_rgb_bwd_abs"), "--parent names a tree that already has the abs entry point"
    plib.siu3r_raster_composite_rgb_bwd.argtypes = _lib.SIGNATURES["siu3r_raster_composite_rgb_bwd"]
    contenders = {"parent_plain": lambda: _lib.check(plib.siu3r_raster_composite_rgb_bwd(*common(grads["parent_plain"]), _stream())), **contenders}


def event_turns(fns, n=20, turns=5):
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(turns):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / n * 1e3)
    return out


summary = lambda turns: {"min": min(turns), "max": max(turns), "turns": turns}
us = event_turns(contenders)
pairs = sum(st.totals(1))
record["composite_backward_us"] = {k: summary(v) for k, v in us.items()}
record["composite_backward_scene"] = (f"synthetic.pixel_aligned_scene(512, 512, 2, seed=0): {G} Gaussians, {V} views {W} x {H}, {pairs} (tile, Gaussian) pairs; "
                                      "the clears of grad (and abs_mean2d) are inside the calls")
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
record["composite_backward_agreement"] = {"abs_launch_grad_vs_plain_max_diff_over_max": rel(grads["abs"], grads["plain"]),
                                          "abs_over_signed_mean2d_ratio_of_sums": float(abs_m.sum() / grads["abs"][..., :2].abs().sum())}
if parent:
    record["composite_backward_agreement"]["plain_vs_parent_plain_max_diff_over_max"] = rel(grads["plain"], grads["parent_plain"])
for k, v in us.items():
    print(f"composite backward, {k}: {min(v):.1f} us (turns {' '.join(f'{u:.1f}' for u in v)})")
print(record["composite_backward_agreement"])

# ---- one refinement iteration ------------------------------------------------------------------------------------------------------------
child = lambda tree: json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--refine-only", "--root", tree, "--turns", "1"], check=True,
                                               capture_output=True, text=True).stdout.strip().splitlines()[-1])
refine_ms = refine_turns({"plain": dict(density=DensityControl(start=NEVER)), "abs": dict(density=DensityControl(start=NEVER, absgrad=True))}, 5)
if parent:  # two libraries of one package cannot share a process: both trees' plain iteration in fresh child processes that take turns
    refine_ms.update(parent_plain=[], plain_child_process=[])
    for _ in range(5):
        refine_ms["parent_plain"] += child(parent)
        refine_ms["plain_child_process"] += child(ROOT)
record["refine_iteration_ms"] = {k: summary(v) for k, v in refine_ms.items()}
record["refine_scene"] = ("tests/refine_scenes.py: 20,000 Gaussians, 4 views 128 x 128, scales / opacities / harmonics free, optimizer=torch, "
                          "DensityControl(start beyond the run): statistics kept, no event")
for k, v in refine_ms.items():
    print(f"refine iteration, {k}: {min(v):.3f} ms (turns {' '.join(f'{u:.3f}' for u in v)})")
if parent:
    record["parent_condition"] = {
        "rule": "best turn of the plain path on this tree <= worst turn of the parent's, same board, same run",
        "composite_backward": bool(min(us["plain"]) <= max(us["parent_plain"])),
        "refine_iteration": bool(min(refine_ms["plain_child_process"]) <= max(refine_ms["parent_plain"]))}
    print(record["parent_condition"])

# ---- what the first event does, signed at 2e-4 against absolute at 8e-4 -------------------------------------------------------------------
truth = _truth()
train, Kt = _cams([0, 1, 2, 3])
held, Kh = _cams([4])
cov_of = lambda s: refine.covariances_from(s["rotations"], s["scales"])
targets = _render(train, Kt, truth["means"], cov_of(truth), truth["harmonics"], truth["opacities"])[0]
held_target = _render(held, Kh, truth["means"], cov_of(truth), truth["harmonics"], truth["opacities"])[0][0]
G0 = truth["means"].shape[0]
half = torch.randperm(G0, generator=torch.Generator().manual_seed(21))[: G0 // 2].sort().values.cuda()
start = {k: v[half].clone() for k, v in truth.items()}
psnr = lambda s, c: _psnr(_render(held, Kh, s["means"], c, s["harmonics"], s["opacities"])[0][0], held_target)
record["first_event"] = {"scene": "half of tests/refine_scenes.py's 20,000 Gaussians, 4 training views, 60 iterations, events at 20 and 40, scene_extent 5, "
                                  "held-out view: camera seed 4", "held_out_psnr_at_the_start": psnr(start, cov_of(start))}
for name, ctl in (("signed_2e-4", DensityControl(grad_threshold=2e-4, start=20, every=20, scene_extent=5.0)),
                  ("absgrad_8e-4", DensityControl(absgrad=True, grad_threshold=8e-4, start=20, every=20, scene_extent=5.0)),
                  ("no_control", None)):
    out, losses = refine.refine_gaussians(*(start[k] for k in FIELDS), targets, train, Kt, NEAR, FAR, BG, iters=60, density=ctl)
    ev = out.get("density_events", [])
    record["first_event"][name] = {"rows_added_by_the_first_event": ev[0]["rows_out"] - ev[0]["rows_in"] if ev else 0, "events": ev, "rows_at_the_end": out["means"].shape[0],
                                   "objective_first_last": [losses[0], losses[-1]], "held_out_psnr": psnr(out, out["covariances"])}
    print(f"first event, {name}: {record['first_event'][name]}")

path = os.path.abspath(args[args.index("--out") + 1]) if "--out" in args else os.path.join(ROOT, "profiles", "absgrad_timing.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
print("wrote", path)
