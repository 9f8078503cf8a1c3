"""The bilateral-grid unit (csrc/bilagrid.hip) and what it costs a refinement iteration, written to profiles/bilagrid_timing.json:
microseconds of the slice, its backward to the image, its backward to the grid (at the default 16 x 16 x 8 grid and at a 4 x 4 x 4 grid with
one view: 16 workgroups on 256 CUs) and the total variation, next to the affine exposure's forward and backward, at V = 6, 512 x 512
(device events around 200 calls, five turns, the minimum and every turn); and milliseconds of one refine_gaussians iteration of the
tests/refine_scenes.py family (20,000 Gaussians, 4 views at 128 x 128, the "appearance" fields free) with cameras=None, the affine control
and the bilagrid control, host clock around 30 iterations ending in a synchronise, three alternating turns.
  python tools/mb_bilagrid.py                      this tree
  python tools/mb_bilagrid.py --parent PATH        also cameras=None on another checkout (the parent commit, built), in child processes that
                                                   take turns with this tree's
  python tools/mb_bilagrid.py --out FILE           write the record there instead of profiles/bilagrid_timing.json
  python tools/mb_bilagrid.py --kernels-only       the calls only, nothing written: the program to put behind
                                                   `rocprofv3 --kernel-trace --stats --` (profiles/bilagrid_kernel_stats.csv)
The event times are per Python call (autograd, allocations and the launches included): where a kernel is shorter than the host side of a
call they measure the enqueue rate of the host and are an upper bound; the kernel trace has the kernels' own durations.
No threshold is attached to any of these numbers; the file is the record."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
CHILD = "--refine-only" in args  # a child process: one set of refinement turns of the tree at --root, printed as a JSON line
root = os.path.abspath(args[args.index("--root") + 1]) if "--root" in args else ROOT
parent = os.path.abspath(args[args.index("--parent") + 1]) if "--parent" in args else None
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _render, _truth
from siu3r_amd import refine

assert torch.cuda.is_available(), "mb_bilagrid.py measures on the GPU"


def refine_turns(variants, turns=3, iters=30):
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
    print(json.dumps(refine_turns({"cameras_none": {}})["cameras_none"]))
    sys.exit(0)

from siu3r_amd import losses
from siu3r_amd.cameras import CameraControl, identity_grids

props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} {props.uuid}")


def event_us(fn, n=200, turns=5):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(turns):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / n * 1e3)
    return out


def backward_of(out, leaves, g):
    def run():
        for t in leaves:
            t.grad = None
        out.backward(g, retain_graph=True)
    return run


V, S = 6, 512
g = torch.Generator().manual_seed(0)
img = torch.rand(V, 3, S, S, generator=g).cuda()
g_out = torch.randn(V, 3, S, S, generator=g).cuda()
M = (torch.eye(3, 4).repeat(V, 1, 1) + 0.05 * torch.randn(V, 3, 4, generator=g)).cuda()
grids = identity_grids(V, (16, 16, 8), "cuda") + 0.05 * torch.randn(V, 12, 8, 16, 16, generator=g).cuda()
small = identity_grids(1, (4, 4, 4), "cuda") + 0.05 * torch.randn(1, 12, 4, 4, 4, generator=g).cuda()
x, m = img.clone().requires_grad_(True), M.clone().requires_grad_(True)
xg, a = img.clone().requires_grad_(True), grids.clone().requires_grad_(True)
a_only, a_small, a_tv = grids.clone().requires_grad_(True), small.clone().requires_grad_(True), grids.clone().requires_grad_(True)
plane = V * 3 * S * S * 4
kernels = {
    "exposure_forward": (event_us(lambda: losses.apply_exposure(img, M)), 2 * plane),
    "exposure_backward_both_gradients": (event_us(backward_of(losses.apply_exposure(x, m), (x, m), g_out)), 3 * plane),
    "bilagrid_forward": (event_us(lambda: losses.apply_bilagrid(img, grids)), 2 * plane),                                  # image in, image out
    "bilagrid_backward_image_only": (event_us(backward_of(losses.apply_bilagrid(xg, grids), (xg,), g_out)), 3 * plane),   # g_out and image in, g_in out
    "bilagrid_backward_grid_only": (event_us(backward_of(losses.apply_bilagrid(img, a_only), (a_only,), g_out)), None),   # each pixel is read by 4 vertices
    "bilagrid_backward_both_gradients": (event_us(backward_of(losses.apply_bilagrid(xg, a), (xg, a), g_out)), None),
    "bilagrid_backward_grid_only_4x4x4_one_view": (event_us(backward_of(losses.apply_bilagrid(img[:1], a_small), (a_small,), g_out[:1])), None),
    "bilagrid_tv_value_and_gradient": (event_us(lambda: losses.bilagrid_tv(a_tv)), None),
}
record = {"device": props.name, "gpu_uuid": str(props.uuid), "shape": [V, 3, S, S], "grid": [V, 12, 8, 16, 16], "kernels_us": {}}
for k, (us, byt) in kernels.items():
    record["kernels_us"][k] = {"min": min(us), "turns": us}
    if byt:
        record["kernels_us"][k].update(algorithmic_bytes=byt, share_of_8TBps_peak=byt / 8e12 / (min(us) * 1e-6))
    print(f"{k}: {min(us):.2f} us (turns {' '.join(f'{u:.2f}' for u in us)})")

if "--kernels-only" in args:
    sys.exit(0)
child = lambda: json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--refine-only", "--root", parent], check=True, capture_output=True,
                                          text=True).stdout.strip().splitlines()[-1])
refine_ms = {}
if parent:
    refine_ms["parent_cameras_none"] = child()
refine_ms.update(refine_turns({"cameras_none": {}, "affine_control": dict(cameras=CameraControl(pose=False, exposure="affine")),
                               "bilagrid_control": dict(cameras=CameraControl(pose=False, exposure="bilagrid"))}))
if parent:
    refine_ms["parent_cameras_none"] += child()
record["refine_iteration_ms"] = {k: {"min": min(v), "turns": v} for k, v in refine_ms.items()}
record["refine_scene"] = "tests/refine_scenes.py: 20,000 Gaussians, 4 views 128 x 128, scales / opacities / harmonics free, optimizer=torch, pose off"
for k, v in refine_ms.items():
    print(f"refine iteration, {k}: {min(v):.3f} ms (turns {' '.join(f'{u:.3f}' for u in v)})")
path = os.path.abspath(args[args.index("--out") + 1]) if "--out" in args else os.path.join(ROOT, "profiles", "bilagrid_timing.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
print("wrote", path)
