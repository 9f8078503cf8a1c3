"""The camera unit (csrc/camera.hip) and what it costs a refinement iteration, written to profiles/camera_step_timing.json:
microseconds of the exposure forward, the exposure backward (both gradients) and the camera step at V = 6, 512 x 512 (device events around
200 calls, five turns, the minimum and every turn), with the exposure kernels' algorithmic bytes as a fraction of the 8 TB/s HBM peak; and
milliseconds of one refine_gaussians iteration of the tests/refine_scenes.py family (20,000 Gaussians, 4 views at 128 x 128, the
"appearance" fields free) with cameras=None and with a CameraControl, host clock around 30 iterations ending in a synchronise, three
alternating turns.
  python tools/mb_camera.py                        this tree
  python tools/mb_camera.py --parent PATH          also cameras=None on another checkout (the parent commit, built), in child processes that
                                                   take turns with this tree's
  python tools/mb_camera.py --out FILE             write the record there instead of profiles/camera_step_timing.json
  python tools/mb_camera.py --kernels-only         the three calls only, nothing written: the program to put behind
                                                   `rocprofv3 --kernel-trace --stats --` (profiles/camera_kernel_stats.csv)
The event times are per Python call (autograd, allocations and the launches included): where the kernels are shorter than the host side of
a call, as here, they measure the enqueue rate of the host and are an upper bound; the kernel trace has the kernels' own durations.
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

assert torch.cuda.is_available(), "mb_camera.py measures on the GPU"


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
from siu3r_amd.cameras import CameraControl, CameraState

props = torch.cuda.get_device_properties(0)
print(f"device: {props.name}")


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


V, S = 6, 512
g = torch.Generator().manual_seed(0)
img = torch.rand(V, 3, S, S, generator=g).cuda()
g_out = torch.randn(V, 3, S, S, generator=g).cuda()
M = (torch.eye(3, 4).repeat(V, 1, 1) + 0.05 * torch.randn(V, 3, 4, generator=g)).cuda()
x, m = img.clone().requires_grad_(True), M.clone().requires_grad_(True)
out = losses.apply_exposure(x, m)


def backward():
    x.grad = m.grad = None
    out.backward(g_out, retain_graph=True)


state = CameraState(torch.eye(4).repeat(V, 1, 1).cuda())
state.rot_delta.grad, state.trans_delta.grad = torch.randn(V, 3, generator=g).cuda(), torch.randn(V, 3, generator=g).cuda()
state.M.grad = torch.randn(V, 3, 4, generator=g).cuda()
plane = V * 3 * S * S * 4
kernels = {
    "exposure_forward": (event_us(lambda: losses.apply_exposure(img, M)), 2 * plane),                 # image in, image out
    "exposure_backward_both_gradients": (event_us(backward), 3 * plane),                              # g_out and image in, g_in out
    "camera_step": (event_us(lambda: state.step(state.step_count + 1, (1e-6, 1e-6, 1e-6))), None),    # (includes the [V,6] gradient concatenation)
}
record = {"device": props.name, "shape": [V, 3, S, S], "kernels_us": {}}
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
refine_ms.update(refine_turns({"cameras_none": {}, "camera_control": dict(cameras=CameraControl()), "camera_control_pose_only": dict(cameras=CameraControl(exposure=False)),
                               "camera_control_exposure_only": dict(cameras=CameraControl(pose=False))}))
if parent:
    refine_ms["parent_cameras_none"] += child()
record["refine_iteration_ms"] = {k: {"min": min(v), "turns": v} for k, v in refine_ms.items()}
record["refine_scene"] = "tests/refine_scenes.py: 20,000 Gaussians, 4 views 128 x 128, scales / opacities / harmonics free, optimizer=torch"
for k, v in refine_ms.items():
    print(f"refine iteration, {k}: {min(v):.3f} ms (turns {' '.join(f'{u:.3f}' for u in v)})")
path = os.path.abspath(args[args.index("--out") + 1]) if "--out" in args else os.path.join(ROOT, "profiles", "camera_step_timing.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
print("wrote", path)
