"""Does alias-free refinement help away from the training resolution?  Written to profiles/mip_refine.json.  The scene family of the
refinement tests (tests/refine_scenes.py: 20,000 Gaussians, four training views of 128 x 128), perturbed in scales, opacities and SH, is
refined twice at its training size -- classic, and with refine_gaussians(antialias=MipFilter()) -- and both results are rendered at a
QUARTER of the resolution (32 x 32, the same normalised intrinsics) and compared with the training-size ground truth box-filtered down
(4 x 4 means: what a camera with four times larger pixels would record).  Reported: PSNR per rendering mode, no threshold.
  classic / classic render      the classic result through the classic renderer (the dilation brightens what falls below a pixel)
  classic / anti-aliased render the classic result, only the evaluation render compensated (the 2-D filter alone, at evaluation)
  mip / anti-aliased render     the alias-free result, its 3-D filter baked (mip.bake), through the anti-aliased renderer
and the same at the training size, plus seconds per iteration of either run (host clock around a device synchronise).
  python tools/mip_refine_quality.py [--iters N] [--out FILE]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as Fn
from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _truth
from siu3r_amd import metrics, mip
from siu3r_amd.cuda_splatting import render_cuda
from siu3r_amd.refine import covariances_from, refine_gaussians

assert torch.cuda.is_available(), "mip_refine_quality.py measures on the GPU"
props = torch.cuda.get_device_properties(0)
iters = int(args[args.index("--iters") + 1]) if "--iters" in args else 150
record = {"device": props.name, "gpu_uuid": str(props.uuid), "iters": iters}


def render(c2w, Kn, g, size, antialiased):
    V = c2w.shape[0]
    e = lambda x: x[None].expand(V, *x.shape)
    with torch.no_grad():
        return render_cuda(c2w, Kn, torch.full((V,), NEAR), torch.full((V,), FAR), size, torch.zeros(V, 3), e(g["means"]), e(g["covariances"]), e(g["harmonics"]),
                           e(g["opacities"]), antialiased=antialiased)[0]


def psnr(a, b):
    return float(sum(metrics.psnr(x.permute(1, 2, 0).cpu().numpy(), y.permute(1, 2, 0).cpu().numpy(), data_range=1.0) for x, y in zip(a, b)) / a.shape[0])


truth = _truth()
truth["covariances"] = covariances_from(truth["rotations"], truth["scales"])
c2w, Kn = _cams([0, 1, 2, 3])
held, Kh = _cams([4, 5])
targets = render(c2w, Kn, truth, (H, W), False)
gen = torch.Generator().manual_seed(77)
n = lambda *s: torch.randn(*s, generator=gen).cuda()
G = truth["means"].shape[0]
start = {k: truth[k].clone() for k in FIELDS}
start["harmonics"] = truth["harmonics"] + 0.15 * n(G, 3, 4)
start["opacities"] = torch.sigmoid(torch.logit(truth["opacities"]) + 0.7 * n(G))
start["scales"] = torch.exp(torch.log(truth["scales"]) + 0.2 * n(G, 3))
runs = {}
for name, ctl in (("classic", None), ("mip", mip.MipFilter())):
    for timed in (False, True):  # (the first pass warms the kernels)
        torch.cuda.synchronize()
        t0 = time.time()
        out, losses = refine_gaussians(*(start[k] for k in FIELDS), targets, c2w, Kn, NEAR, FAR, BG, iters=iters if timed else 3, params=("scales", "opacities", "harmonics"),
                                       log_every=max(iters - 1, 1), antialias=ctl)
        torch.cuda.synchronize()
        dt = time.time() - t0
    runs[name] = dict(out=out, losses=losses, seconds_per_iteration=dt / iters)
q = 4
small = (H // q, W // q)
modes = {"classic / classic render": (runs["classic"]["out"], False), "classic / anti-aliased render": (runs["classic"]["out"], True),
         "mip / anti-aliased render": (mip.bake(runs["mip"]["out"]), True), "ground truth / classic render": (truth, False),
         "ground truth / anti-aliased render": (truth, True)}
record["psnr"] = {}
for views, (cc, kk) in (("training views", (c2w, Kn)), ("held-out views", (held, Kh))):
    full = render(cc, kk, truth, (H, W), False)
    low = Fn.avg_pool2d(full, q)
    record["psnr"][views] = {"quarter resolution vs box-filtered ground truth": {m: psnr(render(cc, kk, g, small, aa), low) for m, (g, aa) in modes.items()},
                             "training resolution vs ground truth": {m: psnr(render(cc, kk, g, (H, W), aa), full) for m, (g, aa) in modes.items() if not m.startswith("ground")}}
f3 = runs["mip"]["out"]["filter_3d"]
record["runs"] = {k: dict(first_loss=v["losses"][0], last_loss=v["losses"][-1], seconds_per_iteration=v["seconds_per_iteration"]) for k, v in runs.items()}
record["filter_3d"] = {"median": float(f3.median()), "min": float(f3.min()), "max": float(f3.max()), "median_scale_of_the_result": float(runs["mip"]["out"]["scales"].median())}
record["scene"] = (f"tests/refine_scenes.py: {G} Gaussians, scales 0.01 .. 0.12, four training views {W} x {H} and two held-out ones; start = truth with noise on SH (0.15), logit "
                   f"opacity (0.7), log scale (0.2); params scales / opacities / harmonics; {iters} iterations of torch Adam; quarter resolution {small[1]} x {small[0]}")
print(json.dumps({k: record[k] for k in ("psnr", "runs", "filter_3d")}, indent=1))
path = os.path.abspath(args[args.index("--out") + 1]) if "--out" in args else os.path.join(ROOT, "profiles", "mip_refine.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
print("wrote", path)
