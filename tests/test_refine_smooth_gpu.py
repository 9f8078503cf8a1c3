"""refine.refine_gaussians with the instance-aware depth smoothness (smooth.DepthSmoothness, losses.depth_smoothness,
csrc/depth_smooth.hip): the logs add up, the term goes down and ends below a photometric-only run's, the schedule and the second-order /
expected-depth variant run (the latter beside a depth term), density control runs beside it, and the switched-off path never reaches the
term and keeps its bits.  Scenes as tests/test_refine_gpu.py builds them; the segments are the block map of tests/dense_smooth64.py."""
import numpy as np
import pytest
import torch

import dense_smooth64 as S
from refine_scenes import BG, FAR, FIELDS, H, NEAR, W, _cams, _psnr, _truth

pytestmark = pytest.mark.gpu


def _render(c2w, K, s):
    """(image [V,3,H,W], depth sum w z [V,H,W], opacity sum w [V,H,W]) of a field dict, without gradients"""
    from siu3r_amd.cuda_splatting import render_cuda
    from siu3r_amd.refine import covariances_from

    V = c2w.shape[0]
    e = lambda x: x[None].expand(V, *x.shape)
    cov = s["covariances"] if "covariances" in s else covariances_from(s["rotations"], s["scales"])
    with torch.no_grad():
        img, depth, aux = render_cuda(c2w, K, torch.full((V,), NEAR), torch.full((V,), FAR), (H, W), torch.zeros(V, 3), e(s["means"]), e(cov),
                                      e(s["harmonics"]), e(s["opacities"]), return_aux=True)
    return img, depth, torch.cat([a["opacity"] for a in aux])


def _perturbed(truth, seed=77):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g).cuda()
    G = truth["means"].shape[0]
    start = dict(truth)
    start["means"] = truth["means"] + 0.02 * n(G, 3)
    start["opacities"] = torch.sigmoid(torch.logit(truth["opacities"]) + 0.7 * n(G))
    start["scales"] = torch.exp(torch.log(truth["scales"]) + 0.2 * n(G, 3))
    return {k: v.clone() for k, v in start.items()}


@pytest.fixture(scope="module")
def scene():
    """the truth, its training targets (views 0 and 1: images, expected depth), block segments and the held-out view 4; computed once, read only"""
    truth = _truth()
    train, Kt = _cams([0, 1])
    held, Kh = _cams([4])
    images, depth, opacity = _render(train, Kt, truth)
    held_image, held_depth, held_opacity = _render(held, Kh, truth)
    targets = torch.where(opacity > 0.5, depth / opacity.clamp_min(1e-6), torch.zeros_like(depth))
    return dict(truth=truth, start=_perturbed(truth), train=train, Kt=Kt, held=held, Kh=Kh, images=images, depths=targets,
                segments=S.block_segments(2, H, W).cuda(), held_image=held_image[0], held_depth=held_depth[0], held_opacity=held_opacity[0])


def _args(s):
    return (*(s["start"][k] for k in FIELDS), s["images"], s["train"], s["Kt"], NEAR, FAR, BG)


def test_logs_add_up_and_the_term_goes_down(scene):
    from siu3r_amd import losses
    from siu3r_amd.refine import refine_gaussians
    from siu3r_amd.smooth import DepthSmoothness

    s, w = scene, 2.0
    with_term, l_s = refine_gaussians(*_args(s), iters=60, smooth=DepthSmoothness(weight=w), segments=s["segments"])
    photo_only, l_p = refine_gaussians(*_args(s), iters=60)
    sl = with_term["smooth_losses"]
    assert len(l_s) == len(sl) == len(l_p) == 60 and "smooth_losses" not in photo_only
    assert all(np.isfinite(l_s)) and all(np.isfinite(sl)) and all(np.isfinite(l_p))

    def report(out):
        img, d, o = _render(s["train"], s["Kt"], out)
        term = float(losses.depth_smoothness(d, o, s["segments"]))
        photo = float(losses.photometric_loss(img, s["images"], 0.2))
        img, hd, ho = _render(s["held"], s["Kh"], out)
        m = (ho[0] > 0.5) & (s["held_opacity"] > 0.5)
        ref = s["held_depth"][m] / s["held_opacity"][m]
        absrel = float(((hd[0][m] / ho[0][m] - ref).abs() / ref).mean())
        return term, photo, _psnr(img[0], s["held_image"]), absrel

    t0, f0, p0, a0 = report(s["start"])
    ts, fs, ps, as_ = report(with_term)
    tp, fp, pp, ap = report(photo_only)
    print(f"\nrefine with smoothness (weight {w}): objective {l_s[0]:.5f} -> {l_s[-1]:.5f}, term {sl[0]:.5f} -> {sl[-1]:.5f}; photometric only {l_p[0]:.5f} -> {l_p[-1]:.5f}\n"
          f"term of the final training renders: start {t0:.5f}, with smoothness {ts:.5f}, photometric only {tp:.5f}\n"
          f"held-out PSNR: start {p0:.3f} dB, with smoothness {ps:.3f} dB, photometric only {pp:.3f} dB; "
          f"held-out AbsRel of depth / opacity where opacity > 0.5: start {a0:.5f}, with smoothness {as_:.5f}, photometric only {ap:.5f}")
    # the first logged objective is photometric + w * term of the starting render: both parts recomputed here (float32 sums of three numbers)
    assert abs(sl[0] - t0) <= 1e-5 * t0
    assert abs(l_s[0] - (f0 + w * sl[0])) <= 1e-5 * l_s[0]
    # at every logged iteration the objective is the photometric part (between 0 and 1, and the photometric-only run's at iteration 0) + w * term
    photo = [t - w * x for t, x in zip(l_s, sl)]
    assert all(0.0 < p < 1.0 for p in photo) and abs(photo[0] - l_p[0]) <= 1e-5
    assert ts < t0 and ts < tp and sl[-1] < sl[0]


def test_schedule_runs_and_logs_agree(scene):
    from siu3r_amd.refine import depth_weight_schedule, refine_gaussians
    from siu3r_amd.smooth import DepthSmoothness

    s = scene
    control = DepthSmoothness(weight=(2.0, 0.02))
    out, total = refine_gaussians(*_args(s), iters=10, smooth=control, segments=s["segments"])
    _, plain = refine_gaussians(*_args(s), iters=1)
    lam, sl = control.weights(10), out["smooth_losses"]
    assert lam == depth_weight_schedule((2.0, 0.02), 10) and lam[0] == 2.0 and lam[-1] == 0.02
    assert len(total) == len(sl) == 10 and all(np.isfinite(total)) and all(x > 0 for x in sl)
    photo = [t - l * x for t, l, x in zip(total, lam, sl)]
    print(f"\nschedule: objective {total[0]:.5f} .. {total[-1]:.5f}, term {sl[0]:.5f} .. {sl[-1]:.5f}, photometric part {photo[0]:.5f} .. {photo[-1]:.5f}")
    assert all(0.0 < p < 1.0 for p in photo) and abs(photo[0] - plain[0]) <= 1e-5


def test_second_order_expected_depth_beside_a_depth_term(scene):
    from siu3r_amd.refine import refine_gaussians
    from siu3r_amd.smooth import DepthSmoothness

    s = scene
    out, total = refine_gaussians(*_args(s), iters=10, smooth=DepthSmoothness(weight=0.5, order=2, space="expected"), segments=s["segments"],
                                  depths=s["depths"], lambda_depth=1.0, optimizer="hip")
    sl, dl = out["smooth_losses"], out["depth_losses"]
    assert len(total) == len(sl) == len(dl) == 10 and out["optimizer_steps"] == 10
    assert all(np.isfinite(total)) and all(x > 0 for x in sl) and all(x > 0 for x in dl)
    photo = [t - 0.5 * x - d for t, x, d in zip(total, sl, dl)]
    assert all(0.0 < p < 1.0 for p in photo), photo
    ungated, _ = refine_gaussians(*_args(s), iters=2, smooth=DepthSmoothness(order=2))  # no segments: plain smoothness
    assert len(ungated["smooth_losses"]) == 2 and all(x > 0 for x in ungated["smooth_losses"])
    for k in FIELDS:
        assert bool(torch.isfinite(out[k]).all()) and bool(torch.isfinite(ungated[k]).all())


def test_one_density_event_with_smoothness(scene):
    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import covariances_from, refine_gaussians
    from siu3r_amd.smooth import DepthSmoothness

    s = scene
    control = DensityControl(grad_threshold=2e-5, start=5, every=5, stop=6, scene_extent=5.0)
    out, total = refine_gaussians(*_args(s), iters=10, smooth=DepthSmoothness(weight=1.0), segments=s["segments"], density=control)
    ev = out["density_events"]
    assert [e["iteration"] for e in ev] == [5]
    n = ev[0]["rows_out"]
    print(f"\ndensity event with smoothness: {ev[0]}")
    assert ev[0]["rows_in"] == 20000 and n == 20000 + ev[0]["cloned"] + ev[0]["split"] - ev[0]["pruned"]
    for k in FIELDS:
        assert out[k].shape[0] == n and bool(torch.isfinite(out[k]).all())
    assert out["covariances"].shape == (n, 3, 3) and torch.equal(out["covariances"], covariances_from(out["rotations"], out["scales"]))
    assert len(total) == len(out["smooth_losses"]) == 10 and all(np.isfinite(total)) and all(np.isfinite(out["smooth_losses"]))


def test_switched_off_path_never_calls_depth_smoothness(scene, monkeypatch):
    from siu3r_amd import losses, refine
    from siu3r_amd.smooth import DepthSmoothness

    s = scene
    zero_a, _ = refine.refine_gaussians(*_args(s), iters=0)
    one_a, la = refine.refine_gaussians(*_args(s), iters=1)

    def boom(*a, **k):
        raise AssertionError("depth_smoothness was called on the switched-off path")

    monkeypatch.setattr(losses, "depth_smoothness", boom)
    monkeypatch.setattr(refine, "depth_smoothness", boom)
    zero_b, _ = refine.refine_gaussians(*_args(s), iters=0, smooth=None, segments=None)
    one_b, lb = refine.refine_gaussians(*_args(s), iters=3, smooth=None)
    assert len(lb) == 3 and "smooth_losses" not in one_b and set(zero_a) == set(zero_b)
    assert all(torch.equal(zero_a[k], zero_b[k]) for k in zero_a)  # iters = 0 and the first logged loss: the same bits as without the keyword
    assert la[0] == lb[0]
    with pytest.raises(AssertionError, match="switched-off"):
        refine.refine_gaussians(*_args(s), iters=2, smooth=DepthSmoothness())


def test_error_paths(scene, monkeypatch):
    from siu3r_amd import refine
    from siu3r_amd.smooth import DepthSmoothness

    def boom(*a, **k):
        raise AssertionError("device work was reached")

    monkeypatch.setattr(refine, "render_cuda", boom)
    s = scene
    run = lambda **kw: refine.refine_gaussians(*_args(s), iters=2, **kw)
    with pytest.raises(ValueError, match="segments without"):
        run(segments=s["segments"])
    for bad in (0.0, -1.0, float("inf"), float("nan"), (1.0, 0.0), (0.0, 1.0), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="weight"):
            run(smooth=DepthSmoothness(weight=bad))
    with pytest.raises(ValueError, match="order"):
        run(smooth=DepthSmoothness(order=3))
    with pytest.raises(ValueError, match="space"):
        run(smooth=DepthSmoothness(space="inverse"))
    with pytest.raises(ValueError, match="min_opacity"):
        run(smooth=DepthSmoothness(min_opacity=-1.0))
    with pytest.raises(ValueError, match="segments must be"):
        run(smooth=DepthSmoothness(), segments=s["segments"][:1])
    with pytest.raises(ValueError, match="integer"):
        run(smooth=DepthSmoothness(), segments=s["segments"] > 0)
    with pytest.raises(ValueError, match="DepthSmoothness"):
        run(smooth=1.0)
    with pytest.raises(AssertionError, match="device work"):
        run(smooth=DepthSmoothness(), segments=s["segments"])
