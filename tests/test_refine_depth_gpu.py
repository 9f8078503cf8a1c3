"""refine.refine_gaussians with a depth term (losses.depth_loss, csrc/depth_loss.hip): the term goes down, the switched-off path never
reaches it, the schedule and the logs agree, and density control runs beside it.  Scenes as tests/test_refine_gpu.py builds them."""
import numpy as np
import pytest
import torch

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
    """the truth, its training targets (views 0 and 1: images, depth / opacity, confidence) and the held-out view 4; computed once, read only"""
    truth = _truth()
    train, Kt = _cams([0, 1])
    held, Kh = _cams([4])
    images, depth, opacity = _render(train, Kt, truth)
    held_image, held_depth, held_opacity = _render(held, Kh, truth)
    conf = (opacity > 0.5).float()
    targets = torch.where(opacity > 0.5, depth / opacity.clamp_min(1e-6), torch.zeros_like(depth))
    return dict(truth=truth, start=_perturbed(truth), train=train, Kt=Kt, held=held, Kh=Kh, images=images, depths=targets, conf=conf,
                held_image=held_image[0], held_depth=held_depth[0], held_opacity=held_opacity[0])


def test_depth_term_goes_down_and_beats_the_photometric_run(scene):
    from siu3r_amd import losses
    from siu3r_amd.refine import refine_gaussians

    s = scene
    args = (*(s["start"][k] for k in FIELDS), s["images"], s["train"], s["Kt"], NEAR, FAR, BG)
    with_depth, l_d = refine_gaussians(*args, iters=60, depths=s["depths"], depth_weights=s["conf"], lambda_depth=1.0)
    photo_only, l_p = refine_gaussians(*args, iters=60)
    dl = with_depth["depth_losses"]
    assert len(l_d) == len(dl) == len(l_p) == 60 and "depth_losses" not in photo_only
    assert all(np.isfinite(l_d)) and all(np.isfinite(dl)) and all(np.isfinite(l_p))
    assert dl[-1] < dl[0]

    def report(out):
        _, d, o = _render(s["train"], s["Kt"], out)
        term = float(losses.depth_loss(d, o, s["depths"], s["conf"]))
        img, hd, ho = _render(s["held"], s["Kh"], out)
        m = (ho[0] > 0.5) & (s["held_opacity"] > 0.5)
        ref = s["held_depth"][m] / s["held_opacity"][m]
        absrel = float(((hd[0][m] / ho[0][m] - ref).abs() / ref).mean())
        return term, _psnr(img[0], s["held_image"]), absrel

    t0, p0, a0 = report(s["start"])
    td, pd, ad = report(with_depth)
    tp, pp, ap = report(photo_only)
    print(f"\nrefine with depth: objective {l_d[0]:.5f} -> {l_d[-1]:.5f}, depth term {dl[0]:.5f} -> {dl[-1]:.5f}; photometric only {l_p[0]:.5f} -> {l_p[-1]:.5f}\n"
          f"final depth term of the training renders: start {t0:.5f}, with depth {td:.5f}, photometric only {tp:.5f}\n"
          f"held-out PSNR: start {p0:.3f} dB, with depth {pd:.3f} dB, photometric only {pp:.3f} dB; "
          f"held-out AbsRel of depth / opacity where opacity > 0.5: start {a0:.5f}, with depth {ad:.5f}, photometric only {ap:.5f}")
    assert td < tp


def test_switched_off_path_never_calls_depth_loss(scene, monkeypatch):
    from siu3r_amd import losses, refine

    def boom(*a, **k):
        raise AssertionError("depth_loss was called on the switched-off path")

    monkeypatch.setattr(losses, "depth_loss", boom)
    monkeypatch.setattr(refine, "depth_loss", boom)
    s = scene
    args = (*(s["start"][k] for k in FIELDS), s["images"], s["train"], s["Kt"], NEAR, FAR, BG)
    a, la = refine.refine_gaussians(*args, iters=2)
    b, lb = refine.refine_gaussians(*args, iters=2, depths=s["depths"], depth_weights=s["conf"], lambda_depth=0.0)
    assert len(la) == len(lb) == 2 and "depth_losses" not in a and "depth_losses" not in b
    assert set(a) == set(b) and all(a[k].shape == b[k].shape for k in a)
    with pytest.raises(AssertionError, match="switched-off"):
        refine.refine_gaussians(*args, iters=2, depths=s["depths"], lambda_depth=0.5)


def test_schedule_and_logs_agree(scene):
    from siu3r_amd.refine import depth_weight_schedule, refine_gaussians

    s = scene
    out, total = refine_gaussians(*(s["start"][k] for k in FIELDS), s["images"], s["train"], s["Kt"], NEAR, FAR, BG, iters=10, depths=s["depths"],
                                  depth_weights=s["conf"], lambda_depth=(1.0, 0.01), depth_mode="pearson", depth_space="inverse")
    lam, dl = depth_weight_schedule((1.0, 0.01), 10), out["depth_losses"]
    assert len(total) == len(dl) == 10 and lam[0] == 1.0 and lam[-1] == 0.01
    photo = [t - l * d for t, l, d in zip(total, lam, dl)]
    print(f"\nschedule: objective {total[0]:.5f} .. {total[-1]:.5f}, pearson term {dl[0]:.5f} .. {dl[-1]:.5f}, photometric part {photo[0]:.5f} .. {photo[-1]:.5f}")
    assert all(np.isfinite(total)) and all(0.0 <= d <= 2.0 for d in dl)
    assert all(0.0 < p < 1.0 for p in photo), photo


def test_one_density_event_with_depths(scene):
    from siu3r_amd.density import DensityControl
    from siu3r_amd.refine import covariances_from, refine_gaussians

    s = scene
    control = DensityControl(grad_threshold=2e-5, start=5, every=5, stop=6, scene_extent=5.0)
    out, total = refine_gaussians(*(s["start"][k] for k in FIELDS), s["images"], s["train"], s["Kt"], NEAR, FAR, BG, iters=10, depths=s["depths"],
                                  depth_weights=s["conf"], lambda_depth=1.0, density=control)
    ev = out["density_events"]
    assert [e["iteration"] for e in ev] == [5]
    n = ev[0]["rows_out"]
    print(f"\ndensity event with depths: {ev[0]}")
    assert ev[0]["rows_in"] == 20000 and n == 20000 + ev[0]["cloned"] + ev[0]["split"] - ev[0]["pruned"]
    for k in FIELDS:
        assert out[k].shape[0] == n and bool(torch.isfinite(out[k]).all())
    assert out["covariances"].shape == (n, 3, 3) and torch.equal(out["covariances"], covariances_from(out["rotations"], out["scales"]))
    assert len(total) == len(out["depth_losses"]) == 10 and all(np.isfinite(total)) and all(np.isfinite(out["depth_losses"]))
