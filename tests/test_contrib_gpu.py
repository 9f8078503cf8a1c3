"""siu3r_raster_contrib (siu3r_amd/csrc/contrib.hip) and its front ends on the GPU.

  1  the entry point on the crafted cases of tests/dense_contrib64.py (a footprint over four tiles, an opaque front wall, the alpha_max
     clamp, culled and off-frame rows, 700 Gaussians over one tile = two refill-and-walk rounds, G == 0), both families, records and bins
     made by the reference stages, against the float64 windows proved by tests/test_contrib_ref.py
  2  bit-equality with the forward's own weights, no tolerance: identity features through the 32-channel K3 composite (output channel g of
     a pixel is that pixel's w_g: fmaf(1, w, 0) and fmaf(0, w, C) are exact) and one-hot precomputed colours through the K2 composite
  3  reproducibility: two calls, and ContributionStats over any chunking of the views, give identical bits
  4  the overflow rule: a NaN wmax row for the view that overflowed an unchecked call, a transparent repeat by default
  5  the documented errors"""
import numpy as np
import pytest
import torch

import dense_contrib64 as K
from test_raster_bwd_stages_gpu import _cam_blocks, _composite_state, _ok, _p, _refused
from test_raster_stages_gpu import _Guarded

pytestmark = pytest.mark.gpu


def _contrib(c, st, want_count=True, want_sum=True):
    V, G = c["V"], c["G"]
    wmax = _Guarded((V, G), torch.float32)
    count = _Guarded((V, G), torch.int32) if want_count else None
    wsum = _Guarded((V, G), torch.int64) if want_sum else None
    _ok("siu3r_raster_contrib", st["arr"], V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(wmax), _p(count),
        _p(wsum))
    for b in (wmax, count, wsum):
        assert b is None or b.guards_intact(), "written outside the buffer"
    return wmax.t, None if count is None else count.t, None if wsum is None else wsum.t


# ---- 1: the entry point against the float64 windows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NEW_NAMES)
def test_entry_point_inside_the_windows(name):
    c = K.contrib_case(name)
    st = _composite_state(c)
    wmax, count, wsum = _contrib(c, st)
    worst = K.check_contrib(name, c, wmax.cpu().numpy(), count.cpu().numpy(), wsum.cpu().numpy())
    print(f"[contrib] {name}: worst wsum error {worst:.3f} of its tolerance")
    # the optional outputs: NULL = not wanted, the others unchanged
    only_max, no_count, no_sum = _contrib(c, st, False, False)
    assert no_count is None and no_sum is None and torch.equal(only_max.view(torch.int32), wmax.view(torch.int32))


def test_no_gaussians():
    c = K.contrib_case("k2_span4")
    arr, cams_dev = _cam_blocks(c["cams"])
    _ok("siu3r_raster_contrib", arr, c["V"], _p(cams_dev), 0, None, None, 16, None, None, None, None)
    _ok("siu3r_raster_contrib", arr, c["V"], None, 0, None, None, 0, None, None, None, None)


# ---- world-space scenes for the front ends ---------------------------------------------------------------------------------------------------
def _scene(kind, which):
    """-> cams (host poses), means, cov6, opacities (GPU), and for the refinement-style calls scales, rotations (x, y, z, w), c2w, Kn"""
    from siu3r_amd import raster

    rng = np.random.default_rng(sum(map(ord, kind + which)))
    crowd = which == "crowd"
    W, H, V = (16, 16, 1) if crowd else (40, 24, 2)
    fx, fy, cx, cy = (W / 1.4, H / 0.9, (W - 1) / 2, (H - 1) / 2) if kind == "k2" else (70.0, 55.0, 0.35 * W, 0.6 * H)
    if crowd:
        n = K.CROWD_G
        px, py, sg, op, z = rng.uniform(1, 15, n), rng.uniform(1, 15, n), rng.uniform(1.5, 3.0, n), rng.uniform(0.005, 0.012, n), 2.0 + 1e-3 * rng.permutation(n)
    else:
        px = np.concatenate([rng.uniform(-2, W + 2, 60), [16.0, 16.2, 15.8], np.full(6, 8.0), rng.uniform(1, 9, 14), rng.uniform(-80, -60, 4)])
        py = np.concatenate([rng.uniform(-2, H + 2, 60), [16.0, 15.9, 16.1], np.full(6, 12.0), rng.uniform(2, H - 2, 14), rng.uniform(0, H, 4)])
        sg = np.concatenate([rng.uniform(0.8, 2.5, 60), [3.0, 3.0, 3.0], np.full(6, 7.0), np.full(14, 0.6), np.full(4, 1.0)])
        op = np.concatenate([rng.uniform(0.05, 0.9, 60), [0.7, 0.999, 0.2], np.full(6, 0.95), rng.uniform(0.3, 0.9, 14), np.full(4, 0.8)])
        z = np.concatenate([rng.uniform(2.0, 3.0, 60), [1.5, 1.6, 1.7], 1.0 + 0.01 * np.arange(6), rng.uniform(3.5, 4.0, 14), rng.uniform(2, 3, 4)])
    means = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], -1)
    s = sg * z / fx
    G = means.shape[0]
    cov6 = np.zeros((G, 6))
    cov6[:, 0] = cov6[:, 3] = cov6[:, 5] = s * s
    c2ws = [torch.eye(4, dtype=torch.float64) for _ in range(V)]
    for v in range(1, V):
        c2ws[v][0, 3] = 0.15 * v
    if kind == "k2":
        import dense_raster_bwd64 as B

        cams = [B.k2_cam(W, H, c, deg=-1) for c in c2ws]
        for cam in cams:
            cam.bg[0] = cam.bg[1] = cam.bg[2] = 0.0
    else:
        cams = [raster.make_cam_k3(torch.linalg.inv(c).float(), fx, fy, cx, cy, W, H) for c in c2ws]
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32).cuda()
    rot = torch.zeros((G, 4), device="cuda")
    rot[:, 3] = 1.0
    Kn = torch.tensor([[fx / W, 0, (cx + 0.5) / W], [0, fy / H, (cy + 0.5) / H], [0, 0, 1]], dtype=torch.float32).cuda()
    return dict(W=W, H=H, V=V, G=G, cams=cams, means=f(means), cov6=f(cov6), opac=f(op), scales=f(np.repeat(s[:, None], 3, 1)), rot=rot,
                c2w=torch.stack(c2ws).float().cuda(), Kn=Kn)


def _stats_of_weights(wmaps):
    """wmaps [V, P, G] f32: pixel p's blending weight of Gaussian g -> the three statistics in the kernel's definitions"""
    wmax = wmaps.amax(1)
    count = (wmaps != 0).sum(1).to(torch.int32)
    wsum = torch.floor(wmaps.double() * 2.0 ** 40).to(torch.int64).sum(1)
    return wmax, count, wsum


def _equal_bits(got, ref, what):
    for k, r in zip(("wmax", "count", "wsum"), ref):
        g = got[k]
        same = torch.equal(g.view(torch.int32), r.view(torch.int32)) if k == "wmax" else torch.equal(g, r)
        assert same, f"{what}: {k} differs from the forward's own weights in {int((g != r).sum())} rows"


# ---- 2: bit-equality with the forward's own weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mix", "crowd"])
def test_k3_equals_the_forward_weights(which):
    from siu3r_amd import raster

    s = _scene("k3", which)
    raster.tune(0, 1)  # the 32-channel kernel: a pixel only ever sees the rows that blend into it, in fused multiply-adds
    try:
        out = raster.rasterize_views_k3(s["cams"], s["means"], s["cov6"], s["opac"], torch.eye(s["G"], device="cuda"))
    finally:
        raster.tune(0, 0)
    ref = _stats_of_weights(out["colors"].reshape(s["V"], -1, s["G"]))
    got = raster.contributions_k3(s["cams"], s["means"], s["cov6"], s["opac"])
    assert int(ref[1].sum()) > 0
    _equal_bits(got, ref, f"k3 {which}")
    if which == "crowd":
        assert int((ref[1] > 0).sum()) > 512, "more than STG survivors blend: the accumulators are flushed in two rounds"


@pytest.mark.parametrize("which", ["mix", "crowd"])
def test_k2_equals_the_forward_weights(which):
    from siu3r_amd import raster

    s = _scene("k2", which)
    V, G = s["V"], s["G"]
    wmaps = torch.zeros((V, s["H"] * s["W"], G), device="cuda")
    for g0 in range(0, G, 3):  # three one-hot Gaussians per render: colour channel c of a pixel is exactly its w of Gaussian g0 + c
        shs = torch.zeros((G, 1, 3), device="cuda")
        for ch in range(min(3, G - g0)):
            shs[g0 + ch, 0, ch] = 1.0
        img = raster.rasterize_views_k2(s["cams"], s["means"], s["cov6"], shs, s["opac"], want_n_touched=False, check_overflow=False)["image"]
        n = min(3, G - g0)
        wmaps[:, :, g0:g0 + n] = img.reshape(V, 3, -1)[:, :n].permute(0, 2, 1)
    ref = _stats_of_weights(wmaps)
    got = raster.contributions_k2(s["cams"], s["means"], s["cov6"], s["opac"])
    assert int(ref[1].sum()) > 0
    _equal_bits(got, ref, f"k2 {which}")


# ---- 3: reproducibility ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["k2", "k3"])
def test_two_calls_give_identical_bits(kind):
    from siu3r_amd import raster

    s = _scene(kind, "mix")
    call = raster.contributions_k2 if kind == "k2" else raster.contributions_k3
    a, b = (call(s["cams"], s["means"], s["cov6"], s["opac"]) for _ in range(2))
    _equal_bits(a, (b["wmax"], b["count"], b["wsum"]), kind)
    assert a["count"].dtype == torch.int32 and a["wsum"].dtype == torch.int64 and a["wmax"].dtype == torch.float32
    assert tuple(a["radii"].shape) == (s["V"], s["G"], 2) and a["state"] is not None


def test_any_chunking_of_the_views_gives_identical_statistics():
    from siu3r_amd import prune

    s = _scene("k2", "mix")
    c2w = torch.cat([s["c2w"], s["c2w"][:1]])  # three views
    c2w[2, 1, 3] = 0.1
    args = (s["means"], s["scales"], s["rot"], s["opac"], c2w, s["Kn"], 0.2, 100.0, (s["H"], s["W"]))
    whole, single, pairs = (prune.gaussian_contributions(*args, view_chunk=n) for n in (8, 1, 2))
    assert int(whole.count.sum()) > 0 and int(whole.views.max()) == 3
    for other in (single, pairs):
        assert torch.equal(whole.wmax.view(torch.int32), other.wmax.view(torch.int32)) and torch.equal(whole.wsum, other.wsum)
        assert torch.equal(whole.count, other.count) and torch.equal(whole.views, other.views)
    assert whole.weight_sum().dtype == torch.float64 and torch.equal(whole.weight_sum(), whole.wsum.double() * 2.0 ** -40)


# ---- 4: overflow -----------------------------------------------------------------------------------------------------------------------------
def test_overflow_poisons_that_view_only_and_the_default_path_repeats():
    from siu3r_amd import raster

    s = _scene("k2", "mix")
    cams = list(s["cams"])
    import dense_raster_bwd64 as B

    away = torch.eye(4, dtype=torch.float64)
    away[0, 3] = 2.5  # view 0 moved aside: it sees only a few of the Gaussians
    cams[0] = B.k2_cam(s["W"], s["H"], away, deg=-1)
    free = raster.contributions_k2(cams, s["means"], s["cov6"], s["opac"])
    E = free["state"].totals(2)
    assert E[0] < E[1] - 1, E
    cap = (E[0] + E[1]) // 2
    tight = raster.contributions_k2(cams, s["means"], s["cov6"], s["opac"], entry_capacity=cap, check_overflow=False)
    assert bool(torch.isnan(tight["wmax"][1]).all()) and int(tight["count"][1].abs().sum()) == 0 and int(tight["wsum"][1].abs().sum()) == 0
    for k in ("wmax", "count", "wsum"):
        assert torch.equal(tight[k][0], free[k][0]), f"{k}: the view that fits is not touched by the other's overflow"
    with pytest.raises(raster.RasterOverflow):
        tight["state"].verify()
    again = raster.contributions_k2(cams, s["means"], s["cov6"], s["opac"], entry_capacity=cap)
    _equal_bits(again, (free["wmax"], free["count"], free["wsum"]), "repeat after overflow")


# ---- 5: error paths --------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    from siu3r_amd import raster
    from siu3r_amd.mcmc import MCMCControl
    from siu3r_amd.prune import ContributionPrune
    from siu3r_amd.refine import refine_gaussians

    c, c3 = K.contrib_case("k2_span4"), K.contrib_case("k3_span4")
    st = _composite_state(c)
    V, G = c["V"], c["G"]
    outs = [_Guarded((V, G), torch.float32), _Guarded((V, G), torch.int32), _Guarded((V, G), torch.int64)]
    base = lambda arr=st["arr"], wmax=outs[0], V=V: [arr, V, _p(st["cams_dev"]), G, _p(st["bin_start"]), _p(st["entries"]), st["cap_e"], _p(st["rec"]), _p(wmax),
                                                     _p(outs[1]), _p(outs[2])]
    mixed = raster._cam_array([c["cams"][0], c3["cams"][1]])
    _refused("siu3r_raster_contrib", "one family", *base(arr=mixed), outs=outs)
    _refused("siu3r_raster_contrib", "null pointer", *base(wmax=None), outs=outs)
    _refused("siu3r_raster_contrib", "bad view array", *base(V=0), outs=outs)
    z = torch.zeros
    scene = (z(4, 3), z(4, 3), z(4, 4), z(4), z(4, 3, 1), z(2, 3, 8, 8), z(2, 4, 4), z(3, 3), 0.1, 10.0, (0, 0, 0))  # (CPU tensors: nothing may reach a device)
    with pytest.raises(ValueError, match="MCMCControl"):
        refine_gaussians(*scene, iters=4, density=MCMCControl(cap_max=8), prune=ContributionPrune())
    with pytest.raises(ValueError, match="every must be positive"):
        refine_gaussians(*scene, iters=4, prune=ContributionPrune(every=0))
