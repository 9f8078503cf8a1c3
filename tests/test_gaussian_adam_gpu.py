"""The fused visibility-aware Adam (siu3r_amd/optim.py::GaussianAdam, csrc/gaussian_adam.hip) on the GPU against tests/dense_adam64.py.

Tolerance of the accuracy tests (the rule of tests/test_depth_loss_gpu.py): HIP, the float64 restatement and the composed float32 torch
restatement (on the CPU) get the SAME float32 inputs for ONE step.  Per field, the HIP error against float64 is measured on the step
p_new - p_old, on exp_avg and on exp_avg_sq, each max-normalised; it may be at most 2 x the composed float32 error, with a floor of 1e-6.
Where the reference is exactly zero the HIP result must be exactly zero.

Shapes: a workgroup of the kernel as built covers 1,024 consecutive floats of ONE field per round (256 threads x 4 floats), and at most
2,048 workgroups are launched.  G = 341 / 342 straddle 1,024 floats of a 3-wide field, G = 1023 / 1024 / 1025 are one below, at and one
above one workgroup of the 1-wide field (opacities); G = 40000 with n = 16 has 2,305 chunks, more than one round of the capped grid."""
import math

import pytest
import torch

import dense_adam64 as A

pytestmark = pytest.mark.gpu

FIELDS = ("means", "scales", "rotations", "opacities", "harmonics")
STATES = ("fresh", "t2", "t1000")
SH_SCALE = 0.05


def _inputs(G, n, kind, state, names=FIELDS, seed=0):
    """{field: (p, g, m, v)} float32 on the CPU, and t"""
    out, t = {}, None
    for i, k in enumerate(names):
        *x, t = A.make_field(kind, (G, *A.FIELD_WIDTHS(n)[k]), seed + 17 * i + G, state)
        out[k] = tuple(x)
    return out, t


def _place(x, offset):
    """x on the GPU; offset: as a contiguous slice starting `offset` floats into its storage (a base that is only 4-byte aligned)"""
    if not offset:
        return x.cuda()
    buf = torch.empty(x.numel() + offset, dtype=x.dtype, device="cuda")
    view = buf[offset:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view


def _optimizer(inputs, t, offsets=(0, 0, 0, 0)):
    from siu3r_amd.optim import GaussianAdam

    params = {k: _place(x[0], offsets[0]).requires_grad_(True) for k, x in inputs.items()}
    opt = GaussianAdam(params, {k: A.LRS[k] for k in inputs}, sh_rest_lr_scale=SH_SCALE)
    opt.rebind(params, {k: (_place(x[2], offsets[2]), _place(x[3], offsets[3])) for k, x in inputs.items()})
    for k, x in inputs.items():
        params[k].grad = _place(x[1], offsets[1])
    opt.step_count = t - 1
    return opt


def _hip(inputs, t, visible=None, offsets=(0, 0, 0, 0)):
    """one GaussianAdam.step from the given state -> {field: (p, m, v)} on the CPU"""
    opt = _optimizer(inputs, t, offsets)
    grads = {k: p.grad.clone() for k, p in opt.params.items()}
    opt.step(visible=None if visible is None else visible.cuda())
    assert opt.step_count == t
    for k, p in opt.params.items():
        assert torch.equal(p.grad.view(torch.int32), grads[k].view(torch.int32)), f"{k}: the gradient was written"
    return {k: (opt.params[k].detach().cpu(), opt.moments[k][0].cpu(), opt.moments[k][1].cpu()) for k in inputs}


def _ref(inputs, t, visible, dtype):
    out = {}
    for k, (p, g, m, v) in inputs.items():
        sh = k == "harmonics"
        out[k] = A.step(p, g, m, v, t, A.LRS[k], A.LRS[k] * SH_SCALE if sh else None, p.shape[-1] if sh else 0, visible=visible, dtype=dtype)
    return out


def _err(got, ref):
    """max-normalised error of `got` against the float64 `ref`; exact zeros of the reference must be exact zeros"""
    got = got.double()
    scale, diff = float(ref.abs().max()), float((got - ref).abs().max())
    return diff / scale if scale > 0 else (0.0 if diff == 0.0 else math.inf)


def _compare(tag, inputs, t, visible=None, offsets=(0, 0, 0, 0)):
    ref, cmp_ = _ref(inputs, t, visible, torch.float64), _ref(inputs, t, visible, torch.float32)
    hip = _hip(inputs, t, visible, offsets)
    vis = A.visible_rows(visible, next(iter(inputs.values()))[0].shape[0])
    lines = []
    for k, (p, _, m, v) in inputs.items():
        old = (p.double(), m.double(), v.double())
        for q, name in enumerate(("step", "exp_avg", "exp_avg_sq")):
            r = ref[k][q] - old[0] if q == 0 else ref[k][q]
            h = hip[k][q].double() - old[0] if q == 0 else hip[k][q].double()
            c = cmp_[k][q].double() - old[0] if q == 0 else cmp_[k][q].double()
            e_hip, e_cmp = _err(h, r), _err(c, r)
            lines.append(f"{k}.{name} composed-f32 {e_cmp:.2e} hip {e_hip:.2e}")
            assert not bool(h[r == 0].any()), f"{tag} {k}.{name}: the reference is exactly zero where hip is not"
            assert e_hip <= max(2.0 * e_cmp, 1e-6), f"{tag} {k}.{name}: hip error {e_hip:.3e} > max(2 x composed float32 error {e_cmp:.3e}, 1e-6)"
            assert torch.equal(hip[k][q][~vis], (p, m, v)[q][~vis]), f"{tag} {k}.{name}: an invisible row changed"
    print(f"\n{tag}: {int(vis.sum())} of {len(vis)} rows visible; " + "; ".join(lines))
    return hip


def _visibilities(G, seed):
    """(tag, visible) for: dense, radii of 1 and 3 views with about half the rows visible, a uint8 mask"""
    r1, _ = A.make_radii(G, 1, seed)
    r3, _ = A.make_radii(G, 3, seed + 1)
    mask = (torch.rand(G, generator=torch.Generator().manual_seed(seed + 2)) < 0.5).to(torch.uint8)
    return [("dense", None), ("radii V=1", r1), ("radii V=3", r3), ("mask", mask)]


@pytest.mark.parametrize("n", [1, 4, 16, 25])
@pytest.mark.parametrize("G", [1, 2, 341, 342, 1023, 1024, 1025, 1365, 4097])
def test_five_fields_against_float64(G, n):
    kind = "noise" if (G + n) % 2 else "render"
    for state in STATES:
        inputs, t = _inputs(G, n, kind, state)
        for tag, visible in _visibilities(G, G + n):
            _compare(f"{kind} {state} G={G} n={n} {tag}", inputs, t, visible)


def test_more_chunks_than_workgroups():
    inputs, t = _inputs(40000, 16, "render", "t2")
    _compare("render t2 G=40000 n=16 dense", inputs, t)
    _compare("render t2 G=40000 n=16 radii V=3", inputs, t, A.make_radii(40000, 3, 9)[0])


@pytest.mark.parametrize("field,n", [("harmonics", 25), ("harmonics", 16), ("opacities", 1), ("rotations", 1)])
@pytest.mark.parametrize("G", [1, 341, 1025, 4097])
def test_one_field_table(G, field, n):
    inputs, t = _inputs(G, n, "noise", "t1000", names=(field,))
    for tag, visible in _visibilities(G, G)[:2]:
        _compare(f"one field {field} G={G} n={n} {tag}", inputs, t, visible)


@pytest.mark.parametrize("offsets", [(1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 3, 0), (0, 0, 0, 2)])
@pytest.mark.parametrize("G,n", [(342, 4), (1365, 25)])
def test_bases_that_are_only_four_byte_aligned(G, n, offsets):
    """every tensor, or one of the four, is a contiguous slice starting 1 .. 3 floats into its storage: the scalar path, the same bits"""
    inputs, t = _inputs(G, n, "noise", "t2")
    for tag, visible in _visibilities(G, 3)[::2]:
        hip = _compare(f"offsets {offsets} G={G} n={n} {tag}", inputs, t, visible, offsets)
        aligned = _hip(inputs, t, visible)
        for k in inputs:
            assert all(torch.equal(a, b) for a, b in zip(hip[k], aligned[k])), k


def test_no_visible_row_changes_nothing():
    G = 1365
    inputs, t = _inputs(G, 4, "noise", "t2")
    for visible in (torch.zeros(2, G, 2, dtype=torch.int32), -torch.ones(1, G, 2, dtype=torch.int32), torch.zeros(G, dtype=torch.uint8),
                    torch.zeros(G, dtype=torch.bool)):
        opt = _optimizer(inputs, t)
        before = {k: (p.detach().clone(), p.grad.clone(), *(m.clone() for m in opt.moments[k])) for k, p in opt.params.items()}
        opt.step(visible=visible.cuda())
        for k, p in opt.params.items():
            after = (p.detach(), p.grad, *opt.moments[k])
            assert all(torch.equal(a, b) for a, b in zip(after, before[k])), k
        assert opt.step_count == t


def test_all_rows_visible_through_radii_is_the_dense_step():
    G = 4097
    inputs, t = _inputs(G, 16, "render", "t1000")
    dense = _hip(inputs, t)
    radii = torch.zeros(3, G, 2, dtype=torch.int32)
    radii[torch.arange(G) % 3, torch.arange(G), torch.arange(G) % 2] = 1 + torch.arange(G, dtype=torch.int32) % 50
    assert bool(A.visible_rows(radii, G).all())
    for visible in (radii, torch.ones(G, dtype=torch.uint8), torch.full((G,), 255, dtype=torch.uint8), torch.ones(G, dtype=torch.bool)):
        got = _hip(inputs, t, visible)
        for k in inputs:
            assert all(torch.equal(a, b) for a, b in zip(got[k], dense[k])), k
    assert not torch.equal(dense["means"][0], inputs["means"][0])


@pytest.mark.parametrize("form", ["radii", "mask"])
def test_the_gradient_of_an_invisible_row_is_not_read(form):
    G = 1365
    inputs, t = _inputs(G, 25, "noise", "t2")
    radii, vis = A.make_radii(G, 3, seed=4)
    visible = radii if form == "radii" else vis
    clean = _hip(inputs, t, visible)
    poisoned = {k: (p, torch.where(vis.reshape((G,) + (1,) * (g.dim() - 1)), g, torch.full_like(g, float("nan"))), m, v) for k, (p, g, m, v) in inputs.items()}
    got = _hip(poisoned, t, visible)
    for k, (p, _, m, v) in inputs.items():
        for q, old in enumerate((p, m, v)):
            assert torch.equal(got[k][q], clean[k][q]) and bool(torch.isfinite(got[k][q]).all()), k
            assert torch.equal(got[k][q][~vis], old[~vis]), k
        assert not torch.equal(got[k][0][vis], p[vis]), k


def test_two_calls_give_identical_bits():
    G = 4097
    inputs, t = _inputs(G, 16, "render", "t2")
    for visible in (None, A.make_radii(G, 3, 8)[0]):
        a, b = _hip(inputs, t, visible), _hip(inputs, t, visible)
        for k in inputs:
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
            assert not torch.equal(a[k][0], inputs[k][0])


def test_non_finite_gradients_propagate_as_in_the_reference():
    G = 50
    inputs, t = _inputs(G, 4, "noise", "t2", names=("means", "harmonics"))
    for k in inputs:
        inputs[k][1].view(-1)[5], inputs[k][1].view(-1)[17], inputs[k][1].view(-1)[40] = float("nan"), float("inf"), -float("inf")
    ref, hip = _ref(inputs, t, None, torch.float64), _hip(inputs, t)
    for k in inputs:
        for q in range(3):
            assert torch.equal(torch.isnan(hip[k][q]), torch.isnan(ref[k][q])) and torch.equal(torch.isinf(hip[k][q]), torch.isinf(ref[k][q])), (k, q)
        assert int(torch.isnan(hip[k][0]).sum()) == 3  # (m / (sqrt(v) + eps) of an infinite gradient is inf / inf)


def test_carried_steps_a_rate_override_and_the_state_interface():
    from siu3r_amd.optim import GaussianAdam

    G = 342
    inputs, _ = _inputs(G, 4, "noise", "fresh")
    params = {k: x[0].cuda().requires_grad_(True) for k, x in inputs.items()}
    opt = GaussianAdam(params, A.LRS, sh_rest_lr_scale=SH_SCALE)
    ref = {k: (x[0].double(), x[2].double(), x[3].double()) for k, x in inputs.items()}
    assert opt.step_count == 0 and set(opt.moments) == set(FIELDS) and not any(bool(m.any()) or bool(v.any()) for m, v in opt.moments.values())
    for t in (1, 2, 3):
        radii, _ = A.make_radii(G, 2, seed=t)
        over = {"means": 7e-4} if t == 2 else None
        for k in FIELDS:
            g = A.make_field("noise", inputs[k][0].shape, 900 + t)[1]
            params[k].grad = g.cuda()
            sh = k == "harmonics"
            lr = over[k] if over and k in over else A.LRS[k]
            ref[k] = A.step(*ref[k][:1], g, *ref[k][1:], t, lr, lr * SH_SCALE if sh else None, 4 if sh else 0, visible=radii)
        opt.step(visible=radii.cuda(), lrs=over)
        assert opt.step_count == t and opt.lrs["means"] == A.LRS["means"]
    for k in FIELDS:
        assert float((params[k].detach().cpu().double() - ref[k][0]).abs().max()) <= 1e-5 * float(ref[k][0].abs().max()), k
    opt.zero_grad()
    assert all(p.grad is None for p in params.values())
    opt.zero_moments("opacities")
    assert not bool(opt.moments["opacities"][0].any()) and not bool(opt.moments["opacities"][1].any()) and bool(opt.moments["means"][0].any())
    # rebind: another row count, the step count stays
    smaller = {k: p.detach()[:100].clone().requires_grad_(True) for k, p in params.items()}
    opt.rebind(smaller, {k: (m[:100].clone(), v[:100].clone()) for k, (m, v) in opt.moments.items()})
    for p in smaller.values():
        p.grad = torch.ones_like(p)
    opt.step(visible=torch.ones(100, dtype=torch.bool, device="cuda"))
    assert opt.step_count == 4 and opt.G == 100 and not torch.equal(smaller["means"].detach(), params["means"].detach()[:100])


def test_step_does_not_synchronise():
    G = 1365
    inputs, t = _inputs(G, 4, "noise", "t2")
    radii = A.make_radii(G, 3, 1)[0].cuda()
    opt = _optimizer(inputs, t)
    opt.step(visible=radii)  # (warm: the workspace, the code object)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(visible=radii)
        opt.step()
        opt.step(lrs={"means": 1e-5})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.step_count == t + 3


def test_element_indices_past_32_bits():
    """One field of 2^32 + 1,024 floats, of which only rows at the start, around element 2^31 and around element 2^32 are visible (the
    invisible rows are never read, so nothing else is initialised): the bits of the same rows stepped as a small field, and sampled
    invisible rows untouched."""
    from siu3r_amd.optim import GaussianAdam

    W = 64
    G = (1 << 26) + 16
    free, _ = torch.cuda.mem_get_info()
    if free < 76 * (1 << 30):
        pytest.skip(f"needs 4 x 17 GB of device memory, {free / 2 ** 30:.0f} GB are free")
    rows = torch.tensor([0, 1, (1 << 25) - 1, 1 << 25, (1 << 26) - 1, 1 << 26, G - 1]).cuda()
    watch = torch.tensor([2, (1 << 25) + 1, G - 2]).cuda()  # invisible rows with known content
    t, lr = 2, 1e-2
    p, g, m, v, _ = A.make_field("noise", (len(rows), W), 77, "t2")
    try:
        big = [torch.empty((G, W), dtype=torch.float32, device="cuda") for _ in range(4)]
        for buf, x in zip(big, (p, g, m, v)):
            buf[rows] = x.cuda()
            buf[watch] = 3.25
        mask = torch.zeros(G, dtype=torch.uint8, device="cuda")
        mask[rows] = 1
        param = big[0].requires_grad_(True)
        opt = GaussianAdam({"big": param}, {"big": lr})
        opt.rebind({"big": param}, {"big": (big[2], big[3])})
        param.grad = big[1]
        opt.step_count = t - 1
        opt.step(visible=mask)
        small = p.cuda().requires_grad_(True)
        ref = GaussianAdam({"big": small}, {"big": lr})
        ref.rebind({"big": small}, {"big": (m.cuda(), v.cuda())})
        small.grad = g.cuda()
        ref.step_count = t - 1
        ref.step()
        for got, want in ((param.detach(), small.detach()), (big[2], ref.moments["big"][0]), (big[3], ref.moments["big"][1])):
            assert torch.equal(got[rows], want)
            assert bool((got[watch] == 3.25).all())
        assert not torch.equal(small.detach().cpu(), p)
    finally:
        big = param = opt = None
        torch.cuda.empty_cache()


def test_error_paths():
    from siu3r_amd.optim import GaussianAdam

    G = 16
    mk = lambda *s, **kw: torch.zeros(*s, device="cuda", **kw).requires_grad_(kw.get("dtype", torch.float32).is_floating_point)
    lrs = {"means": 1e-3, "harmonics": 1e-3}
    good = lambda: {"means": mk(G, 3), "harmonics": mk(G, 3, 4)}
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianAdam({"means": torch.zeros(G, 3, requires_grad=True)}, lrs)
    with pytest.raises(ValueError, match="float32"):
        GaussianAdam({"means": mk(G, 3, dtype=torch.float64)}, lrs)
    with pytest.raises(ValueError, match="rows"):
        GaussianAdam({"means": mk(G, 3), "harmonics": mk(G + 1, 3, 4)}, lrs)
    with pytest.raises(ValueError, match="contiguous"):
        GaussianAdam({"means": torch.zeros(3, G, device="cuda").t().requires_grad_(True)}, lrs)
    with pytest.raises(ValueError, match=r"\[G, 3, n\]"):
        GaussianAdam({"harmonics": mk(G, 12)}, lrs)
    with pytest.raises(ValueError, match="unknown field"):
        GaussianAdam(good(), dict(lrs, colours=1e-3))
    with pytest.raises(ValueError, match="no learning rate"):
        GaussianAdam(good(), {"means": 1e-3})
    with pytest.raises(ValueError, match=">= 0"):
        GaussianAdam(good(), dict(lrs, means=-1e-3))
    with pytest.raises(ValueError, match="fields"):
        GaussianAdam({f"f{i}": mk(G, 2) for i in range(9)}, {f"f{i}": 1e-3 for i in range(9)})
    with pytest.raises(ValueError, match="sh_rest_lr_scale"):
        GaussianAdam(good(), lrs, sh_rest_lr_scale=-1.0)
    opt = GaussianAdam(good(), lrs)
    with pytest.raises(RuntimeError, match="no gradient"):
        opt.step()
    for p in opt.params.values():
        p.grad = torch.ones_like(p)
    before = {k: p.detach().clone() for k, p in opt.params.items()}
    with pytest.raises(ValueError, match="unknown field"):
        opt.step(lrs={"scales": 1e-3})
    with pytest.raises(ValueError, match=">= 0"):
        opt.step(lrs={"means": -1.0})
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step(visible=torch.ones(G, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        opt.step(visible=torch.ones(G + 1, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="radii"):
        opt.step(visible=torch.ones(2, G + 1, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="radii"):
        opt.step(visible=torch.ones(G, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="int32 radii"):
        opt.step(visible=torch.ones(2, G, 2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        opt.step(visible=torch.ones(2, G, 4, dtype=torch.int32, device="cuda")[:, :, ::2])
    opt.params["means"].grad = torch.ones(3, G, device="cuda").t()
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    opt.params["means"].grad = torch.ones(G, 3, device="cuda")
    with pytest.raises(ValueError, match="fields must stay"):
        opt.rebind({"means": mk(G, 3)}, opt.moments)
    with pytest.raises(ValueError, match="moments"):
        opt.rebind(good(), {"means": (torch.zeros(G, 3, device="cuda"),) * 2, "harmonics": (torch.zeros(G, 3, 5, device="cuda"),) * 2})
    with pytest.raises(RuntimeError, match="GPU"):
        opt.rebind(good(), {"means": (torch.zeros(G, 3),) * 2, "harmonics": (torch.zeros(G, 3, 4),) * 2})
    with pytest.raises(ValueError, match="unknown field"):
        opt.zero_moments("scales")
    assert opt.step_count == 0 and all(torch.equal(p.detach(), before[k]) for k, p in opt.params.items()) and opt.G == G
    opt.step()
    assert opt.step_count == 1 and not torch.equal(opt.params["means"].detach(), before["means"])
