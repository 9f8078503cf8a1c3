"""cameras.CameraState.step (siu3r_camera_step, csrc/camera.hip) on the GPU against one step of tests/dense_camera64.py in float64.

Bounds: the kernel computes in fp64 from the fp32 state and rounds once per stored value (2^-24 relative); every stored moment and M
entry must be within 2^-22 relative of the reference (the margin covers sqrt / sin / cos and the matrix exponential's own error), with an
absolute floor of 1e-30; every c2w entry within 2^-22 x max(1, the largest magnitude of its row)."""
import math

import pytest
import torch

import dense_camera64 as D

pytestmark = pytest.mark.gpu

REL = 2.0 ** -22
BETAS, EPS = (0.9, 0.999), 1e-8


def _state(V, fixed, seed, pose=True, exposure=True, grad_scale=1.0):
    """a CameraState with random fp32 poses, M, moments and gradients in its holders"""
    from siu3r_amd.cameras import CameraState

    g = torch.Generator().manual_seed(seed)
    c2w = torch.eye(4).repeat(V, 1, 1)
    q, _ = torch.linalg.qr(torch.randn(V, 3, 3, generator=g))
    c2w[:, :3, :3] = q
    c2w[:, :3, 3] = 3.0 * torch.randn(V, 3, generator=g)
    st = CameraState(c2w.cuda(), pose=pose, exposure=exposure, fixed=fixed, betas=BETAS, eps=EPS)
    with torch.no_grad():
        st.M += (0.1 * torch.randn(V, 3, 4, generator=g)).cuda()
    st.exp_avg.copy_(grad_scale * 0.3 * torch.randn(V, 18, generator=g))
    st.exp_avg_sq.copy_((grad_scale * 0.3 * torch.randn(V, 18, generator=g)) ** 2)
    g_xi = grad_scale * torch.randn(V, 6, generator=g)
    if pose:
        st.trans_delta.grad, st.rot_delta.grad = g_xi[:, :3].contiguous().cuda(), g_xi[:, 3:].contiguous().cuda()
    if exposure:
        st.M.grad = (grad_scale * torch.randn(V, 3, 4, generator=g)).cuda()
    return st, g_xi


def _snapshot(st):
    return [t.detach().clone() for t in (st.c2w, st.M, st.exp_avg, st.exp_avg_sq)]


def _reference(st, g_xi, t, lrs):
    g_m = st.M.grad if st.exposure else torch.zeros(st.V, 3, 4)
    return D.camera_step(st.c2w, st.M, g_xi, g_m, st.exp_avg, st.exp_avg_sq, st.free.cpu(), t, lrs, BETAS, EPS, pose=st.pose, exposure=st.exposure)


def _check(st, ref, what):
    c2w, M, m1, m2, _ = ref
    for name, got, want in (("exp_avg", st.exp_avg, m1), ("exp_avg_sq", st.exp_avg_sq, m2), ("M", st.M.detach(), M)):
        err = (got.cpu().double() - want).abs()
        bound = REL * want.abs() + 1e-30
        assert bool((err <= bound).all()), f"{what}: {name} off by {float((err / (want.abs() + 1e-30)).max()):.3e} relative (bound {REL:.3e})"
    err = (st.c2w.cpu().double() - c2w).abs()
    bound = REL * c2w.abs().amax(dim=2, keepdim=True).clamp_min(1.0)
    assert bool((err <= bound).all()), f"{what}: c2w off by {float((err / bound).max()):.3e} x the bound"
    return float((err / bound).max())


@pytest.mark.parametrize("halves", ["pose", "exposure", "both"])
@pytest.mark.parametrize("V,fixed", [(1, ()), (5, (0, 3))])
@pytest.mark.parametrize("th_target", [1e-9, 1e-4, 9e-3, 1.1e-2, 0.3, 2.0])
def test_one_step_against_float64(th_target, V, fixed, halves):
    pose, exposure = halves != "exposure", halves != "pose"
    t = 7
    st, g_xi = _state(V, fixed, seed=V * 10 + len(halves), pose=pose, exposure=exposure)
    free_view = next(v for v in range(V) if v not in fixed)
    lr_rot = 1.0
    if pose:  # the update is linear in the rate: scale it so that the first free view's rotation angle is the target
        lr_rot = th_target / float(_reference(st, g_xi, t, (1.0, 1.0, 1.0))[4][free_view])
    lrs = (0.37 * lr_rot, lr_rot, min(th_target, 0.05))
    ref = _reference(st, g_xi, t, lrs)
    before = _snapshot(st)
    st.step(t, lrs)
    worst = _check(st, ref, f"th ~ {th_target:g}, V = {V}, {halves}")
    th = [float(x) for x in ref[4]]
    print(f"\nth target {th_target:g} V={V} {halves}: theta per view {' '.join(f'{x:.3e}' for x in th)}; c2w error {worst:.3f} x the bound")
    if pose:
        assert abs(th[free_view] / th_target - 1.0) <= 1e-6
    for v in fixed:  # a fixed view keeps every bit
        for a, b in zip(before, _snapshot(st)):
            assert torch.equal(a[v], b[v])
    after = _snapshot(st)
    if not pose:
        assert torch.equal(before[0], after[0]) and torch.equal(before[2][:, :6], after[2][:, :6]) and torch.equal(before[3][:, :6], after[3][:, :6])
    if not exposure:
        assert torch.equal(before[1], after[1]) and torch.equal(before[2][:, 6:], after[2][:, 6:]) and torch.equal(before[3][:, 6:], after[3][:, 6:])
    free = [v for v in range(V) if v not in fixed]
    assert not torch.equal(before[2][free], after[2][free])


def test_zero_gradients_and_moments_keep_the_bits_of_the_pose():
    st, _ = _state(4, (1,), seed=3)
    with torch.no_grad():
        st.c2w[2, 0, 1] = -0.0  # a product with the identity would make it +0
        st.c2w[2, 1, 3] = 0.0
    st.exp_avg.zero_(), st.exp_avg_sq.zero_()
    st.trans_delta.grad.zero_(), st.rot_delta.grad.zero_(), st.M.grad.zero_()
    before = _snapshot(st)
    st.step(1, (3e-3, 3e-3, 1e-2))
    for a, b in zip(before, _snapshot(st)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_two_calls_on_equal_inputs_give_equal_bits():
    res = []
    for _ in range(2):
        st, _ = _state(5, (0,), seed=11)
        st.step(3, (2e-3, 4e-3, 1e-2))
        res.append(_snapshot(st))
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_rotation_stays_orthonormal_over_300_steps():
    """300 consecutive steps of about 1e-2 rad: R is never re-orthonormalised, every step rounds the fp64 product to fp32 once.  Expected
    drift of R^T R - I: 300 x 2^-24 = 2e-5 in the worst case, a few 1e-6 as a random walk.  The bound is 1e-5."""
    V = 4
    st, _ = _state(V, (0,), seed=21, exposure=False)
    st.exp_avg.zero_(), st.exp_avg_sq.zero_()
    g = torch.Generator().manual_seed(5)
    lr = 1e-2 / math.sqrt(3.0)  # a constant gradient steps every rotation component by the rate
    for t in range(1, 301):
        if t % 50 == 1:
            g_xi = torch.randn(V, 6, generator=g)
            st.trans_delta.grad, st.rot_delta.grad = g_xi[:, :3].contiguous().cuda(), g_xi[:, 3:].contiguous().cuda()
        st.step(t, (lr, lr, 0.0))
    R = st.c2w[:, :3, :3].double()
    drift = float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64, device="cuda")).abs().max())
    print(f"\nR^T R - I after 300 steps of ~1e-2 rad: {drift:.3e} (bound 1e-5)")
    assert drift <= 1e-5
    assert torch.equal(st.c2w[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).repeat(V, 1))


def test_error_paths():
    from siu3r_amd.cameras import CameraState

    c2w = torch.eye(4).repeat(3, 1, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        CameraState(c2w)
    with pytest.raises(ValueError, match="V,4,4"):
        CameraState(torch.eye(3).repeat(3, 1, 1).cuda())
    with pytest.raises(ValueError, match="every"):
        CameraState(c2w.cuda(), fixed=(0, 1, 2))
    st = CameraState(c2w.cuda())
    with pytest.raises(RuntimeError, match="no gradient"):
        st.step(1, (1e-3, 1e-3, 1e-3))
    st, _ = _state(3, (0,), seed=2)
    with pytest.raises(RuntimeError, match="step count"):
        st.step(0, (1e-3, 1e-3, 1e-3))
    with pytest.raises(RuntimeError, match="rate"):
        st.step(1, (-1e-3, 1e-3, 1e-3))
