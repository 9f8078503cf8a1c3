"""CPU tests of the camera optimisation (siu3r_amd/cameras.py, csrc/camera.hip): the C ABI of the new entry points, CameraControl's
validation and rate schedule, the float64 reference's closed-form se(3) exponential against the matrix exponential, and the compiler's
resource remarks of the new unit."""
import os
import re

import pytest
import torch

import dense_camera64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("siu3r_exposure_ws", "siu3r_exposure_apply", "siu3r_exposure_apply_bwd", "siu3r_camera_step")


def test_new_symbols_are_declared_exported_and_signed():
    from siu3r_amd import _lib

    text = open(os.path.join(ROOT, "include", "siu3r_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(siu3r_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/siu3r_hip.h"
        assert hasattr(l, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert l.siu3r_abi_version() == _lib.ABI_VERSION == 13
    # the size query is a host function: 12 doubles per workgroup of 2,048 pixels
    assert l.siu3r_exposure_ws(6, 512, 512) == 6 * 128 * 12 * 8
    assert l.siu3r_exposure_ws(1, 1, 1) == 96 and l.siu3r_exposure_ws(2, 3, 683) == 2 * 2 * 96
    assert l.siu3r_exposure_ws(0, 4, 4) == 0


def test_camera_control_validation():
    from siu3r_amd.cameras import CameraControl

    CameraControl().validate(2)
    CameraControl(fixed=()).validate(1)
    CameraControl(pose=False, fixed=(1, 3)).validate(5)
    with pytest.raises(ValueError, match="both off"):
        CameraControl(pose=False, exposure=False).validate(4)
    with pytest.raises(ValueError, match="outside"):
        CameraControl(fixed=(4,)).validate(4)
    with pytest.raises(ValueError, match="outside"):
        CameraControl(fixed=(-1,)).validate(4)
    with pytest.raises(ValueError, match="every"):
        CameraControl().validate(1)
    with pytest.raises(ValueError, match="every"):
        CameraControl(fixed=(0, 1, 1, 0)).validate(2)
    for name in ("lr_rot", "lr_trans", "lr_exposure", "lr_final_scale"):
        for bad in (0.0, -1e-3, float("inf"), float("nan")):
            with pytest.raises(ValueError, match=name):
                CameraControl(**{name: bad}).validate(3)
    with pytest.raises(ValueError, match="start"):
        CameraControl(start=-1).validate(3)


def test_refine_validates_the_control_before_any_device_work():
    """CPU tensors: a bad control raises ValueError before anything touches a device"""
    from siu3r_amd.cameras import CameraControl
    from siu3r_amd.refine import refine_gaussians

    G, V = 4, 3
    args = (torch.zeros(G, 3), torch.ones(G, 3), torch.ones(G, 4), torch.full((G,), 0.5), torch.zeros(G, 3, 4), torch.zeros(V, 3, 16, 16),
            torch.eye(4).repeat(V, 1, 1), torch.eye(3), 0.5, 100.0, (0, 0, 0))
    with pytest.raises(ValueError, match="both off"):
        refine_gaussians(*args, cameras=CameraControl(pose=False, exposure=False))
    with pytest.raises(ValueError, match="outside"):
        refine_gaussians(*args, cameras=CameraControl(fixed=(3,)))
    with pytest.raises(ValueError, match="every"):
        refine_gaussians(*args, cameras=CameraControl(fixed=(0, 1, 2)))
    with pytest.raises(ValueError, match="lr_rot"):
        refine_gaussians(*args, cameras=CameraControl(lr_rot=0.0))


def test_rate_schedule_end_points():
    from siu3r_amd.cameras import CameraControl

    c = CameraControl(lr_trans=2e-3, lr_rot=3e-3, lr_exposure=1e-2, lr_final_scale=0.1)
    r = c.rates(200)
    assert len(r) == 200 and r[0] == (2e-3, 3e-3, 1e-2) and r[-1] == (2e-3 * 0.1, 3e-3 * 0.1, 1e-2 * 0.1)
    assert all(a[k] > b[k] for a, b in zip(r, r[1:]) for k in range(3))
    mid = r[100][1] / 3e-3
    assert abs(mid - 0.1 ** (100 / 199)) <= 1e-12  # log-linear
    late = CameraControl(start=50).rates(60)
    assert len(late) == 10 and late[0] == (3e-3, 3e-3, 1e-2) and abs(late[-1][2] - 1e-3) <= 1e-18
    assert CameraControl(start=5).rates(5) == [] and CameraControl().rates(1) == [(3e-3, 3e-3, 1e-2)]


@pytest.mark.parametrize("th", [0.0, 1e-12, 1e-8, 1e-4, 9.9e-3, 1.01e-2, 0.1, 1.0, 3.0])
def test_closed_form_exponential_against_matrix_exp(th):
    """the closed form with its series switch at 1e-2 against torch.linalg.matrix_exp in float64, to 1e-14 on every entry"""
    g = torch.Generator().manual_seed(int(th * 1e6) % 1000 + 1)
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm()
    rho = torch.randn(3, generator=g, dtype=torch.float64)
    xi = torch.cat((rho, axis * th))
    got, want = D.se3_exp_closed(xi), D.se3_exp(xi)
    err = float((got - want).abs().max())
    print(f"\nth = {th:g}: closed form vs matrix_exp max |d| = {err:.2e}")
    assert err <= 1e-14
    R = got[:3, :3]
    assert float((R.T @ R - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14


def test_zero_update_is_exactly_the_identity():
    assert torch.equal(D.se3_exp_closed(torch.zeros(6, dtype=torch.float64)), torch.eye(4, dtype=torch.float64))
    c = torch.randn(4, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal((c.double() @ D.se3_exp_closed(torch.zeros(6))).float(), c)


def test_code_object_resources():
    """no kernel of the unit uses scratch memory or spills; LDS is the reduction's 12 x 4 doubles only"""
    from siu3r_amd import build as B

    res = B.kernel_resources("camera.hip")
    for n in ("exposure_fwd_kernel", "exposure_bwd_kernelILb1ELb1", "exposure_bwd_kernelILb1ELb0", "exposure_bwd_kernelILb0ELb1", "exposure_gm_kernel",
              "camera_step_kernel"):
        assert any(n in k for k in res), (n, sorted(res))
    for k, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] <= 12 * 4 * 8, (k, r)
