"""The ray / point adjoints' C ABI and the pose parametrisation, without a GPU: argument validation of rf_render_backward_rays and
rf_grid_query_backward_points before any device access, and so3_exp / perturb_pose against torch.autograd.gradcheck."""
import ctypes as C
import os

import pytest
import torch

import thr3ed_atom_amd as rf
from thr3ed_atom_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _grid():
    g = _lib.RFGrid()
    g.densities_dev, g.features_dev = 16, 16
    g.dims[0], g.dims[1], g.dims[2] = 4, 4, 4
    g.num_features, g.density_stride, g.feature_stride = 27, 1, 27
    return g


def test_new_entry_points_are_exported(lib):
    for name in ("rf_render_backward_rays", "rf_grid_query_backward_points"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.rf_abi_version() == 4


def test_render_backward_rays_validates_before_any_launch(lib):
    g, r, fwd, gr = _grid(), _lib.RFRayBatch(), _lib.RFRenderOut(), _lib.RFRenderGrads()
    r.num_rays, r.num_samples = 4, 8
    r.origins_dev, r.directions_dev, r.t_vals_dev = 16, 16, 16
    out = (16, 16)
    assert lib.rf_render_backward_rays(None, C.byref(r), 0, C.byref(fwd), C.byref(gr), *out, None) == -1  # NULL grid
    assert lib.rf_render_backward_rays(C.byref(g), None, 0, C.byref(fwd), C.byref(gr), *out, None) == -1  # NULL rays
    assert lib.rf_render_backward_rays(C.byref(g), C.byref(r), 0, None, C.byref(gr), *out, None) == -1  # NULL fwd
    assert lib.rf_render_backward_rays(C.byref(g), C.byref(r), 0, C.byref(fwd), None, *out, None) == -1  # NULL grads
    assert lib.rf_render_backward_rays(C.byref(g), C.byref(r), 0, C.byref(fwd), C.byref(gr), *out, None) == -1  # fwd without caches
    bad = _grid()
    bad.num_features = 5
    assert lib.rf_render_backward_rays(C.byref(bad), C.byref(r), 0, C.byref(fwd), C.byref(gr), *out, None) == -3
    cam = _lib.RFCamera()
    cam.height, cam.width, cam.focal = 4, 4, 3.0
    rc = _lib.RFRayBatch()
    rc.num_rays, rc.num_samples, rc.t_vals_dev = 4, 8, 16
    rc.camera = C.pointer(cam)
    assert lib.rf_render_backward_rays(C.byref(g), C.byref(rc), 0, C.byref(fwd), C.byref(gr), *out, None) == -3  # camera batch
    r.num_rays = 0
    assert lib.rf_render_backward_rays(C.byref(g), C.byref(r), 0, C.byref(fwd), C.byref(gr), *out, None) == 0  # zero rays: no-op
    r.num_rays = 4
    assert lib.rf_render_backward_rays(C.byref(g), C.byref(r), 0, C.byref(fwd), C.byref(gr), None, None, None) == 0  # nothing asked


def test_grid_query_backward_points_validates_before_any_launch(lib):
    g = _grid()
    assert lib.rf_grid_query_backward_points(None, 16, 4, 16, 16, None) == -1
    assert lib.rf_grid_query_backward_points(C.byref(g), None, 4, 16, 16, None) == -1
    assert lib.rf_grid_query_backward_points(C.byref(g), 16, 4, None, 16, None) == -1
    assert lib.rf_grid_query_backward_points(C.byref(g), 16, 4, 16, None, None) == -1
    assert lib.rf_grid_query_backward_points(C.byref(g), 16, -1, 16, 16, None) == -2
    assert lib.rf_grid_query_backward_points(C.byref(g), None, 0, None, None, None) == 0  # zero points: no-op
    g.dims[1] = 0
    assert lib.rf_grid_query_backward_points(C.byref(g), 16, 4, 16, 16, None) == -2


@pytest.mark.parametrize("omega", [(0.3, -0.2, 0.5), (0.0, 0.0, 0.0), (1e-4, 2e-4, -3e-4), (2.0, 1.0, -1.5)])
def test_so3_exp_gradcheck(omega):
    w = torch.tensor(omega, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(rf.so3_exp, (w,))
    R = rf.so3_exp(w.detach())
    assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-12)
    assert abs(torch.linalg.det(R).item() - 1.0) < 1e-12


def test_so3_exp_is_rodrigues():
    w = torch.tensor([0.0, 0.0, 0.7], dtype=torch.float64)
    c, s = torch.cos(torch.tensor(0.7, dtype=torch.float64)), torch.sin(torch.tensor(0.7, dtype=torch.float64))
    expect = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    assert torch.allclose(rf.so3_exp(w), expect, atol=1e-14)
    assert torch.equal(rf.so3_exp(torch.zeros(3, dtype=torch.float64)), torch.eye(3, dtype=torch.float64))


def test_perturb_pose_gradcheck():
    pose = rf.pose_spherical(30.0, -30.0, 4.0)

    def f(omega, tau):
        p = rf.perturb_pose(pose, omega, tau)
        return torch.cat([p.rotation.reshape(-1), p.translation.reshape(-1)])

    omega = torch.tensor([0.05, -0.02, 0.03], dtype=torch.float64, requires_grad=True)
    tau = torch.tensor([0.01, 0.02, -0.03], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(f, (omega, tau))
    p = rf.perturb_pose(pose, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    assert p.translation.shape == (3, 1)
    assert torch.allclose(p.rotation, pose.rotation.double()) and torch.allclose(p.translation, pose.translation.double())
