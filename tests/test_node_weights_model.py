"""CPU checks of the float64 model behind tests/test_hip_node_weights.py (tests/node_weights_model.py), of the end-to-end scene's
conditions, of the Python layer's argument validation and of the two new C entry points' presence and error codes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import node_weights_model as nm
from tests.helpers import hotdog_like_camera, procedural_grid, signed_density_grid
from thr3ed_atom_amd import _lib

TOL = 1e-5  # the project's parity bar on acc = sum_i w_i (tests/test_hip_parity.py)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _rays(n_side=12, focal=16.0, yaw=30.0, pitch=-30.0):
    pose = rf.pose_spherical(yaw, pitch, hotdog_like_camera()["radius"])
    o, d = orc.cast_rays(n_side, n_side, focal, torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


@pytest.mark.parametrize("mode", ["relu", "softplus", "abs", "identity"])
def test_weights_sum_to_the_oracles_accumulated_weight_and_corner_weights_to_one(mode):
    cam = hotdog_like_camera()
    dims, rho = (9, 8, 17), (0.5 if mode == "identity" else 100.0 / 3.0)
    dens, feat = signed_density_grid(dims, 3, 11) if mode == "identity" else procedural_grid(dims, 3, 11)
    aabb = orc.make_aabb(dims, (3.0 / 17,) * 3)
    o, d = _rays()
    ref = orc.render(dens, feat, o, d, aabb, cam["near"], cam["far"], 40, rho, mode)
    _, pts, inside, deltas = nm.sample_geometry(o, d, aabb, cam["near"], cam["far"], 40)
    assert torch.equal(deltas, ref["deltas"]) and bool(inside.any()) and not bool(inside.all())
    w, lin, b, ok = nm.sample_weights(dens, aabb, rho, mode, pts, inside, deltas)
    acc = ref["acc"].numpy()[:, 0].astype(np.float64)
    finite = np.isfinite(acc)  # (identity: a negative last sample makes the reference's own alpha -inf)
    assert finite.sum() >= 0.5 * len(acc)
    np.testing.assert_allclose(w.sum(-1)[finite], acc[finite], rtol=0, atol=TOL)
    np.testing.assert_allclose(b.sum(-1), 1.0, rtol=0, atol=1e-12)
    assert not ok.all()  # samples in the half-voxel border have corners outside the grid


def test_prune_model_on_hand_written_cases():
    # 1-D: one hot node at 4 of 9; dilate d keeps 4-d .. 4+d
    M = np.zeros((9, 1, 1))
    M[4] = 0.5
    for d in (0, 1, 2):
        keep = nm.keep_mask(M, 0.0, d)[:, 0, 0]
        assert keep.tolist() == [abs(i - 4) <= d for i in range(9)]
    # strict: a node AT the threshold is not hot
    assert not nm.keep_mask(M, 0.5, 0).any() and nm.keep_mask(M, np.nextafter(0.5, 0), 0).sum() == 1
    # borders: a hot corner node, dilate 2 -> the 3^3 nodes of the corner, clipped to the grid
    M = np.zeros((4, 5, 6))
    M[0, 4, 5] = 1e-6
    keep = nm.keep_mask(M, 0.0, 2)
    want = np.zeros_like(keep)
    want[0:3, 2:5, 3:6] = True
    assert np.array_equal(keep, want)
    # 3-D Chebyshev ball away from the border
    M = np.zeros((7, 7, 7))
    M[3, 3, 3] = 2.0
    assert nm.keep_mask(M, 1.0, 1).sum() == 27 and nm.keep_mask(M, 1.0, 2).sum() == 125 and nm.keep_mask(M, 2.0, 2).sum() == 0
    # the density rule: min(D, fill) keeps the bits of densities at or below the fill; |.| grids go to 0
    dens = np.array([-2.0, -0.0, 0.0, 3.0, 0.25], dtype=np.float32).reshape(5, 1, 1, 1)
    M = np.zeros((5, 1, 1))
    M[4] = 1.0
    keep, new, counts = nm.prune(dens, M, 0.0, 0, 0.0, "relu")
    assert counts == (1, 4) and keep[:, 0, 0].tolist() == [False] * 4 + [True]
    assert new.view(np.uint32).ravel().tolist() == np.array([-2.0, -0.0, 0.0, 0.0, 0.25], dtype=np.float32).view(np.uint32).tolist()
    _, new, _ = nm.prune(dens, M, 0.0, 0, -1.0, "softplus")
    assert new.ravel().tolist() == [-2.0, -1.0, -1.0, -1.0, 0.25]
    _, new, _ = nm.prune(dens, M, 0.0, 0, 0.0, "abs")
    assert new.view(np.uint32).ravel().tolist() == np.array([0.0, 0.0, 0.0, 0.0, 0.25], dtype=np.float32).view(np.uint32).tolist()


def _scene():
    cam = hotdog_like_camera()
    dens, feat = nm.scene_grid()
    return dens, feat, orc.make_aabb(nm.SCENE_DIMS, nm.SCENE_VOXEL), cam["near"], cam["far"]


def test_a_model_without_the_transmittance_is_rejected_at_the_bar():
    """The comparison of the GPU test can fail: w_i = alpha_i instead of T_i alpha_i is further than TOL from the model on the scene."""
    dens, _, aabb, near, far = _scene()
    intr, poses = nm.scene_views()
    o, d = orc.cast_rays(intr[0], intr[1], intr[2], torch.as_tensor(poses[0].rotation), torch.as_tensor(poses[0].translation))
    args = (dens, aabb, nm.SCENE_RHO, "relu", o.reshape(-1, 3), d.reshape(-1, 3), near, far, nm.SCENE_SAMPLES)
    right, _, _ = nm.model_max_weight(*args)
    wrong, _, _ = nm.model_max_weight(*args, drop_transmittance=True)
    assert np.abs(right - wrong).max() > 1000 * TOL


def test_the_end_to_end_scene_meets_its_conditions():
    """In the kernel's float32 form of the transmittance: the blob is never weighted under the six views, the speck's largest
    weight is below tau and non-zero, every shell node some view can reach is above it, and no non-zero product lies below 1e-30
    (so that an exact zero is an exact zero whatever a device does with denormals)."""
    dens, _, aabb, near, far = _scene()
    M, smallest = nm.scene_float32_products(dens, aabb, near, far)
    shell, blob, speck = nm.scene_regions()
    assert M[blob].max() == 0.0
    assert 0.0 < M[speck].max() < nm.SCENE_TAU
    x, y, z = nm.SPECK
    assert M[x - 1 : x + 2, y - 1 : y + 2, z - 1 : z + 2].max() < nm.SCENE_TAU  # no neighbour keeps the speck alive at dilate 1
    assert M[shell].max() > nm.SCENE_TAU and (M[shell] > nm.SCENE_TAU).sum() > 500
    assert smallest >= 1e-30
    # sigma * delta >= 20 for every sample whose eight corners are wall nodes
    assert nm.SHELL_DENSITY * nm.SCENE_RHO * (float(np.float32(far)) - float(np.float32(near))) / (nm.SCENE_SAMPLES - 1) >= 20.0
    # the float64 model agrees on what is weighted at all (a float64 transmittance never reaches 0: compare above 1e-30)
    intr, poses = nm.scene_views()
    M64 = None
    for pose in poses:
        o, d = orc.cast_rays(intr[0], intr[1], intr[2], torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))
        M64, _, _ = nm.model_max_weight(dens, aabb, nm.SCENE_RHO, "relu", o.reshape(-1, 3), d.reshape(-1, 3), near, far, nm.SCENE_SAMPLES, prefill=M64)
    assert np.array_equal(M64 > 1e-30, M > 0.0)
    np.testing.assert_allclose(M64, M, rtol=0, atol=TOL)


def test_python_layer_validates_its_arguments():
    dens, feat = procedural_grid((4, 4, 4), 3, 3)
    grid = rf.VoxelGrid(dens, feat, rf.VoxelSize(0.75, 0.75, 0.75), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU())
    M = torch.zeros(4, 4, 4)
    for bad in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=0.0, dilate=5),
                dict(threshold=0.0, dilate=-1), dict(threshold=0.0, fill_density=float("nan"))):
        with pytest.raises(ValueError):
            rf.prune_voxel_grid(grid, M, **bad)
    soft = rf.VoxelGrid(dens, feat, rf.VoxelSize(0.75, 0.75, 0.75), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.Softplus())
    with pytest.raises(ValueError, match="softplus"):
        rf.prune_voxel_grid(soft, M, 0.0)
    absg = rf.VoxelGrid(dens, feat, rf.VoxelSize(0.75, 0.75, 0.75))  # (the reference's default: |.| / identity)
    with pytest.raises(ValueError, match="only fill is 0"):
        rf.prune_voxel_grid(absg, M, 0.0, fill_density=-1.0)
    # no CPU fallback: the launch itself refuses host tensors
    with pytest.raises(RuntimeError, match="HIP device"):
        rf.prune_voxel_grid(grid, M, 0.0)
    bounds, intr = rf.CameraBounds(2.0, 6.0), rf.CameraIntrinsics(8, 8, 10.0)
    pose = rf.pose_spherical(0.0, -30.0, 4.0)
    with pytest.raises(ValueError, match="num_samples"):
        rf.node_max_weights(grid, [pose], intr, bounds, 0)
    with pytest.raises(ValueError, match="intrinsics"):
        rf.node_max_weights(grid, [pose], rf.CameraIntrinsics(8, 0, 10.0), bounds, 8)
    with pytest.raises(ValueError, match="pose"):
        rf.node_max_weights(grid, [torch.zeros(4, 4)], intr, bounds, 8)
    with pytest.raises(ValueError, match="out must be"):
        rf.node_max_weights(grid, [pose], intr, bounds, 8, out=torch.zeros(4, 4, 5))
    with pytest.raises(RuntimeError, match="HIP device"):
        rf.node_max_weights(grid, [pose], intr, bounds, 8)


def test_the_two_entry_points_are_exported_with_prototypes(lib):
    for name in ("rf_node_max_weight", "rf_prune_grid"):
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    assert len(lib.rf_node_max_weight.argtypes) == 5 and len(lib.rf_prune_grid.argtypes) == 9
    assert lib.rf_abi_version() == 4  # additive: the ABI version stays
    for name in ("node_max_weights", "prune_voxel_grid", "PruneStats"):
        assert hasattr(rf, name)


def test_error_codes_come_before_any_device_access(lib):
    """(fake non-null pointers: a launch would fault, a code returns)"""
    g, r = _lib.RFGrid(), _lib.RFRayBatch()
    assert lib.rf_node_max_weight(None, C.byref(r), 0, 16, None) == -1
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), 0, 16, None) == -1  # null grid tensors
    g.densities_dev, g.features_dev = 16, 16
    g.dims[0], g.dims[1], g.dims[2] = 4, 4, 4
    g.num_features, g.density_stride, g.feature_stride = 3, 1, 3
    assert lib.rf_node_max_weight(C.byref(g), None, 0, 16, None) == -1
    r.num_rays, r.num_samples = 4, 0
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), 0, 16, None) == -2  # num_samples < 1
    r.num_samples = 8
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), 0, 16, None) == -1  # rays without t_vals / origins
    r.num_rays = 0
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), 0, None, None) == -1  # no buffer
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), _lib.FLAG_OCCUPANCY_SKIP, 16, None) == -1  # the flag without a mask
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), 0, 16, None) == 0  # zero rays: no-op
    g.dims[1] = 0
    assert lib.rf_node_max_weight(C.byref(g), C.byref(r), 0, 16, None) == -2
    assert lib.rf_prune_grid(C.byref(g), 16, 0.0, 1, 0.0, 16, None, None, None) == -2  # bad dims
    g.dims[1] = 4
    assert lib.rf_prune_grid(None, 16, 0.0, 1, 0.0, 16, None, None, None) == -1
    assert lib.rf_prune_grid(C.byref(g), None, 0.0, 1, 0.0, 16, None, None, None) == -1
    assert lib.rf_prune_grid(C.byref(g), 16, 0.0, 1, 0.0, None, None, None, None) == -1
    for dilate in (-1, 5):
        assert lib.rf_prune_grid(C.byref(g), 16, 0.0, dilate, 0.0, 16, None, None, None) == -2
    for threshold in (-1e-9, float("inf"), float("nan")):
        assert lib.rf_prune_grid(C.byref(g), 16, threshold, 1, 0.0, 16, None, None, None) == -2
    g.density_mode = _lib.DENSITY_MODES["abs"]
    assert lib.rf_prune_grid(C.byref(g), 16, 0.0, 1, -1.0, 16, None, None, None) == -2  # |.|: the only fill is 0
