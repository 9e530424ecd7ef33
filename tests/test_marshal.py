"""The one marshalling path of the Python binding (thr3ed_atom_amd/_marshal.py and the ray-batch helpers of ops.py): cameras, ray
batches, the jitter choice and the mesh checks, on the CPU -- none of this needs the library or a device.  The expected messages
are spelled out: they are the ones the GPU tests and callers match on."""
import re

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from thr3ed_atom_amd import _marshal, mesh_raster, ops

ROTATION = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]  # not symmetric: a transposed pose would show
TRANSLATION = [1.5, -2.5, 3.5]
POSE = rf.CameraPose(torch.tensor(ROTATION), torch.tensor(TRANSLATION).reshape(3, 1))


def raises(kind, text):
    return pytest.raises(kind, match="^" + re.escape(text) + "$")


def test_package_names_are_the_shared_helpers():
    assert ops._ptr is _marshal.ptr and ops._stream is _marshal.stream and ops._require_hip is _marshal.require_hip
    assert ops._camera_struct is _marshal.camera_struct and mesh_raster._camera is _marshal.checked_camera
    assert _marshal.ptr(None) is None and _marshal.ptr(torch.zeros(1)) != 0
    with raises(RuntimeError, "image must live on a HIP device (got cpu); the render path has no CPU fallback"):
        _marshal.require_hip(torch.zeros(1), "image")


def test_camera_struct_is_row_major_rotation_and_translation():
    cam = _marshal.camera_struct(7, 9, 1111.111, POSE.rotation, POSE.translation)
    assert (cam.height, cam.width) == (7, 9)
    assert cam.focal == float(np.float32(1111.111)) != 1111.111
    expected = [v for row, t in zip(ROTATION, TRANSLATION) for v in row + [t]]
    assert list(cam.pose) == [float(np.float32(v)) for v in expected]


@pytest.mark.parametrize("intrinsics, message", [
    ((True, 4, 2.0), "the image must be between 1 and 16384 pixels along each edge, got True x 4"),
    ((0, 4, 2.0), "the image must be between 1 and 16384 pixels along each edge, got 0 x 4"),
    ((4, 16385, 2.0), "the image must be between 1 and 16384 pixels along each edge, got 4 x 16385"),
    ((4.5, 4, 2.0), "the image must be between 1 and 16384 pixels along each edge, got 4.5 x 4"),
    ((4, 4, 0.0), "focal must be positive and finite, got 0.0"),
    ((4, 4, float("nan")), "focal must be positive and finite, got nan"),
    ((4, 4, float("inf")), "focal must be positive and finite, got inf"),
])
def test_checked_camera_rejections(intrinsics, message):
    with raises(ValueError, message):
        _marshal.checked_camera(POSE, intrinsics)


def test_checked_camera_edge_limit_is_the_callers():
    with raises(ValueError, "the image must be between 1 and 8 pixels along each edge, got 9 x 4"):
        _marshal.checked_camera(POSE, (9, 4, 2.0), 8)


def test_checked_camera_pose():
    bad = rf.CameraPose(torch.tensor(ROTATION), torch.tensor([0.0, float("nan"), 0.0]).reshape(3, 1))
    with raises(ValueError, "the camera pose is not finite"):
        _marshal.checked_camera(bad, (4, 4, 2.0))
    cam = _marshal.checked_camera(POSE, (16384, 1, 2.5))
    assert bytes(cam) == bytes(_marshal.camera_struct(16384, 1, 2.5, POSE.rotation, POSE.translation))


def test_non_negative():
    assert _marshal.non_negative(0, "near") == 0.0 and _marshal.non_negative(0.1, "near") == float(np.float32(0.1))
    with raises(ValueError, "near must be non-negative and finite, got -1.0"):
        _marshal.non_negative(-1, "near")
    with raises(ValueError, "reach must be non-negative and finite, got nan"):
        _marshal.non_negative(float("nan"), "reach")
    with raises(ValueError, "depth_bias must be non-negative and finite, got inf"):
        _marshal.non_negative(float("inf"), "depth_bias")


def test_ray_batch_struct_of_a_camera():
    camera = (6, 5, 20.0, POSE.rotation, POSE.translation)
    whole, keep = ops._ray_batch_struct(ops.RayBatch(None, None, 8, 0.5, 4.0, camera=camera), "cpu", "a test")
    assert (whole.num_rays, whole.first_ray, whole.num_samples, whole.near, whole.far) == (30, 0, 8, 0.5, 4.0)
    assert not whole.origins_dev and not whole.directions_dev and not whole.t_rand_dev and whole.jitter_key == 0
    assert bytes(whole.camera.contents) == bytes(_marshal.camera_struct(*camera))
    assert any(torch.is_tensor(k) and k.data_ptr() == whole.t_vals_dev and torch.equal(k, torch.linspace(0.0, 1.0, 8)) for k in keep)
    rest, _ = ops._ray_batch_struct(ops.RayBatch(None, None, 8, 0.5, 4.0, camera=camera, first_ray=7), "cpu", "a test")
    assert (rest.num_rays, rest.first_ray) == (23, 7)
    part, _ = ops._ray_batch_struct(ops.RayBatch(None, None, 8, 0.5, 4.0, camera=camera, first_ray=7, num_rays=11), "cpu", "a test")
    assert (part.num_rays, part.first_ray) == (11, 7)
    keyed = ops.RayBatch(None, None, 8, 0.5, 4.0, t_rand=ops.KeyedJitter(-1, 99), camera=camera, first_ray=7)
    rb, _ = ops._ray_batch_struct(keyed, "cpu", "a test")
    assert rb.jitter_key == 0xFFFFFFFFFFFFFFFF and rb.first_ray == 7 and not rb.t_rand_dev  # (a frame's first_ray is the pixel's, not the jitter's)
    assert ops._jitter_flags(2, keyed.t_rand) == 2 | 16 and ops._jitter_flags(2, None) == 2
    assert ops._ray_batch_struct(keyed._replace(t_rand=ops.KeyedJitter((1 << 64) + 5)), "cpu", "a test")[0].jitter_key == 5


def flat_rays(n=5):
    return rf.Rays(torch.arange(3.0 * n).reshape(n, 3).double(), torch.ones(n, 3))


def test_flat_ray_batch_jitter_choice():
    rays, S = flat_rays(), 4
    t_rand = torch.rand(5, S, dtype=torch.float64)
    batch = ops._flat_ray_batch(rays, S, (0.1, 4.0), True, t_rand, 7, "distortion_loss")
    assert torch.equal(batch.t_rand, t_rand.float()) and batch.t_rand.dtype == torch.float32  # a tensor wins over key and perturb
    assert batch.origins.dtype == torch.float32 and torch.equal(batch.origins, rays.origins.float()) and batch.num_samples == S
    assert (batch.near, batch.far) == (float(np.float32(0.1)), 4.0) and batch.camera is None
    keyed = ops.KeyedJitter(3, 2)
    assert ops._flat_ray_batch(rays, S, rf.CameraBounds(0.1, 4.0), True, keyed, 7, "distortion_loss").t_rand is keyed
    assert ops._flat_ray_batch(rays, S, (0.1, 4.0), True, None, 7, "distortion_loss").t_rand == ops.KeyedJitter(7, 0)
    torch.manual_seed(11)
    drawn = ops.draw_jitter_key()
    torch.manual_seed(11)
    assert ops._flat_ray_batch(rays, S, (0.1, 4.0), True, None, None, "distortion_loss").t_rand == ops.KeyedJitter(drawn, 0)
    assert ops._flat_ray_batch(rays, S, (0.1, 4.0), False, None, None, "distortion_loss").t_rand is None


@pytest.mark.parametrize("name", ["distortion_loss", "render_geometry"])
def test_flat_ray_rejections_through_the_public_functions(name):
    grid = rf.VoxelGrid(torch.zeros(2, 2, 2, 1), torch.zeros(2, 2, 2, 3), rf.VoxelSize(1, 1, 1))
    function = getattr(rf, name)
    with raises(AssertionError, f"{name} takes FLAT rays [N, 3]"):
        function(grid, rf.Rays(torch.zeros(2, 5, 3), torch.ones(2, 5, 3)), 4, (0.5, 4.0))
    with raises(ValueError, "t_rand must be [5, 4]"):
        function(grid, flat_rays(), 4, (0.5, 4.0), t_rand=torch.zeros(5, 3))


def meshes():
    vertices, faces = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int64)
    return [(rf.Mesh(vertices, faces, None, None), "{} takes a Mesh of tensors"),
            (rf.Mesh(torch.from_numpy(vertices), torch.from_numpy(faces), None, None),
             "{} takes a mesh on a HIP device (got vertices on cpu, faces on cpu); there is no CPU path")]


@pytest.mark.parametrize("mesh, message", meshes(), ids=["numpy", "cpu"])
def test_mesh_arrays_through_the_public_functions(mesh, message):
    with raises(ValueError, message.format("simplify_mesh")):
        rf.simplify_mesh(mesh, 0.5)
    with raises(ValueError, message.format("bake_texture")):
        rf.bake_texture(mesh, None)
    with raises(ValueError, message.format("render_mesh")):
        rf.render_mesh(mesh, POSE, (4, 4, 2.0))
    with raises(ValueError, message.format("bake_texture")):  # (the view bakes report the mesh in bake_texture's words)
        rf.bake_texture_from_views(mesh, [], [], (4, 4, 2.0))


def test_mesh_arrays_devices_and_shapes(monkeypatch):
    """the checks behind the device test, reached on the CPU by answering ``is_cuda`` with True; ``simplify_mesh`` now refuses
    vertices and faces on two devices in the words ``bake_texture`` and ``render_mesh`` always used"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    good_v, good_f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    elsewhere = rf.Mesh(torch.zeros(3, 3, device="meta"), good_f, None, None)
    for call in (lambda: rf.simplify_mesh(elsewhere, 0.5), lambda: rf.bake_texture(elsewhere, None), lambda: rf.render_mesh(elsewhere, POSE, (4, 4, 2.0))):
        with raises(ValueError, "vertices are on meta, faces on cpu"):
            call()
    vertices, faces = _marshal.mesh_arrays(rf.Mesh(good_v.requires_grad_(), good_f, None, None), "render_mesh")
    assert faces.dtype == torch.int64 and not vertices.requires_grad and vertices.is_contiguous() and faces.is_contiguous()
    for bad in (torch.zeros(3, 2), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3)):
        with raises(ValueError, "vertices must be a float32 tensor of shape [V, 3]"):
            _marshal.mesh_arrays(rf.Mesh(bad, good_f, None, None), "render_mesh")
    for bad in (torch.zeros(1, 3), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)):
        with raises(ValueError, "faces must be an integer tensor of shape [T, 3]"):
            _marshal.mesh_arrays(rf.Mesh(good_v.detach(), bad, None, None), "render_mesh")
