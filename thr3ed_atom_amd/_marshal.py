"""How tensors, cameras and meshes cross the C ABI (include/relu_field.h): raw pointers, the stream handle, the RFCamera of a posed
pinhole camera, the checks every mesh entry point makes before its first launch, the visibility pass and the offsets of a segmented
sum.  A leaf: it imports the library binding and the camera tuples and nothing else of the package, so ``ops``, ``voxels``, ``mesh``,
``texture``, ``mesh_raster`` and the two fits can all use it."""
import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .camera import CameraIntrinsics, CameraPose


def ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_hip(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); the render path has no CPU fallback")


def non_negative(value, name: str) -> float:
    value = float(np.float32(value))
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f"{name} must be non-negative and finite, got {value!r}")
    return value


def positive(value, name: str) -> float:
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"{name} must be positive and finite, got {value!r}")
    return value


def iteration_count(iterations) -> int:
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
        raise ValueError(f"iterations must be a non-negative integer, got {iterations!r}")
    return int(iterations)


def identity_pose() -> CameraPose:
    return CameraPose(torch.eye(3), torch.zeros(3, 1))


def camera_struct(height, width, focal, rotation, translation) -> "_lib.RFCamera":
    cam = _lib.RFCamera()
    cam.height, cam.width, cam.focal = int(height), int(width), float(np.float32(focal))
    rot = torch.as_tensor(rotation).detach().to("cpu", torch.float32).reshape(3, 3)
    trans = torch.as_tensor(translation).detach().to("cpu", torch.float32).reshape(3)
    for i in range(3):
        for j in range(3):
            cam.pose[4 * i + j] = float(rot[i, j])
        cam.pose[4 * i + 3] = float(trans[i])
    return cam


def checked_camera(camera_pose: CameraPose, camera_intrinsics: CameraIntrinsics, max_edge: int = _lib.RASTER_MAX_EDGE) -> "_lib.RFCamera":
    """``camera_struct`` of a camera the rasteriser takes: integer edges in [1, max_edge], a positive finite focal, a finite pose"""
    height, width, focal = camera_intrinsics
    if isinstance(height, bool) or isinstance(width, bool) or int(height) != height or int(width) != width or not (1 <= int(height) <= max_edge and 1 <= int(width) <= max_edge):
        raise ValueError(f"the image must be between 1 and {max_edge} pixels along each edge, got {height} x {width}")
    focal = float(np.float32(focal))
    if not (math.isfinite(focal) and focal > 0.0):
        raise ValueError(f"focal must be positive and finite, got {camera_intrinsics[2]!r}")
    cam = camera_struct(height, width, focal, camera_pose.rotation, camera_pose.translation)
    if not all(math.isfinite(x) for x in cam.pose):
        raise ValueError("the camera pose is not finite")
    return cam


def mesh_arrays(mesh, what: str) -> Tuple[Tensor, Tensor]:
    """The checked (vertices float32 [V, 3], faces int64 [T, 3]) of a Mesh on one HIP device, detached and contiguous; ``what`` is the
    public function the messages name."""
    vertices, faces = mesh.vertices, mesh.faces
    if not (torch.is_tensor(vertices) and torch.is_tensor(faces)):
        raise ValueError(f"{what} takes a Mesh of tensors")
    if not vertices.is_cuda or not faces.is_cuda:
        raise ValueError(f"{what} takes a mesh on a HIP device (got vertices on {vertices.device}, faces on {faces.device}); there is no CPU path")
    if vertices.device != faces.device:
        raise ValueError(f"vertices are on {vertices.device}, faces on {faces.device}")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("vertices must be a float32 tensor of shape [V, 3]")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
        raise ValueError("faces must be an integer tensor of shape [T, 3]")
    return vertices.detach().contiguous(), faces.detach().to(torch.int64).contiguous()


def require_finite_vertices(vertices: Tensor) -> None:
    """(one host read)"""
    if not bool(torch.isfinite(vertices).all()):
        raise ValueError("the mesh has vertices that are not finite")


def require_faces_in_range(status: Tensor, num_vertices: int) -> None:
    """the status word a mesh kernel raises when a face indexes outside the vertices (one host read)"""
    if int(status.item()):
        raise ValueError(f"faces index outside [0, {num_vertices})")


def raster_visibility(cam: "_lib.RFCamera", vertices: Tensor, faces: Tensor, near: float, flags: int, visibility: Tensor, status: Tensor) -> None:
    """one view's visibility pass into ``visibility`` (int64 [H, W], overwritten); a face outside the vertices raises ``status``"""
    visibility.fill_(-1)  # all ones: nothing hit
    rc = _lib.load().rf_mesh_raster_visibility(C.byref(cam), vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), int(faces.shape[0]), near, flags,
                                               visibility.data_ptr(), status.data_ptr(), stream(vertices.device))
    _lib.check(rc, "rf_mesh_raster_visibility")


def segment_offsets(keys: Tensor, count: int) -> Tensor:
    """int64 [count + 1]: where the entries of each key in [0, count) begin once they are sorted by key (``keys`` in any order)"""
    counts = torch.bincount(keys, minlength=count) if count and keys.numel() else torch.zeros(count, dtype=torch.int64, device=keys.device)
    offsets = torch.zeros(count + 1, dtype=torch.int64, device=keys.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets
