"""A rasteriser for the meshes the export chain writes (``extract_mesh`` -> ``simplify_mesh`` -> ``bake_texture`` -> ``write_obj``), and
the metrics that say how far such an asset is from the field it came from.  ``render_mesh`` turns (Mesh, TextureBake, pose,
intrinsics) into an image with exactly the camera convention of ``cast_rays`` -- the pixel's ray is the one the field's renders use,
operation for operation -- by two HIP launches (rf_mesh_raster_visibility / rf_mesh_raster_shade of csrc/mesh_raster_kernels.hip): a
64-bit atomic-minimum visibility buffer over the triangles, then one lane per pixel.  tests/mesh_raster_model.py restates the rule
independently in float64 numpy; DESIGN.md section 22 has the contract and the measurements, docs/mesh_raster_errors.md the error bound.

Not done here: clipping at the near plane (a face with a corner nearer than ``near`` is dropped whole), anti-aliasing, mip-mapping,
transparency, lighting."""
import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal
from ._marshal import ptr
from .camera import CameraIntrinsics, CameraPose, mse2psnr
from .constants import EXTRA_ACCUMULATED_WEIGHTS
from .mesh import Mesh
from .metrics import ssim
from .texture import TextureBake

MAX_EDGE = _lib.RASTER_MAX_EDGE


class MeshRender(NamedTuple):
    colour: Optional[Tensor]        # [H, W, 3] float32; None when there is neither a bake nor vertex colours
    depth: Tensor                   # [H, W, 1] float32: the ray parameter of the hit (RenderOut.depth's quantity), 0 where nothing was hit
    mask: Tensor                    # [H, W] bool
    face_ids: Tensor                # [H, W] int32, -1 where nothing was hit
    barycentrics: Optional[Tensor]  # [H, W, 3] float32 (0 where nothing was hit)


def _check_raster_mesh(mesh: Mesh, bake: Optional[TextureBake]):
    vertices, faces = _marshal.mesh_arrays(mesh, "render_mesh")
    dev, V, T = vertices.device, vertices.shape[0], faces.shape[0]
    uvs = texture = colours = None
    if bake is not None:
        uvs, texture = bake.uvs, bake.texture
        if not (torch.is_tensor(uvs) and torch.is_tensor(texture)) or uvs.device != dev or texture.device != dev:
            raise ValueError(f"the mesh is on {dev}, the bake is not")
        if tuple(uvs.shape) != (T, 3, 2) or uvs.dtype != torch.float32:
            raise ValueError(f"the bake has UVs of shape {tuple(uvs.shape)}, the mesh has {T} faces")
        if texture.dim() != 3 or texture.shape[2] != 3 or texture.dtype != torch.float32:
            raise ValueError("the bake's texture must be a float32 tensor of shape [H, W, 3]")
        if T and not (1 <= texture.shape[0] <= MAX_EDGE and 1 <= texture.shape[1] <= MAX_EDGE):
            raise ValueError(f"the bake's texture is {texture.shape[1]} x {texture.shape[0]} texels: each edge must be in [1, {MAX_EDGE}]")
        uvs, texture = uvs.detach().contiguous(), texture.detach().contiguous()
    elif mesh.colours is not None:
        colours = mesh.colours
        if not torch.is_tensor(colours) or colours.device != dev:
            raise ValueError(f"the mesh is on {dev}, its colours are not")
        if tuple(colours.shape) != (V, 3) or colours.dtype != torch.float32:
            raise ValueError("colours must be a float32 tensor of shape [V, 3]")
        colours = colours.detach().contiguous()
    return vertices, faces, uvs, texture, colours


_camera = _marshal.checked_camera


def render_mesh(mesh: Mesh, camera_pose: CameraPose, camera_intrinsics: CameraIntrinsics, bake: Optional[TextureBake] = None, *, near: float = 0.0,
                white_bkgd: bool = False, cull_backfaces: bool = False, barycentrics: bool = False) -> MeshRender:
    """Rasterise ``mesh`` (vertices float32 [V, 3], faces [T, 3], on a HIP device) from a posed pinhole camera.  Pixel (i, j) has the
    ray of ``cast_rays``; a face covers it when the ray's three edge values (the triple products d . (p_a x p_b) of the corners seen
    from the camera) are all >= 0 or all <= 0 and do not sum to 0: edges are inclusive, shared edges are watertight (both faces
    evaluate the shared edge with the same bits), zero-area and edge-on faces are never drawn.  The nearest face wins, the lower
    face index on exact depth ties.  ``depth`` is the ray parameter of the hit -- the quantity ``RenderOut.depth`` holds.  A face
    with any corner at a camera depth below ``near`` is not drawn at all (no clipping).  ``cull_backfaces``: only faces whose
    (v1 - v0) x (v2 - v0) points towards the camera are drawn (the outside of an ``extract_mesh`` surface).

    The colour comes from ``bake`` when given -- a bilinear fetch of ``bake.texture`` at the interpolated per-corner ``bake.uvs``, texel
    coordinates (u W_t - 1/2, (1 - v) H_t - 1/2), clamped to the image -- else from ``mesh.colours`` interpolated over the face; with
    neither, ``colour`` is None.  Pixels without a hit get the background (black, or white with ``white_bkgd``), depth 0, face id -1.
    Two launches, integer atomics only: two calls give the same bits.  An empty mesh gives the background without a launch.
    ValueError: a CPU mesh, mesh and bake on different devices, non-finite vertices, faces indexing outside the vertices, a bake
    whose ``uvs`` do not match the faces, an image edge outside [1, 16384], a focal or ``near`` that is not finite or not positive /
    negative, a pose that is not finite."""
    vertices, faces, uvs, texture, colours = _check_raster_mesh(mesh, bake)
    cam = _camera(camera_pose, camera_intrinsics)
    near = _marshal.non_negative(near, "near")
    H, W, T, V, dev = cam.height, cam.width, faces.shape[0], vertices.shape[0], vertices.device
    background = 1.0 if white_bkgd else 0.0
    has_colour = texture is not None or colours is not None
    if T == 0:
        return MeshRender(torch.full((H, W, 3), background, dtype=torch.float32, device=dev) if has_colour else None,
                          torch.zeros((H, W, 1), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.bool, device=dev),
                          torch.full((H, W), -1, dtype=torch.int32, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev) if barycentrics else None)
    lib = _lib.load()
    with torch.no_grad():
        _marshal.require_finite_vertices(vertices)
        flags = (_lib.FLAG_WHITE_BKGD if white_bkgd else 0) | (_lib.RASTER_CULL_BACKFACES if cull_backfaces else 0)
        stream = _marshal.stream(dev)
        visibility = torch.empty((H, W), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _marshal.raster_visibility(cam, vertices, faces, near, flags, visibility, status)
        _marshal.require_faces_in_range(status, V)
        colour = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if has_colour else None
        depth = torch.empty((H, W, 1), dtype=torch.float32, device=dev)
        face_ids = torch.empty((H, W), dtype=torch.int32, device=dev)
        bary = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if barycentrics else None
        th, tw = (0, 0) if texture is None else (texture.shape[0], texture.shape[1])
        rc = lib.rf_mesh_raster_shade(C.byref(cam), vertices.data_ptr(), V, faces.data_ptr(), T, visibility.data_ptr(), ptr(uvs), ptr(texture), th, tw,
                                      ptr(colours), flags, ptr(colour), depth.data_ptr(), face_ids.data_ptr(), ptr(bary), stream)
        _lib.check(rc, "rf_mesh_raster_shade")
    return MeshRender(colour, depth, face_ids >= 0, face_ids, bary)


def evaluate_mesh_against_field(mesh: Mesh, bake: Optional[TextureBake], vol_mod, poses: Sequence[CameraPose], camera_intrinsics: CameraIntrinsics,
                                **render_overrides) -> Dict[str, object]:
    """How far an exported mesh is from the field it came from, over the cameras ``poses``: every view is rendered both ways on the same
    background -- ``render_mesh(mesh, pose, camera_intrinsics, bake)`` and ``vol_mod.render`` / ``vol_mod.render_geometry`` with
    ``render_overrides`` -- and compared.  Returns the means over the views of ``psnr`` and ``ssim`` (``rf.ssim``; "valid" windows,
    "same" for images below 11 pixels) of the colours, ``depth_l1`` (mean |mesh depth - median depth| over the pixels both cover;
    NaN for a view without any) and ``mask_iou`` (mesh mask against accumulated weight > 1/2; 1 when both are empty), and
    ``per_image``: the list of the same four numbers per view.  Views whose ``depth_l1`` is NaN do not enter its mean."""
    cfg = getattr(vol_mod, "render_config", None)
    white = bool(render_overrides.get("white_bkgd", getattr(cfg, "white_bkgd", False)))
    height, width, _ = camera_intrinsics
    padding = "valid" if min(int(height), int(width)) >= 11 else "same"
    per_image = []
    with torch.no_grad():
        for pose in poses:
            mine = render_mesh(mesh, pose, camera_intrinsics, bake, white_bkgd=white)
            if mine.colour is None:
                raise ValueError("evaluate_mesh_against_field needs a bake or vertex colours")
            field = vol_mod.render(pose, camera_intrinsics, **render_overrides)
            geometry = vol_mod.render_geometry(pose, camera_intrinsics, **{k: v for k, v in render_overrides.items() if k != "white_bkgd"})
            reference = field.colour.to(mine.colour.device, torch.float32).contiguous()
            mse = torch.mean((mine.colour - reference) ** 2)
            psnr = float("inf") if float(mse) == 0.0 else float(mse2psnr(float(mse)))
            field_mask = geometry.extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0] > 0.5
            both = mine.mask & field_mask
            union = int((mine.mask | field_mask).sum())
            depth_l1 = float((mine.depth[..., 0] - geometry.depth[..., 0]).abs()[both].mean()) if bool(both.any()) else float("nan")
            per_image.append({"psnr": psnr, "ssim": float(ssim(mine.colour, reference, padding=padding)), "depth_l1": depth_l1,
                              "mask_iou": float(int(both.sum()) / union) if union else 1.0})
    def mean(key):
        vals = [p[key] for p in per_image if not math.isnan(p[key])]
        return float(np.mean(vals)) if vals else float("nan")
    return {"psnr": mean("psnr"), "ssim": mean("ssim"), "depth_l1": mean("depth_l1"), "mask_iou": mean("mask_iou"), "per_image": per_image}


def read_obj(path_stem: str, device=None) -> Tuple[Mesh, TextureBake]:
    """Read back the triple ``write_obj`` writes -- ``path_stem``.obj, .mtl and the texture its ``map_Kd`` names (.png, or the .npy
    written when PIL is absent) -- as (Mesh, TextureBake) on ``device`` (default: the CPU).  Only that dialect: v / vt / vn / f
    a/ta[/na] lines with three fresh vt per face in face order.  The texture comes back as uint8 / 255; ``opacity`` is None; the
    atlas layout (patch, block, cols, rows) is recovered from the first face's UVs."""
    out_dir, stem = os.path.dirname(os.path.abspath(path_stem)), os.path.basename(path_stem)
    v, vt, vn, f = [], [], [], []
    mtllib = None
    with open(os.path.join(out_dir, stem + ".obj")) as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            kind = parts[0]
            if kind == "v":
                v.append(parts[1:4])
            elif kind == "vt":
                vt.append(parts[1:3])
            elif kind == "vn":
                vn.append(parts[1:4])
            elif kind == "f":
                if len(parts) != 4:
                    raise ValueError(f"{path_stem}.obj: only triangles are read")
                f.append([c.split("/") for c in parts[1:]])
            elif kind == "mtllib":
                mtllib = parts[1]
    if mtllib is None:
        raise ValueError(f"{path_stem}.obj names no material library")
    vertices = np.array(v, dtype=np.float64).astype(np.float32).reshape(-1, 3)
    T = len(f)
    corners = np.array(f, dtype=np.int64).reshape(T, 3, -1)
    if T and corners.shape[2] < 2:
        raise ValueError(f"{path_stem}.obj: faces carry no texture coordinates")
    faces = corners[..., 0] - 1 if T else np.zeros((0, 3), np.int64)
    uv_all = np.array(vt, dtype=np.float64).astype(np.float32).reshape(-1, 2)
    if T and not np.array_equal(corners[..., 1].reshape(-1), np.arange(1, 3 * T + 1)):
        raise ValueError(f"{path_stem}.obj: not the vt order write_obj writes")
    if len(uv_all) != 3 * T or (T and (faces.min() < 0 or faces.max() >= len(vertices))):
        raise ValueError(f"{path_stem}.obj: malformed")
    uvs = uv_all.reshape(T, 3, 2)
    normals = np.array(vn, dtype=np.float64).astype(np.float32).reshape(-1, 3) if len(vn) == len(vertices) and vn else None
    texture_name = None
    with open(os.path.join(out_dir, mtllib)) as fh:
        for line in fh:
            parts = line.split()
            if parts and parts[0] == "map_Kd":
                texture_name = parts[1]
    if texture_name is None:
        raise ValueError(f"{mtllib} names no map_Kd texture")
    if texture_name.endswith(".npy"):
        image = np.load(os.path.join(out_dir, texture_name))
    else:
        from PIL import Image

        image = np.asarray(Image.open(os.path.join(out_dir, texture_name)).convert("RGB"))
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError(f"{texture_name}: not a uint8 RGB image")
    patch = block = cols = rows = 0
    if T:
        patch = int(round(float(uvs[0, 1, 0] - uvs[0, 0, 0]) * image.shape[1])) + 1
        block = patch + _lib.TEXTURE_GUTTER
        cols, rows = image.shape[1] // block, image.shape[0] // block
    dev = torch.device("cpu") if device is None else torch.device(device)
    mesh = Mesh(torch.from_numpy(vertices).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev), None, None if normals is None else torch.from_numpy(normals).to(dev))
    texture = torch.from_numpy(image.astype(np.float32) / np.float32(255.0)).to(dev)
    return mesh, TextureBake(texture, None, torch.from_numpy(np.ascontiguousarray(uvs)).to(dev), patch, block, cols, rows)
