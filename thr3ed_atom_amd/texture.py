"""Texture baking of a field onto a triangle mesh, and textured OBJ export: the step after ``simplify_mesh`` that gives a small mesh
back what the field knows about its appearance.  Every triangle gets its own right-angled patch of ``patch`` texel centres per leg
in a uniform atlas -- vertex clustering leaves triangles of about one cell, so nothing needs unwrapping, packing or searching:
integer arithmetic maps texel -> triangle -> 3-D point -- and every texel holds a short composited ray through the field along the
triangle's normal, sampled by ONE fused HIP launch (rf_texture_bake of csrc/texture_kernels.hip).  The layout below is restated
independently in float64 numpy by tests/texture_model.py; DESIGN.md section 21 has the contract and the measurements,
docs/texture_errors.md the error bound.

Not done here: chart atlases with shared seams, mip-safe gutters beyond the one texel this layout has, a normal map, baking by
rendering from the training cameras.  (The rasteriser that looks at the result is thr3ed_atom_amd/mesh_raster.py.)"""
import ctypes as C
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .mesh import Mesh, to8b
from .voxels import as_kernel_grid

MIN_PATCH, MAX_PATCH, GUTTER = _lib.TEXTURE_MIN_PATCH, _lib.TEXTURE_MAX_PATCH, _lib.TEXTURE_GUTTER
MAX_SAMPLES, MAX_EDGE = _lib.TEXTURE_MAX_SAMPLES, _lib.TEXTURE_MAX_EDGE


class TextureBake(NamedTuple):
    texture: Tensor            # [H, W, 3] float32 in [0, 1]; image row 0 is the top
    opacity: Optional[Tensor]  # [H, W] float32: the accumulated weight of the texel's short ray
    uvs: Tensor                # [T, 3, 2] float32 per corner, v = 1 at the top of the image (OBJ)
    patch: int
    block: int                 # patch + 4: the edge of the square that holds two triangles
    cols: int
    rows: int


class AtlasLayout(NamedTuple):
    patch: int
    block: int
    cols: int
    rows: int
    width: int
    height: int


def atlas_layout(num_faces: int, patch: int, cols: Optional[int] = None) -> AtlasLayout:
    """blocks of ``patch + 4`` texels, two triangles per block, ``cols`` blocks per row (default ceil(sqrt(blocks)))"""
    if isinstance(patch, bool) or not isinstance(patch, (int, np.integer)) or not MIN_PATCH <= int(patch) <= MAX_PATCH:
        raise ValueError(f"patch must be an integer in [{MIN_PATCH}, {MAX_PATCH}], got {patch!r}")
    patch, num_faces = int(patch), int(num_faces)
    block = patch + GUTTER
    blocks = (num_faces + 1) // 2
    if cols is None:
        cols = math.isqrt(blocks)
        cols += cols * cols < blocks
    elif isinstance(cols, bool) or not isinstance(cols, (int, np.integer)) or int(cols) < 1:
        raise ValueError(f"cols must be a positive integer, got {cols!r}")
    cols = int(cols)
    rows = -(-blocks // cols) if cols else 0
    if cols * block > MAX_EDGE or rows * block > MAX_EDGE:
        raise ValueError(f"the atlas would be {cols * block} x {rows * block} texels: more than {MAX_EDGE} along an edge (use a smaller patch or fewer faces)")
    return AtlasLayout(patch, block, cols, rows, cols * block, rows * block)


def corner_texels(layout: AtlasLayout, num_faces: int) -> np.ndarray:
    """int64 [T, 3, 2]: (column, row) in the image of the texel whose centre is corner c of face t"""
    P, B = layout.patch, layout.block
    t = np.arange(int(num_faces), dtype=np.int64)
    blk, upper = t // 2, (t % 2).astype(bool)
    lower_c = np.array([[1, 1], [P, 1], [1, P]], dtype=np.int64)
    upper_c = np.array([[P + 2, P + 2], [3, P + 2], [P + 2, 3]], dtype=np.int64)
    inside = np.where(upper[:, None, None], upper_c[None], lower_c[None])
    origin = np.stack([(blk % max(layout.cols, 1)) * B, (blk // max(layout.cols, 1)) * B], axis=-1)
    return inside + origin[:, None, :]


def corner_uvs(layout: AtlasLayout, num_faces: int) -> np.ndarray:
    """float32 [T, 3, 2]: u = (c + 1/2) / W, v = 1 - (r + 1/2) / H of the corner texels"""
    cr = corner_texels(layout, num_faces).astype(np.float64)
    if not num_faces:
        return np.zeros((0, 3, 2), np.float32)
    u = (cr[..., 0] + 0.5) / layout.width
    v = 1.0 - (cr[..., 1] + 0.5) / layout.height
    return np.stack([u, v], axis=-1).astype(np.float32)


def _check_bake_mesh(mesh: Mesh):
    vertices, faces = mesh.vertices, mesh.faces
    if not (torch.is_tensor(vertices) and torch.is_tensor(faces)):
        raise ValueError("bake_texture takes a Mesh of tensors")
    if not vertices.is_cuda or not faces.is_cuda:
        raise ValueError(f"bake_texture takes a mesh on a HIP device (got vertices on {vertices.device}, faces on {faces.device}); there is no CPU path")
    if vertices.device != faces.device:
        raise ValueError(f"vertices are on {vertices.device}, faces on {faces.device}")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("vertices must be a float32 tensor of shape [V, 3]")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
        raise ValueError("faces must be an integer tensor of shape [T, 3]")
    return vertices.detach().contiguous(), faces.detach().to(torch.int64).contiguous()


def bake_texture(mesh: Mesh, grid_or_model, patch: int = 8, *, reach: Optional[float] = None, samples: int = 16, diffuse: bool = False,
                 cols: Optional[int] = None, opacity: bool = True) -> TextureBake:
    """Bake the appearance of a field onto ``mesh`` (vertices float32 [V, 3], faces [T, 3], on the field's HIP device) as a
    per-triangle texture atlas.  Face t goes into block t // 2 of ``patch + 4`` texels square (even faces the lower-left right-angled
    patch, odd ones the upper-right), ``cols`` blocks per image row (default ceil(sqrt(blocks))).  A texel's point p is the affine
    image of its centre in its face; its value is a short ray along the face's unit normal n, from ``reach`` outside to ``reach``
    inside in ``samples`` midpoint samples, composited like a render with the surface point's own colour as background:
    ``sum_s w_s c(q_s) + (1 - sum_s w_s) c(p)``, ``c(x) = sigmoid(sum_k Y_k(-n) f_k(x))`` (``diffuse=True``: ``sigmoid(C0 f_0(x))``, the
    colour ``extract_mesh`` writes).  ``reach`` is in world units (default: twice the largest voxel edge); 0 gives exactly c(p).

    ``grid_or_model``: a VoxelGrid on any storage, a VolumetricModel, or a module with the reference VoxelGrid's attribute names.
    Returns a TextureBake: ``texture`` [H, W, 3] and ``opacity`` [H, W] (None with ``opacity=False``) on the device -- texels that no
    face owns are 0 in both -- and the per-corner ``uvs`` [T, 3, 2] (v = 1 at image row 0, as OBJ wants them).  One launch, no
    atomics: two calls give the same bits.  An empty mesh gives a 0 x 0 bake without a launch.
    ValueError: a CPU mesh or grid, mesh and grid on different devices, non-finite vertices, faces indexing outside the vertices,
    patch outside [2, 64], samples outside [1, 256], a negative or non-finite reach, cols too small for the faces' blocks to stay
    within 16384 texels per edge."""
    vertices, faces = _check_bake_mesh(mesh)
    grid = as_kernel_grid(getattr(grid_or_model, "thre3d_repr", grid_or_model))
    first = grid.kernel_tensors()[0]
    if not first.is_cuda:
        raise ValueError(f"bake_texture takes a field on a HIP device (got {first.device}); there is no CPU path")
    if first.device != vertices.device:
        raise ValueError(f"the mesh is on {vertices.device}, the field on {first.device}")
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= int(samples) <= MAX_SAMPLES:
        raise ValueError(f"samples must be an integer in [1, {MAX_SAMPLES}], got {samples!r}")
    if reach is None:
        reach = 2.0 * max((hi - lo) / n for (lo, hi), n in zip(grid.aabb, grid.grid_dims))
    reach = float(np.float32(reach))
    if not (math.isfinite(reach) and reach >= 0.0):
        raise ValueError(f"reach must be non-negative and finite, got {reach!r}")
    T, V, dev = faces.shape[0], vertices.shape[0], vertices.device
    layout = atlas_layout(T, patch, cols)
    uvs = torch.from_numpy(corner_uvs(layout, T)).to(dev)
    if T == 0:
        return TextureBake(torch.empty((0, 0, 3), dtype=torch.float32, device=dev), torch.empty((0, 0), dtype=torch.float32, device=dev) if opacity else None,
                           uvs, layout.patch, layout.block, layout.cols, layout.rows)
    lib = _lib.load()
    with torch.no_grad():
        if not bool(torch.isfinite(vertices).all()):
            raise ValueError("the mesh has vertices that are not finite")
        texture = torch.empty((layout.height, layout.width, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((layout.height, layout.width), dtype=torch.float32, device=dev) if opacity else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rf_grid = grid.to_rf_grid()  # (waits for parameters still arriving, like a render)
        flags = _lib.FLAG_RENDER_DIFFUSE if diffuse else 0
        rc = lib.rf_texture_bake(C.byref(rf_grid), vertices.data_ptr(), V, faces.data_ptr(), T, layout.patch, layout.cols, layout.rows, reach, int(samples),
                                 flags, texture.data_ptr(), None if alpha is None else alpha.data_ptr(), status.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "rf_texture_bake")
        if int(status.item()):
            raise ValueError(f"faces index outside [0, {V})")
    return TextureBake(texture, alpha, uvs, layout.patch, layout.block, layout.cols, layout.rows)


def write_obj(mesh: Mesh, bake: TextureBake, path_stem: str) -> None:
    """Write ``path_stem``.obj (v, three vt per face, vn when the mesh has normals, f a/ta/na, mtllib, usemtl), ``path_stem``.mtl
    (map_Kd) and ``path_stem``.png (the texture through ``to8b``; ``path_stem``.npy with the uint8 array when PIL is absent)."""
    stem = os.path.basename(path_stem)
    out_dir = os.path.dirname(os.path.abspath(path_stem))
    os.makedirs(out_dir, exist_ok=True)
    v = mesh.vertices.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype(np.int64).reshape(-1, 3)
    uv = bake.uvs.detach().cpu().numpy().astype(np.float32).reshape(-1, 2)
    if uv.shape[0] != 3 * f.shape[0]:
        raise ValueError(f"the bake has UVs for {uv.shape[0] // 3} faces, the mesh has {f.shape[0]}")
    nrm = None if mesh.normals is None else mesh.normals.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
    image = to8b(bake.texture.detach().cpu().numpy())
    try:
        from PIL import Image

        texture_name = stem + ".png"
        Image.fromarray(image).save(os.path.join(out_dir, texture_name))
    except ImportError:
        texture_name = stem + ".npy"
        np.save(os.path.join(out_dir, texture_name), image)
    with open(os.path.join(out_dir, stem + ".mtl"), "w") as fh:
        fh.write(f"newmtl {stem}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {texture_name}\n")
    lines = [f"mtllib {stem}.mtl", f"usemtl {stem}"]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    lines += ["vt %.9g %.9g" % tuple(t) for t in uv.tolist()]
    if nrm is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(n) for n in nrm.tolist()]
    a, ta = f + 1, np.arange(1, 3 * len(f) + 1, dtype=np.int64).reshape(-1, 3)
    if nrm is not None:
        lines += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (x[0], t[0], x[0], x[1], t[1], x[1], x[2], t[2], x[2]) for x, t in zip(a.tolist(), ta.tolist())]
    else:
        lines += ["f %d/%d %d/%d %d/%d" % (x[0], t[0], x[1], t[1], x[2], t[2]) for x, t in zip(a.tolist(), ta.tolist())]
    with open(os.path.join(out_dir, stem + ".obj"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
