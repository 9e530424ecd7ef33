"""Texture baking of a field onto a triangle mesh, and textured OBJ export: the step after ``simplify_mesh`` that gives a small mesh
back what the field knows about its appearance.  Every triangle gets its own right-angled patch of ``patch`` texel centres per leg
in a uniform atlas -- vertex clustering leaves triangles of about one cell, so nothing needs unwrapping, packing or searching:
integer arithmetic maps texel -> triangle -> 3-D point.  Two ways to fill it:

``bake_texture``: every texel holds a short composited ray through the field along the triangle's normal, sampled by ONE fused HIP
launch (rf_texture_bake of csrc/texture_kernels.hip).  DESIGN.md section 21 has the contract and the measurements,
docs/texture_errors.md the error bound, tests/texture_model.py the float64 model of it and of the layout.

``bake_texture_from_views`` / ``bake_texture_from_field_views``: posed images -- the field's own renders from the poses an asset will
be viewed from, or the dataset's photographs -- are projected onto the atlas.  Per chunk of 16 views the mesh rasteriser
(thr3ed_atom_amd/mesh_raster.py) writes one depth buffer per view and ONE HIP launch (rf_texture_project_views of
csrc/texture_views_kernels.hip) projects every texel into every view: shadow-map test against that depth, weight by the viewing
angle, bilinear fetch, least-squares sums; the division is torch.  DESIGN.md section 23, docs/texture_views_errors.md,
tests/texture_views_model.py.

Not done here: chart atlases with shared seams, mip-safe gutters beyond the one texel this layout has, a normal map, per-view
exposure, blending across the seams between faces."""
import ctypes as C
import math
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal
from ._marshal import checked_camera, mesh_arrays, non_negative, ptr, require_faces_in_range, require_finite_vertices
from .camera import CameraPose
from .constants import EXTRA_ACCUMULATED_WEIGHTS
from .mesh import Mesh, to8b
from .voxels import as_kernel_grid

MIN_PATCH, MAX_PATCH, GUTTER = _lib.TEXTURE_MIN_PATCH, _lib.TEXTURE_MAX_PATCH, _lib.TEXTURE_GUTTER
MAX_SAMPLES, MAX_EDGE = _lib.TEXTURE_MAX_SAMPLES, _lib.TEXTURE_MAX_EDGE
MAX_VIEWS, MAX_COS_POWER = _lib.TEXTURE_VIEWS_MAX_VIEWS, _lib.TEXTURE_VIEWS_MAX_COS_POWER


class TextureBake(NamedTuple):
    texture: Tensor            # [H, W, 3] float32 in [0, 1]; image row 0 is the top
    opacity: Optional[Tensor]  # [H, W] float32: the accumulated weight of the texel's short ray
    uvs: Tensor                # [T, 3, 2] float32 per corner, v = 1 at the top of the image (OBJ)
    patch: int
    block: int                 # patch + 4: the edge of the square that holds two triangles
    cols: int
    rows: int


class ViewBake(NamedTuple):
    bake: TextureBake  # the texture (opacity None) with the layout and UVs of ``bake_texture``
    weight: Tensor     # [H, W] float32: sum over the views that saw the texel of omega m^2
    views: Tensor      # [H, W] int32: how many views saw the texel


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
    vertices, faces = mesh_arrays(mesh, "bake_texture")
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
    reach = non_negative(reach, "reach")
    T, V, dev = faces.shape[0], vertices.shape[0], vertices.device
    layout = atlas_layout(T, patch, cols)
    uvs = torch.from_numpy(corner_uvs(layout, T)).to(dev)
    if T == 0:
        return TextureBake(torch.empty((0, 0, 3), dtype=torch.float32, device=dev), torch.empty((0, 0), dtype=torch.float32, device=dev) if opacity else None,
                           uvs, layout.patch, layout.block, layout.cols, layout.rows)
    lib = _lib.load()
    with torch.no_grad():
        require_finite_vertices(vertices)
        texture = torch.empty((layout.height, layout.width, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((layout.height, layout.width), dtype=torch.float32, device=dev) if opacity else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rf_grid = grid.to_rf_grid()  # (waits for parameters still arriving, like a render)
        flags = _lib.FLAG_RENDER_DIFFUSE if diffuse else 0
        rc = lib.rf_texture_bake(C.byref(rf_grid), vertices.data_ptr(), V, faces.data_ptr(), T, layout.patch, layout.cols, layout.rows, reach, int(samples),
                                 flags, texture.data_ptr(), ptr(alpha), status.data_ptr(), _marshal.stream(dev))
        _lib.check(rc, "rf_texture_bake")
        require_faces_in_range(status, V)
    return TextureBake(texture, alpha, uvs, layout.patch, layout.block, layout.cols, layout.rows)


class _ViewProjector:
    """The state of one view bake: the checked mesh, the atlas, the accumulators; ``add`` takes at most 16 views at a time."""

    def __init__(self, mesh: Mesh, camera_intrinsics, patch, cols, near, depth_bias, min_cos, cos_power, two_sided, background):
        self.vertices, self.faces = mesh_arrays(mesh, "bake_texture")  # (the view bakes report the mesh in bake_texture's words)
        self.intrinsics = camera_intrinsics
        self.H, self.W = int(camera_intrinsics[0]), int(camera_intrinsics[1])
        self.T, self.V, self.dev = self.faces.shape[0], self.vertices.shape[0], self.vertices.device
        self.layout = atlas_layout(self.T, patch, cols)
        self.near, self.background = non_negative(near, "near"), non_negative(background, "background")
        min_cos = float(np.float32(min_cos))
        if not 0.0 <= min_cos < 1.0:
            raise ValueError(f"min_cos must be in [0, 1), got {min_cos!r}")
        if isinstance(cos_power, bool) or not isinstance(cos_power, (int, np.integer)) or not 0 <= int(cos_power) <= MAX_COS_POWER:
            raise ValueError(f"cos_power must be an integer in [0, {MAX_COS_POWER}], got {cos_power!r}")
        self.min_cos, self.cos_power = min_cos, int(cos_power)
        self.flags = _lib.TEXTURE_VIEWS_TWO_SIDED if two_sided else 0
        self.accum = self.count = self.visibility = self.status = None
        with torch.no_grad():
            if self.T:
                require_finite_vertices(self.vertices)
                if int(self.faces.min()) < 0 or int(self.faces.max()) >= self.V:
                    raise ValueError(f"faces index outside [0, {self.V})")
                if depth_bias is None:  # the mean edge length of the faces
                    corners = self.vertices.double()[self.faces]
                    depth_bias = float(np.float32(float((corners - corners.roll(1, dims=1)).norm(dim=-1).mean())))
                self.accum = torch.zeros((self.layout.height, self.layout.width, 4), dtype=torch.float32, device=self.dev)
                self.count = torch.zeros((self.layout.height, self.layout.width), dtype=torch.int32, device=self.dev)
                self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.depth_bias = non_negative(0.0 if depth_bias is None else depth_bias, "depth_bias")
        checked_camera(CameraPose(torch.eye(3), torch.zeros(3, 1)), camera_intrinsics)  # (the intrinsics' own errors, even with zero views)

    def add(self, images: Tensor, poses, alphas: Optional[Tensor], intrinsics=None) -> None:
        n = len(poses)
        intrinsics = [self.intrinsics] * n if intrinsics is None else intrinsics
        if any((int(intr[0]), int(intr[1])) != (self.H, self.W) for intr in intrinsics):
            raise ValueError(f"all views must have {self.H} x {self.W} pixels")
        if not 1 <= n <= MAX_VIEWS:
            raise ValueError(f"a chunk holds 1 to {MAX_VIEWS} views, got {n}")
        if tuple(images.shape) != (n, self.H, self.W, 3):
            raise ValueError(f"the images of {n} views of {self.H} x {self.W} pixels must have shape {(n, self.H, self.W, 3)}, got {tuple(images.shape)}")
        if alphas is not None and tuple(alphas.shape) != (n, self.H, self.W):
            raise ValueError(f"the alphas of {n} views of {self.H} x {self.W} pixels must have shape {(n, self.H, self.W)}, got {tuple(alphas.shape)}")
        cams = (_lib.RFCamera * n)(*[checked_camera(pose, intr) for pose, intr in zip(poses, intrinsics)])
        if not self.T:
            return
        lib = _lib.load()
        with torch.no_grad():
            images = images.detach().to(self.dev, torch.float32).contiguous()
            alphas = None if alphas is None else alphas.detach().to(self.dev, torch.float32).contiguous()
            stream = _marshal.stream(self.dev)
            if self.visibility is None:
                self.visibility = torch.empty((MAX_VIEWS, self.H, self.W), dtype=torch.int64, device=self.dev)
            for k in range(n):
                _marshal.raster_visibility(cams[k], self.vertices, self.faces, self.near, 0, self.visibility[k], self.status)
            rc = lib.rf_texture_project_views(self.vertices.data_ptr(), self.V, self.faces.data_ptr(), self.T, self.layout.patch, self.layout.cols, self.layout.rows,
                                              n, cams, images.data_ptr(), self.visibility.data_ptr(), ptr(alphas), self.near,
                                              self.depth_bias, self.min_cos, self.cos_power, self.background, self.flags, self.accum.data_ptr(),
                                              self.count.data_ptr(), self.status.data_ptr(), stream)
            _lib.check(rc, "rf_texture_project_views")

    def finish(self, fallback: Optional[TextureBake], min_weight: float) -> ViewBake:
        lay, dev = self.layout, self.dev
        uvs = torch.from_numpy(corner_uvs(lay, self.T)).to(dev)
        if fallback is not None:
            if (fallback.patch, fallback.block, fallback.cols, fallback.rows) != (lay.patch, lay.block, lay.cols, lay.rows) or \
                    tuple(fallback.texture.shape) != (lay.height if self.T else 0, lay.width if self.T else 0, 3):
                raise ValueError(f"the fallback bake has the layout (patch, block, cols, rows) = {(fallback.patch, fallback.block, fallback.cols, fallback.rows)}, "
                                 f"this bake {(lay.patch, lay.block, lay.cols, lay.rows)}")
            if fallback.texture.device != dev:
                raise ValueError(f"the mesh is on {dev}, the fallback bake on {fallback.texture.device}")
        if not self.T:
            empty = TextureBake(torch.empty((0, 0, 3), dtype=torch.float32, device=dev), None, uvs, lay.patch, lay.block, lay.cols, lay.rows)
            return ViewBake(empty, torch.empty((0, 0), dtype=torch.float32, device=dev), torch.empty((0, 0), dtype=torch.int32, device=dev))
        with torch.no_grad():
            require_faces_in_range(self.status, self.V)
            texture, weight = finalise_views(self.accum, None if fallback is None else fallback.texture.detach().to(torch.float32), min_weight)
        return ViewBake(TextureBake(texture, None, uvs, lay.patch, lay.block, lay.cols, lay.rows), weight, self.count)


def finalise_views(accum: Tensor, fallback_texture: Optional[Tensor], min_weight: float):
    """accum [H, W, 4] of rf_texture_project_views -> (texture [H, W, 3], weight [H, W]): sum / weight where weight > min_weight, the
    fallback's texel (or 0) elsewhere"""
    weight = accum[..., 3].contiguous()
    seen = weight > min_weight
    texture = accum[..., :3] / torch.where(seen, weight, torch.ones_like(weight))[..., None]
    other = torch.zeros_like(texture) if fallback_texture is None else fallback_texture
    return torch.where(seen[..., None], texture, other).contiguous(), weight


def _view_chunk(items, lo: int, hi: int, last_dim: Optional[int], what: str) -> Tensor:
    """views lo .. hi of a [N, ...] tensor or of a sequence of per-view tensors, stacked"""
    if torch.is_tensor(items):
        return items[lo:hi]
    chunk = [torch.as_tensor(x) for x in items[lo:hi]]
    if any(x.shape != chunk[0].shape or x.device != chunk[0].device for x in chunk) or (last_dim is not None and (chunk[0].dim() != 3 or chunk[0].shape[-1] != last_dim)):
        raise ValueError(f"the {what} must all have the same shape and device")
    return torch.stack(chunk)


def _intrinsics_per_view(camera_intrinsics, num_views: int):
    """one (H, W, focal) for all views, or one per view"""
    if len(camera_intrinsics) and isinstance(camera_intrinsics[0], (tuple, list)):
        if len(camera_intrinsics) != num_views:
            raise ValueError(f"{len(camera_intrinsics)} intrinsics, {num_views} poses: the counts must match")
        return list(camera_intrinsics)
    return [camera_intrinsics] * max(num_views, 1)


def bake_texture_from_views(mesh: Mesh, images, poses: Sequence, camera_intrinsics, patch: int = 8, *, alphas=None, background: float = 0.0,
                            fallback: Optional[TextureBake] = None, near: float = 0.0, depth_bias: Optional[float] = None, min_cos: float = 0.1,
                            cos_power: int = 2, two_sided: bool = False, min_weight: float = 1e-3, cols: Optional[int] = None) -> ViewBake:
    """Bake posed images onto the atlas of ``bake_texture`` (same layout, same ``uvs``: ``write_obj``, ``read_obj`` and ``render_mesh``
    take the result as it is).  ``images``: a [N, H, W, 3] tensor or a sequence of N [H, W, 3] tensors (CPU items are uploaded chunk
    by chunk), ``poses``: N CameraPose, all of ``camera_intrinsics`` (H, W, focal) -- or a sequence of N of them with one H and W --, the camera
    convention of ``cast_rays``;
    ``alphas``: None, or [N, H, W] / N [H, W] coverages m of the pixels, which are then read as m c + (1 - m) ``background``.

    A texel's point p is projected into every view (the inverse of the pixel's ray: the centre of pixel (i, j) is at (j + 1/2, i + 1/2)).
    The view counts when p lies further than ``near`` in front of it and inside the image, when the camera depth of p is at most
    ``depth_bias`` behind the depth the mesh rasteriser saw at that pixel (default: the mean edge length of the faces), and when the
    cosine between the face's normal and the direction to the camera exceeds ``min_cos`` (its magnitude with ``two_sided``); it
    enters with the weight cos^``cos_power``.  The texel is the least-squares colour sum w m (C - (1 - m) background) / sum w m^2 of the
    bilinear fetches C, m at the projection.  Texels whose weight sum is at most ``min_weight`` -- seen by no view, or only
    through near-transparent pixels -- take the ``fallback`` bake's texel (same layout required), or 0 without one.

    Works in chunks of 16 views: one visibility launch per view, ONE projection launch per chunk, no atomics, and chunking does not
    change a bit.  Returns ViewBake(bake, weight [Ht, Wt], views [Ht, Wt] int32).  An empty mesh gives a 0 x 0 bake without a launch;
    zero views give the fallback, or zeros.  ValueError: as ``bake_texture`` and ``render_mesh`` for the mesh, the intrinsics, the
    poses, ``near`` and ``patch`` / ``cols``; counts or sizes of images, poses and alphas that do not match; ``depth_bias``,
    ``background`` or ``min_weight`` negative or not finite; ``min_cos`` outside [0, 1); ``cos_power`` outside [0, 8]; a fallback of
    another layout or device."""
    N = len(poses)
    if len(images) != N or (alphas is not None and len(alphas) != N):
        raise ValueError(f"{len(images)} images, {N} poses" + ("" if alphas is None else f", {len(alphas)} alphas") + ": the counts must match")
    intrinsics = _intrinsics_per_view(camera_intrinsics, N)
    min_weight = non_negative(min_weight, "min_weight")
    projector = _ViewProjector(mesh, intrinsics[0] if N else camera_intrinsics, patch, cols, near, depth_bias, min_cos, cos_power, two_sided, background)
    for lo in range(0, N, MAX_VIEWS):
        hi = min(lo + MAX_VIEWS, N)
        projector.add(_view_chunk(images, lo, hi, 3, "images"), list(poses[lo:hi]), None if alphas is None else _view_chunk(alphas, lo, hi, None, "alphas"),
                      intrinsics[lo:hi])
    return projector.finish(fallback, min_weight)


_NORMAL_RAYS = object()


def bake_texture_from_field_views(mesh: Mesh, vol_mod, poses: Sequence, camera_intrinsics, patch: int = 8, *, fallback=_NORMAL_RAYS, min_weight: float = 1e-3,
                                  render_overrides: Optional[dict] = None, **kw) -> ViewBake:
    """``bake_texture_from_views`` of the field's own renders: every pose is rendered by ``vol_mod.render`` (a chunk of 16 at a time;
    ``render_overrides`` are passed on), the accumulated weight of ``vol_mod.render_geometry`` is the view's alpha plane -- the way
    ``evaluate_mesh_against_field`` obtains it -- and the model's background the background.  ``fallback`` defaults to
    ``bake_texture(mesh, vol_mod, patch)``; the other keywords are those of ``bake_texture_from_views``."""
    overrides = dict(render_overrides or {})
    cfg = getattr(vol_mod, "render_config", None)
    white = bool(overrides.get("white_bkgd", getattr(cfg, "white_bkgd", False)))
    min_weight = non_negative(min_weight, "min_weight")
    projector = _ViewProjector(mesh, camera_intrinsics, patch, kw.pop("cols", None), kw.pop("near", 0.0), kw.pop("depth_bias", None), kw.pop("min_cos", 0.1),
                               kw.pop("cos_power", 2), kw.pop("two_sided", False), 1.0 if white else 0.0)
    if kw:
        raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
    if fallback is _NORMAL_RAYS:
        fallback = bake_texture(mesh, vol_mod, patch, cols=projector.layout.cols if projector.T else None)
    geometry_overrides = {k: v for k, v in overrides.items() if k != "white_bkgd"}
    with torch.no_grad():
        for lo in range(0, len(poses), MAX_VIEWS):
            chunk = list(poses[lo:lo + MAX_VIEWS])
            colours = [vol_mod.render(pose, camera_intrinsics, **overrides).colour.to(projector.dev, torch.float32) for pose in chunk]
            accs = [vol_mod.render_geometry(pose, camera_intrinsics, **geometry_overrides).extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].to(projector.dev, torch.float32)
                    for pose in chunk]
            projector.add(torch.stack(colours), chunk, torch.stack(accs))
    return projector.finish(fallback, min_weight)


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
