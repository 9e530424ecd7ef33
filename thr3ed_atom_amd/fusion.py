"""TSDF fusion of posed depth views (Curless and Levoy 1996) and watertight meshes from it: the surface the VIEWS see instead of the
level set of the density.  Every node of a lattice accumulates, per view, the truncated signed distance between the depth the view
holds at the node's pixel and the node's own camera depth; every ray that passes a node in free space carves it; the zero set of
the mean is meshed by ``extract_mesh``.  The accumulation is the HIP kernel of csrc/fusion_kernels.hip (rf_fuse_depth_views); the
rule, the kernel and the measurements are in DESIGN.md section 26, the error bound in docs/fusion_errors.md.

The depth images may come from anywhere -- an RGB-D capture, ``render_mesh``, ``render_geometry`` of a trained field
(``fuse_field_views``) -- as long as depth is the ray parameter of ``cast_rays`` (= the camera-space depth).
"""
import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal
from .camera import CameraPose
from .composable import _SH_C0
from .constants import EXTRA_ACCUMULATED_WEIGHTS
from .mesh import Mesh, extract_mesh
from .texture import _view_chunk
from .voxels import VoxelGrid, VoxelGridLocation, VoxelSize

MAX_VIEWS = _lib.FUSE_MAX_VIEWS  # per rf_fuse_depth_views call
MAX_DIM = _lib.FUSE_MAX_DIM
DEFAULT_TRUNCATION_VOXELS = 3.0
COLOUR_CLAMP = 1.0 / 512.0  # to_voxel_grid: colours are clamped to [1/512, 1 - 1/512] before the logit


class FusedVolume(NamedTuple):
    tsdf: Tensor                  # [X, Y, Z] float32 in [-1, 1]: distance to the surface / truncation, positive in front of it
    observed: Tensor              # [X, Y, Z] int32: views that saw the node in front of, or within the truncation behind, their surface
    hidden: Tensor                # [X, Y, Z] int32: views in which the node lies more than the truncation behind the surface
    colour: Optional[Tensor]      # [X, Y, Z, 3] float32: mean colour of the views that saw the node within the truncation (0 without one)
    colour_count: Optional[Tensor]  # [X, Y, Z] int32: how many those were
    aabb_min: tuple               # 3 floats (float32 values): the box of the lattice
    aabb_max: tuple
    truncation: float

    def to_voxel_grid(self, storage: str = "reference", fill_colour: float = 0.5) -> VoxelGrid:
        """The volume as a VoxelGrid with Identity/Identity density callables (mode "identity"): ``densities = -tsdf`` (positive inside),
        3 SH-degree-0 features ``logit(clamp(colour, 1/512, 1 - 1/512)) / C0`` (``fill_colour`` for the nodes without a colour sample
        and for a volume fused without images), voxel size and location such that the grid's nodes are the fusion's nodes.  Identity,
        not ReLU: ``extract_mesh`` places a vertex by linear interpolation of the ACTIVATED values on an edge, and a ReLU at level 0
        would snap every vertex to a node."""
        fill = float(fill_colour)
        if not (math.isfinite(fill) and 0.0 <= fill <= 1.0):
            raise ValueError(f"fill_colour must be in [0, 1], got {fill_colour!r}")
        dims = tuple(int(v) for v in self.tsdf.shape)
        colour = torch.full(dims + (3,), fill, dtype=torch.float32, device=self.tsdf.device)
        if self.colour is not None:
            colour = torch.where((self.colour_count > 0)[..., None], self.colour, colour)
        colour = colour.clamp(COLOUR_CLAMP, 1.0 - COLOUR_CLAMP)
        features = torch.log(colour / (1.0 - colour)) / _SH_C0
        size = VoxelSize(*[(hi - lo) / n for lo, hi, n in zip(self.aabb_min, self.aabb_max, dims)])
        location = VoxelGridLocation(*[(hi + lo) / 2 for lo, hi in zip(self.aabb_min, self.aabb_max)])
        grid = VoxelGrid((-self.tsdf)[..., None].contiguous(), features, size, location, density_preactivation=torch.nn.Identity(),
                         density_postactivation=torch.nn.Identity(), expected_density_scale=1.0, storage=storage)
        for (lo, hi), mine_lo, mine_hi in zip(grid.aabb, self.aabb_min, self.aabb_max):  # (Python floats: the float32 values come back)
            if float(np.float32(lo)) != mine_lo or float(np.float32(hi)) != mine_hi:
                raise ValueError(f"the box [{mine_lo}, {mine_hi}] is not reproduced by a voxel size and a location ([{lo}, {hi}])")
        return grid

    def extract_mesh(self, subdivisions: int = 1) -> Mesh:
        """The closed mesh of the fused surface: ``extract_mesh(self.to_voxel_grid(), 0.0, subdivisions)``"""
        return extract_mesh(self.to_voxel_grid(), 0.0, subdivisions)


def _float32_triple(values, name: str) -> tuple:
    values = tuple(float(np.float32(v)) for v in values)
    if len(values) != 3 or not all(math.isfinite(v) for v in values):
        raise ValueError(f"{name} must be 3 finite floats, got {values!r}")
    return values


def _grid_dims(grid_dims) -> tuple:
    dims = tuple(grid_dims)
    if len(dims) != 3 or any(isinstance(d, bool) or int(d) != d or not 1 <= int(d) <= MAX_DIM for d in dims):
        raise ValueError(f"grid_dims must be 3 integers in [1, {MAX_DIM}], got {grid_dims!r}")
    dims = tuple(int(d) for d in dims)
    if dims[0] * dims[1] * dims[2] >= 2**31:
        raise ValueError(f"grid_dims {dims} hold 2^31 nodes or more")
    return dims


def default_truncation(aabb_min, aabb_max, grid_dims, voxels: float = DEFAULT_TRUNCATION_VOXELS) -> float:
    """``voxels`` x the longest voxel edge of the lattice"""
    return float(voxels) * max((hi - lo) / n for lo, hi, n in zip(aabb_min, aabb_max, grid_dims))


def finalise(tsdf_sum: Tensor, counts: Tensor, colour_sum: Optional[Tensor], aabb_min, aabb_max, truncation: float) -> FusedVolume:
    """The sums of rf_fuse_depth_views as a FusedVolume: tsdf = tsdf_sum / observed where observed > 0; -1 where no view observed the
    node and at least one hides it (behind a surface in every view that saw it, the node stays solid: no interior shell appears);
    +1 elsewhere (a node never seen is empty).  colour = colour_sum.rgb / colour_sum.w where w > 0, else 0."""
    observed, hidden = counts[..., 0], counts[..., 1]
    one = torch.ones((), dtype=torch.float32, device=tsdf_sum.device)
    tsdf = torch.where(observed > 0, tsdf_sum / observed.clamp(min=1).to(torch.float32), torch.where(hidden > 0, -one, one))
    colour = colour_count = None
    if colour_sum is not None:
        weight = colour_sum[..., 3]
        colour = torch.where((weight > 0)[..., None], colour_sum[..., :3] / weight.clamp(min=1.0)[..., None], torch.zeros((), dtype=torch.float32, device=weight.device))
        colour_count = weight.to(torch.int32)
    return FusedVolume(tsdf, observed.contiguous(), hidden.contiguous(), colour, colour_count, tuple(aabb_min), tuple(aabb_max), float(truncation))


def fuse_depth_views(depths, poses: Sequence, camera_intrinsics, aabb_min, aabb_max, grid_dims, *, truncation: Optional[float] = None, alphas=None, images=None,
                     min_alpha: float = 0.5, near: float = 0.0, carve: bool = True) -> FusedVolume:
    """Fuse posed depth images into a truncated signed distance volume of ``grid_dims`` nodes in the box [``aabb_min``, ``aabb_max``],
    the nodes placed as a VoxelGrid's are.  ``depths`` [N, H, W] (or N [H, W] / [H, W, 1]) float32 on a HIP device: the ray parameter of
    the first surface per pixel as ``RenderOut.depth`` and ``MeshRender.depth`` hold it; a pixel with depth <= 0 -- or, with ``alphas``
    [N, H, W], with alpha < ``min_alpha`` -- saw nothing, a pixel whose depth is not finite says nothing.  ``poses``: N CameraPose of
    one ``camera_intrinsics``.  ``images`` [N, H, W, 3]: colours to average at the surface.

    Per node and view, views in order: the node is projected to its nearest pixel; a pixel that saw nothing carves the node (tsdf
    +1; ``carve=False``: the view is skipped); otherwise sdf = depth - the node's camera depth, the view is counted as hiding the
    node when sdf < -``truncation`` and adds min(1, sdf / truncation) otherwise.  ``truncation`` defaults to 3 x the longest voxel edge;
    nodes in front of ``near`` are skipped.  Any number of views, 16 per launch; the sums are those of one long loop, two calls give
    the same bits.  Returns the finalised FusedVolume (``finalise``).
    ValueError: counts or shapes that do not match, CPU tensors, a box that is not finite or empty, dims outside [1, 4096],
    ``truncation`` not positive and finite, ``min_alpha`` outside [0, 1], ``near`` negative or not finite, and what
    ``_marshal.checked_camera`` refuses."""
    poses = list(poses)
    N = len(poses)
    dims = _grid_dims(grid_dims)
    lo, hi = _float32_triple(aabb_min, "aabb_min"), _float32_triple(aabb_max, "aabb_max")
    if not all(b > a and math.isfinite(float(np.float32(b) - np.float32(a))) for a, b in zip(lo, hi)):
        raise ValueError(f"the box must have aabb_max > aabb_min on every axis, got {lo} .. {hi}")
    if truncation is None:
        truncation = default_truncation(lo, hi, dims)
    truncation = float(np.float32(truncation))
    if not (math.isfinite(truncation) and truncation > 0.0):
        raise ValueError(f"truncation must be positive and finite, got {truncation!r}")
    near = _marshal.non_negative(near, "near")
    min_alpha = float(np.float32(min_alpha))
    if not 0.0 <= min_alpha <= 1.0:
        raise ValueError(f"min_alpha must be in [0, 1], got {min_alpha!r}")
    H, W = int(camera_intrinsics[0]), int(camera_intrinsics[1])
    cams = [_marshal.checked_camera(pose, camera_intrinsics) for pose in poses]
    if not N:  # (the intrinsics are checked all the same)
        _marshal.checked_camera(CameraPose(torch.eye(3), torch.zeros(3, 1)), camera_intrinsics)
    given = {}
    for name, items, last in (("depths", depths, None), ("alphas", alphas, None), ("images", images, 3)):
        if items is None:
            given[name] = None
            continue
        if len(items) != N:
            raise ValueError(f"{len(items)} {name}, {N} poses: the counts must match")
        stack = _view_chunk(items, 0, N, None, name) if N or torch.is_tensor(items) else torch.zeros((0, H, W) + ((3,) if last else ()))
        if last is None and stack.dim() == 4 and stack.shape[-1] == 1:
            stack = stack[..., 0]
        shape = (N, H, W) + ((3,) if last else ())
        if tuple(stack.shape) != shape:
            raise ValueError(f"the {name} of {N} views of {H} x {W} pixels must have shape {shape}, got {tuple(stack.shape)}")
        _marshal.require_hip(stack, name)
        given[name] = stack.detach().to(torch.float32).contiguous()
    depths, alphas, images = given["depths"], given["alphas"], given["images"]
    if depths is None:
        raise ValueError("fuse_depth_views needs depths")
    dev = depths.device
    for name, other in (("alphas", alphas), ("images", images)):
        if other is not None and other.device != dev:
            raise ValueError(f"depths are on {dev}, {name} on {other.device}")
    lib = _lib.load()
    with torch.no_grad():
        tsdf_sum = torch.zeros(dims, dtype=torch.float32, device=dev)
        counts = torch.zeros(dims + (2,), dtype=torch.int32, device=dev)
        colour_sum = torch.zeros(dims + (4,), dtype=torch.float32, device=dev) if images is not None else None
        box_lo, box_hi, cdims = _lib.float3(lo), _lib.float3(hi), (C.c_int32 * 3)(*dims)
        stream = _marshal.stream(dev)
        flags = _lib.FUSE_CARVE if carve else 0
        for first in range(0, N, MAX_VIEWS):
            last = min(first + MAX_VIEWS, N)
            chunk = (_lib.RFCamera * (last - first))(*cams[first:last])
            rc = lib.rf_fuse_depth_views(box_lo, box_hi, cdims, last - first, chunk, depths[first:last].data_ptr(), _marshal.ptr(None if alphas is None else alphas[first:last]),
                                         _marshal.ptr(None if images is None else images[first:last]), near, truncation, min_alpha, flags, tsdf_sum.data_ptr(),
                                         counts.data_ptr(), _marshal.ptr(colour_sum), stream)
            _lib.check(rc, "rf_fuse_depth_views")
        return finalise(tsdf_sum, counts, colour_sum, lo, hi, truncation)


def fuse_field_views(vol_mod, poses: Sequence, camera_intrinsics, grid_dims=None, *, truncation: Optional[float] = None, quantile: float = 0.5, images: bool = True,
                     render_overrides: Optional[dict] = None) -> FusedVolume:
    """``fuse_depth_views`` of the field's own geometry: for every pose ``vol_mod.render_geometry(pose, camera_intrinsics, quantile)``
    gives the depth (the median depth at 0.5; 0 where the ray never accumulates the quantile: a miss) and its accumulated weight the
    alpha plane, exactly as ``fit_mesh_to_field_views`` gathers them and ``evaluate_mesh_against_field`` scores them; with ``images`` the
    colour of ``vol_mod.render`` without jitter is averaged at the surface.  The box is the model's grid's and so are, by default, the
    dims.  ``render_overrides`` are passed on to the renders (``white_bkgd`` concerns colour only)."""
    grid = vol_mod.thre3d_repr
    aabb = grid.aabb
    dims = tuple(grid.grid_dims) if grid_dims is None else grid_dims
    overrides = dict(render_overrides or {})
    geometry_overrides = {k: v for k, v in overrides.items() if k != "white_bkgd"}
    depths, accs, colours = [], [], []
    with torch.no_grad():
        for pose in poses:
            geometry = vol_mod.render_geometry(pose, camera_intrinsics, quantile=quantile, **geometry_overrides)
            dev = geometry.depth.device
            depths.append(geometry.depth[..., 0].to(dev, torch.float32))
            accs.append(geometry.extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].to(dev, torch.float32))
            if images:
                colours.append(vol_mod.render(pose, camera_intrinsics, **{**overrides, "perturb_sampled_points": False}).colour.to(dev, torch.float32))
    return fuse_depth_views(depths, list(poses), camera_intrinsics, [r[0] for r in aabb], [r[1] for r in aabb], dims, truncation=truncation, alphas=accs,
                            images=colours if images else None)
