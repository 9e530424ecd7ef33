"""Content bounds, crop and resample of a field, and AABB tightening (what DVGO does after its coarse stage): find the index box of
the nodes that hold density (``content_bounds``: one HIP launch, rf_node_bounds), move the field into another box -- an exact crop
(``crop_voxel_grid``) or a general re-grid (``resample_voxel_grid``), both one launch of rf_resample_grid -- and spend a node budget
inside the content box instead of the box training started with (``tighten_voxel_grid``).  A grid on the CPU takes a plain torch
restatement of the same definitions, so the host logic can be exercised without a GPU.  DESIGN.md section 15 has the contract, both
kernels and the measurements.

Geometry: a grid of n nodes per axis with voxel size v and centre c covers [c - n v / 2, c + n v / 2]; node i sits at the centre of
its voxel, lo + (i + 1/2) v (the render maps the box to [-1, 1] and interpolates with align_corners=False)."""
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops
from .voxels import (AxisAlignedBoundingBox, ForeignVoxelGridView, VoxelGrid, VoxelGridLocation, VoxelSize, as_kernel_grid,
                     scale_voxel_grid_with_required_output_size)


class TightenStats(NamedTuple):
    old_dims: Tuple[int, int, int]
    new_dims: Tuple[int, int, int]
    old_aabb: AxisAlignedBoundingBox
    new_aabb: AxisAlignedBoundingBox
    passing_nodes: int


def _grid_of(model_or_grid):
    return as_kernel_grid(getattr(model_or_grid, "thre3d_repr", model_or_grid))


def _module_of(grid):
    """the module that carries voxel_size / get_config_dict (the grid itself, or the module behind a foreign view)"""
    return grid.module if isinstance(grid, ForeignVoxelGridView) else grid


def _reference_tensors(grid) -> Tuple[Tensor, Tensor]:
    """(densities [X,Y,Z,1], features [X,Y,Z,F]) in the reference layout, detached, whatever the storage"""
    m = _module_of(grid)
    return m.densities.detach(), m.features.detach()


def _new_grid(grid, densities: Tensor, features: Tensor, voxel_size: VoxelSize, grid_location: VoxelGridLocation) -> VoxelGrid:
    config = dict(_module_of(grid).get_config_dict())
    config["grid_location"] = grid_location
    return VoxelGrid(densities, features, voxel_size, **config, storage=grid.storage)


def _activated(raw: Tensor, rho: float, mode: str) -> Tensor:
    """sigma_n = post(pre(D_n * rho)) in float32, the kernels' helpers restated"""
    pre = raw.to(torch.float32) * torch.tensor(rho, dtype=torch.float32)
    if mode == "abs":
        return pre.abs()
    if mode == "relu":
        return torch.clamp_min(pre, 0.0)
    if mode == "softplus":
        return torch.where(pre > 20.0, pre, torch.log1p(torch.exp(pre)))
    return pre


def content_bounds(grid, threshold: float = 0.0):
    """((x0, y0, z0), (x1, y1, z1), count): the inclusive index box of the nodes whose OWN activated density
    ``post(pre(D * expected_density_scale))`` exceeds ``threshold`` (strictly; a node's value: no interpolation) and their number, or
    ``None`` when no node does.  One launch of rf_node_bounds on the GPU (exact: integer atomics) and one host read of its seven
    values.  Every storage, any VoxelGrid-like module.  Under softplus every node has sigma > 0, so ``threshold == 0`` is refused
    there: name a positive one."""
    grid = _grid_of(grid)
    threshold = float(threshold)
    if not (threshold >= 0.0):
        raise ValueError("threshold must be non-negative (and not NaN)")
    mode = grid.density_mode
    if mode is None:
        raise ValueError("content_bounds needs one of the density activations the HIP kernels implement")
    if mode == "softplus" and threshold == 0.0:
        raise ValueError("every node of a softplus grid has sigma > 0: content_bounds needs a positive threshold there")
    dims = tuple(int(v) for v in grid.grid_dims)
    first, _ = grid.kernel_tensors()
    with torch.no_grad():
        if first.is_cuda:
            bounds = torch.tensor([*dims, -1, -1, -1], dtype=torch.int32, device=first.device)
            count = torch.zeros(1, dtype=torch.int64, device=first.device)
            ops.node_bounds_raw(grid, threshold, bounds, count)
            values, n = bounds.tolist(), int(count.item())
        else:
            dens = _reference_tensors(grid)[0][..., 0]
            passing = _activated(dens, float(grid._expected_density_scale), mode) > torch.tensor(threshold, dtype=torch.float32)
            n = int(passing.sum())
            values = [*dims, -1, -1, -1]
            if n:
                idx = passing.nonzero()
                values = [*idx.min(dim=0).values.tolist(), *idx.max(dim=0).values.tolist()]
    if n == 0:
        return None
    return tuple(values[:3]), tuple(values[3:]), n


def _resample_cpu(densities: Tensor, features: Tensor, dims, scale, offset, fill: float) -> Tuple[Tensor, Tensor]:
    """rf_resample_grid restated with torch on reference-layout CPU tensors (float32; the same index and weight definitions, the
    corners added in the same order)"""
    vol = torch.cat([densities, features], dim=-1).to(torch.float32)
    src = vol.shape[:3]
    axes = []
    for a in range(3):
        # s = fmaf(scale, i, offset): the product and the sum are exact in float64, so this is ONE rounding to float32
        s = (torch.arange(dims[a], dtype=torch.float64) * float(np.float32(scale[a])) + float(np.float32(offset[a]))).to(torch.float32)
        outside = (s < -0.5) | (s > src[a] - 0.5)
        s = s.clamp(0.0, float(src[a] - 1))
        i0 = s.floor().to(torch.int64).clamp_max(src[a] - 1)
        i1 = (i0 + 1).clamp_max(src[a] - 1)
        lam = s - i0.to(torch.float32)
        axes.append((i0, i1, 1.0 - lam, lam, outside))
    out = None
    for k in range(8):
        d = (k >> 2, (k >> 1) & 1, k & 1)
        ix, iy, iz = (axes[a][d[a]] for a in range(3))
        wx, wy, wz = (axes[a][2 + d[a]] for a in range(3))
        w = ((wx[:, None, None] * wy[None, :, None]) * wz[None, None, :])[..., None]
        term = vol[ix[:, None, None], iy[None, :, None], iz[None, None, :]] * w
        out = term if out is None else out + term
    outside = axes[0][4][:, None, None] | axes[1][4][None, :, None] | axes[2][4][None, None, :]
    empty = torch.zeros(vol.shape[-1], dtype=torch.float32)
    empty[0] = fill
    out = torch.where(outside[..., None], empty, out)
    return out[..., :1].contiguous(), out[..., 1:].contiguous()


def _resample_into(grid, dims, scale, offset, fill: float, voxel_size: VoxelSize, grid_location: VoxelGridLocation) -> VoxelGrid:
    dims = tuple(int(v) for v in dims)
    first, _ = grid.kernel_tensors()
    with torch.no_grad():
        if first.is_cuda:
            new = _new_grid(grid, torch.empty((*dims, 1), dtype=torch.float32, device=first.device),
                            torch.empty((*dims, int(grid._num_features)), dtype=torch.float32, device=first.device), voxel_size, grid_location)
            ops.resample_grid_raw(grid, new, scale, offset, fill)
            return new
        dens, feat = _resample_cpu(*_reference_tensors(grid), dims, scale, offset, fill)
        return _new_grid(grid, dens, feat, voxel_size, grid_location)


def crop_voxel_grid(grid, lo, hi, margin: int = 1) -> VoxelGrid:
    """A new VoxelGrid holding the nodes ``[lo - margin, hi + margin]`` (inclusive indices per axis, clipped to the grid) of ``grid``:
    same voxel size, storage, activations, ``expected_density_scale`` and ``tunable``, and a ``grid_location`` that keeps every kept
    node where it was in the world.  One launch of rf_resample_grid with scale 1 and integer offsets: a bit-exact copy."""
    grid = _grid_of(grid)
    margin = int(margin)
    if margin < 0:
        raise ValueError("margin must not be negative")
    dims = tuple(int(v) for v in grid.grid_dims)
    voxel = VoxelSize(*(float(v) for v in _module_of(grid).voxel_size))
    first, last = [], []
    for a in range(3):
        i0, i1 = max(int(lo[a]) - margin, 0), min(int(hi[a]) + margin, dims[a] - 1)
        if i0 > i1:
            raise ValueError(f"empty crop on axis {a}: lo {tuple(lo)}, hi {tuple(hi)}, dims {dims}")
        first.append(i0)
        last.append(i1)
    location = VoxelGridLocation(*(float(grid._aabb[a][0]) + (first[a] + last[a] + 1) / 2 * voxel[a] for a in range(3)))
    new_dims = tuple(last[a] - first[a] + 1 for a in range(3))
    return _resample_into(grid, new_dims, (1.0, 1.0, 1.0), tuple(float(i) for i in first), 0.0, voxel, location)


def resample_map(src_aabb, src_voxel_size, grid_location, voxel_size, grid_dims):
    """(scale [3], offset [3]) of rf_resample_grid for a destination lattice given by its centre, voxel size and dims: float64
    arithmetic, rounded once to float32.  scale_a = v_dst / v_src, offset_a = (lo_dst - lo_src) / v_src + scale_a / 2 - 1/2."""
    scale, offset = [], []
    for a in range(3):
        v_src, v_dst = float(src_voxel_size[a]), float(voxel_size[a])
        lo_dst = float(grid_location[a]) - int(grid_dims[a]) * v_dst / 2
        sc = v_dst / v_src
        scale.append(float(np.float32(sc)))
        offset.append(float(np.float32((lo_dst - float(src_aabb[a][0])) / v_src + 0.5 * sc - 0.5)))
    return tuple(scale), tuple(offset)


def resample_voxel_grid(grid, grid_location, voxel_size, grid_dims, fill_density: Optional[float] = None) -> VoxelGrid:
    """The general re-grid: a new VoxelGrid of ``grid_dims`` nodes with ``voxel_size`` centred at ``grid_location`` whose raw
    channels are ``grid``'s, trilinearly interpolated at the new nodes' world positions; a node outside ``grid``'s box becomes
    ``(fill_density, features 0)``.  The default fill is 0; a softplus grid has no raw density with sigma = 0 and must name one
    (e.g. -10), as for ``prune_voxel_grid``.  One launch of rf_resample_grid."""
    grid = _grid_of(grid)
    mode = grid.density_mode
    if fill_density is None:
        if mode == "softplus":
            raise ValueError("a softplus grid has no raw density with sigma = 0: pass fill_density (e.g. -10.0)")
        fill_density = 0.0
    fill_density = float(fill_density)
    if math.isnan(fill_density):
        raise ValueError("fill_density must not be NaN")
    dims = tuple(int(v) for v in grid_dims)
    voxel = VoxelSize(*(float(v) for v in voxel_size))
    location = VoxelGridLocation(*(float(v) for v in grid_location))
    if min(dims) < 1 or not all(math.isfinite(v) and v > 0.0 for v in voxel) or not all(math.isfinite(v) for v in location):
        raise ValueError("grid_dims must be >= 1, voxel_size finite and positive, grid_location finite")
    scale, offset = resample_map(grid._aabb, _module_of(grid).voxel_size, location, voxel, dims)
    return _resample_into(grid, dims, scale, offset, fill_density, voxel, location)


def tightened_dims(dims, voxel_size, num_nodes: int) -> Tuple[int, int, int]:
    """DVGO's rule: ``num_nodes`` cubic voxels inside the box of ``dims`` nodes of ``voxel_size``:
    dims_a = max(2, round(extent_a / cbrt(volume / num_nodes)))"""
    extent = [int(n) * float(v) for n, v in zip(dims, voxel_size)]
    edge = (extent[0] * extent[1] * extent[2] / int(num_nodes)) ** (1.0 / 3.0)
    return tuple(max(2, int(math.floor(e / edge + 0.5))) for e in extent)


def tighten_voxel_grid(grid, threshold: float = 0.0, margin: int = 1, num_nodes: Optional[int] = None):
    """(new_grid, TightenStats): ``grid`` cropped to the box of its content -- ``content_bounds(grid, threshold)`` plus ``margin``
    nodes -- and, when ``num_nodes`` is given, resampled inside that box to about ``num_nodes`` cubic voxels
    (``tightened_dims``; ``scale_voxel_grid_with_required_output_size`` does the resampling, as at a stage transition).  A field
    without a passing node is returned as it is, with ``passing_nodes == 0``."""
    kernel_grid = _grid_of(grid)
    old_dims = tuple(int(v) for v in kernel_grid.grid_dims)
    old_aabb = AxisAlignedBoundingBox(*kernel_grid._aabb)
    if num_nodes is not None and int(num_nodes) < 1:
        raise ValueError("num_nodes must be positive")
    found = content_bounds(kernel_grid, threshold)
    if found is None:
        return getattr(grid, "thre3d_repr", grid), TightenStats(old_dims, old_dims, old_aabb, old_aabb, 0)
    lo, hi, count = found
    new = crop_voxel_grid(kernel_grid, lo, hi, margin)
    if num_nodes is not None:
        target = tightened_dims(new.grid_dims, new.voxel_size, int(num_nodes))
        if target != tuple(new.grid_dims):
            with torch.no_grad():
                new = scale_voxel_grid_with_required_output_size(new, target)
    return new, TightenStats(old_dims, tuple(int(v) for v in new.grid_dims), old_aabb, new.aabb, count)
