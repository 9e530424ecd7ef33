"""Visibility statistics and weight-based pruning of a trained field (what Plenoxels and DVGO clean their grids by): render the
training views, record per node the largest compositing weight any ray ever gave it (``node_max_weights``: one HIP launch per
view, rf_node_max_weight), then empty the nodes that stay below a threshold -- and, with threshold 0, the nodes no view ever saw:
interior junk behind opaque surfaces, leftovers of the initialisation outside every frustum (``prune_voxel_grid``: rf_prune_grid).
Total variation only smooths such floaters; this removes them, so that ``extract_mesh`` loses interior shells and specks and
``build_occupancy`` marks more cells empty.  DESIGN.md section 13 has the contract, the kernels and the measurements."""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.distributed as dist
from torch import Tensor

from . import ops
from . import distributed as rfdist
from .voxels import as_kernel_grid


class PruneStats(NamedTuple):
    kept: int
    pruned: int


def _grid_of(model_or_grid):
    return as_kernel_grid(getattr(model_or_grid, "thre3d_repr", model_or_grid))


def _views(poses):
    """[M, 3, 4] camera-to-world tensor, or a sequence of CameraPose / [3, 4] tensors -> list of (rotation, translation)"""
    out = []
    for p in poses:
        if hasattr(p, "rotation") and hasattr(p, "translation"):
            out.append((p.rotation, p.translation))
        else:
            p = torch.as_tensor(p)
            if tuple(p.shape) != (3, 4):
                raise ValueError(f"a pose must be a CameraPose or a [3, 4] camera-to-world matrix, got {tuple(p.shape)}")
            out.append((p[:, :3], p[:, 3]))
    return out


def node_max_weights(model_or_grid, poses, intrinsics, bounds, num_samples: int, *, render_config=None, out: Optional[Tensor] = None) -> Tensor:
    """M [X, Y, Z] (float32, plain node order): per node the largest ``w_i * b_k`` over every pixel ray of every view, with
    ``w_i = T_i alpha_i`` the compositing weight of sample i exactly as the render computes it and ``b_k`` the trilinear weight of
    the node in the sample's cell.  One launch per view, the rays generated inside the kernel; the samples are never perturbed,
    so the result is deterministic.  ``render_config`` (optional SHVoxGridRenderConfig) contributes ``optimized_sampling`` and
    ``use_occupancy_mask``.  ``out`` (zeros when not given) is only ever raised: pass the result of an earlier call to accumulate
    more views.  Under an initialised process group the views are dealt out to the ranks and M is combined with
    all_reduce(MAX) -- exact, so every rank holds the same bits as a single process would."""
    grid = _grid_of(model_or_grid)
    num_samples = int(num_samples)
    if num_samples < 1:
        raise ValueError("num_samples must be at least 1")
    height, width, focal = intrinsics
    if int(height) < 1 or int(width) < 1 or not float(focal) > 0.0:
        raise ValueError(f"bad camera intrinsics {tuple(intrinsics)}")
    near, far = float(np.float32(bounds.near)), float(np.float32(bounds.far))
    views = _views(poses)
    first, _ = grid.kernel_tensors()
    if out is None:
        out = torch.zeros(tuple(grid.grid_dims), dtype=torch.float32, device=first.device)
    elif tuple(out.shape) != tuple(grid.grid_dims) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != first.device:
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(grid.grid_dims)} on the grid's device")
    use_occupancy = bool(getattr(render_config, "use_occupancy_mask", False)) if render_config is not None else False
    flags = ops.render_flags(False, False, bool(getattr(render_config, "optimized_sampling", False)) if render_config is not None else False, use_occupancy)
    world, rank = rfdist.world_size(), rfdist.rank()
    with torch.no_grad():
        if use_occupancy and not grid.occupancy_current():
            grid.build_occupancy()
        for rotation, translation in views[rank::world]:
            rays = ops.RayBatch(None, None, num_samples, near, far, camera=(int(height), int(width), float(focal), rotation, translation))
            ops.node_max_weight_raw(grid, rays, flags, out)
        if world > 1:
            if dist.get_backend() == "nccl":
                dist.all_reduce(out, op=dist.ReduceOp.MAX)
            else:  # (gloo reduces host tensors)
                host = out.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.MAX)
                out.copy_(host)
    return out


def prune_voxel_grid(grid, max_weight: Tensor, threshold: float, dilate: int = 1, fill_density: Optional[float] = None) -> PruneStats:
    """Empty, in place, every node of ``grid`` that has no node within ``dilate`` steps (Chebyshev distance) whose ``max_weight``
    (``node_max_weights``) exceeds ``threshold`` -- strictly: ``threshold=0`` prunes exactly the nodes no sample ever weighted.  A
    pruned node's raw density becomes ``min(D, fill_density)`` (pruning never raises a density); the default fill is 0 for ReLU,
    |.| and identity grids (|.|: 0 is the only fill).  Softplus has no density with sigma = 0: name a ``fill_density`` (e.g. -10)
    there.  Features are left alone.  Works on every storage and on any VoxelGrid-like module (ForeignVoxelGridView); what hangs
    on the densities -- the occupancy mask, the split shadow of a reference-storage grid -- is marked stale.  Returns
    PruneStats(kept, pruned)."""
    grid = _grid_of(grid)
    threshold, dilate = float(threshold), int(dilate)
    if not (math.isfinite(threshold) and threshold >= 0.0):
        raise ValueError("threshold must be finite and non-negative")
    if not 0 <= dilate <= 4:
        raise ValueError("dilate must be in [0, 4]")
    mode = grid.density_mode
    if mode is None:
        raise ValueError("prune_voxel_grid needs one of the density activations the HIP kernels implement")
    if fill_density is None:
        if mode == "softplus":
            raise ValueError("a softplus grid has no raw density with sigma = 0: pass fill_density (e.g. -10.0)")
        fill_density = 0.0
    fill_density = float(fill_density)
    if math.isnan(fill_density):
        raise ValueError("fill_density must not be NaN")
    if mode == "abs" and fill_density != 0.0:
        raise ValueError("under the |.| density activation the only fill is 0")
    with torch.no_grad():
        counts = torch.zeros(2, dtype=torch.int64, device=max_weight.device)
        ops.prune_grid_raw(grid, max_weight, threshold, dilate, fill_density, counts=counts)
        # the densities changed behind autograd's back (raw-pointer write): the occupancy mask and the split shadow are stale
        grid.invalidate_occupancy()
        kept, pruned = (int(v) for v in counts.tolist())
    return PruneStats(kept, pruned)
