"""Connected-component labelling and floater removal of a trained field (the "keep the largest piece" / "drop pieces under N
voxels" step of every mesh pipeline built on a density grid): label the connected components of the nodes that hold density
(``label_components``: rf_label_components, three HIP launches) and empty every component that is too small or ranks too low
(``remove_small_components``: a torch gather that builds the keep mask, then the existing rf_prune_grid launch).  This removes
what neither total variation nor visibility pruning does -- a floater that a camera did see and that carries weight -- so that
``extract_mesh`` loses its detached shells and ``content_bounds`` / ``tighten_voxel_grid`` stop keeping the box of one speck in a
corner.  DESIGN.md section 19 has the contract, the kernels and the measurements.

Under the default 26-connectivity two occupied nodes that are corners of one cell are neighbours, so no cell has a corner in a
kept component and a corner in a removed one: removal never changes the interpolated field in a cell that touches a kept
component."""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops
from .voxels import as_kernel_grid


class Components(NamedTuple):
    labels: Tensor  # int32 [X, Y, Z] on the device: -1, or the smallest plain linear index of the node's component
    roots: Tensor   # int64 [C]: the labels in use, by size descending, ties by root ascending
    sizes: Tensor   # int64 [C]: the node count of each


class ComponentStats(NamedTuple):
    components: int          # before the call
    removed_components: int
    kept_nodes: int          # occupied nodes of the kept components
    removed_nodes: int


def _grid_of(model_or_grid):
    return as_kernel_grid(getattr(model_or_grid, "thre3d_repr", model_or_grid))


def _check_arguments(grid, threshold, connectivity, what: str):
    threshold, connectivity = float(threshold), int(connectivity)
    if not (threshold >= 0.0):
        raise ValueError("threshold must be non-negative (and not NaN)")
    if connectivity not in _lib.CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {_lib.CONNECTIVITIES}, got {connectivity}")
    mode = grid.density_mode
    if mode is None:
        raise ValueError(f"{what} needs one of the density activations the HIP kernels implement")
    if mode == "softplus" and threshold == 0.0:
        raise ValueError(f"every node of a softplus grid has sigma > 0: {what} needs a positive threshold there")
    first, _ = grid.kernel_tensors()
    if not first.is_cuda:
        raise ValueError(f"{what} takes a grid on a HIP device (got {first.device}); there is no CPU path")
    return threshold, connectivity, mode, first


def rank_components(roots, sizes):
    """the order of ``Components``: size descending, ties by root ascending (host arrays in, a permutation out)"""
    roots, sizes = np.asarray(roots, dtype=np.int64), np.asarray(sizes, dtype=np.int64)
    return np.lexsort((roots, -sizes))


def kept_components(sizes_ranked, min_nodes: Optional[int], keep_largest: Optional[int]):
    """bool [C] over components in ``Components`` order: kept iff size >= min_nodes (when given) and rank < keep_largest (when given)"""
    sizes_ranked = np.asarray(sizes_ranked, dtype=np.int64)
    keep = np.ones(sizes_ranked.shape, dtype=bool)
    if min_nodes is not None:
        keep &= sizes_ranked >= int(min_nodes)
    if keep_largest is not None:
        keep &= np.arange(sizes_ranked.size) < int(keep_largest)
    return keep


def label_components(grid_or_model, threshold: float = 0.0, connectivity: int = 26) -> Components:
    """Components(labels, roots, sizes) of the nodes whose OWN activated density ``post(pre(D * expected_density_scale))`` exceeds
    ``threshold`` (strictly: the predicate of ``content_bounds``), connected through ``connectivity`` = 6 (faces), 18 (+ edges) or 26
    (+ corners) neighbours.  ``labels`` is canonical -- the smallest plain index ``(x Y + y) Z + z`` of the component, -1 off it --
    so it does not depend on the storage, the launch order or the run.  Every storage, any VoxelGrid-like module
    (ForeignVoxelGridView); HIP grids only (a CPU grid raises ValueError).  The component list is compacted on the device
    (``nonzero`` sizes its result on the host); ``roots`` and ``sizes`` stay there.  A softplus grid needs a positive threshold."""
    grid = _grid_of(grid_or_model)
    threshold, connectivity, _, first = _check_arguments(grid, threshold, connectivity, "label_components")
    dims = tuple(int(v) for v in grid.grid_dims)
    with torch.no_grad():
        labels = torch.empty(dims, dtype=torch.int32, device=first.device)
        node_sizes = torch.empty(labels.numel(), dtype=torch.int32, device=first.device)
        ops.label_components_raw(grid, threshold, connectivity, labels, node_sizes)
        roots = node_sizes.nonzero().flatten()  # ascending
        sizes = node_sizes[roots].to(torch.int64)
        order = torch.sort(sizes, descending=True, stable=True).indices  # (stable: equal sizes stay in root order)
    return Components(labels, roots[order], sizes[order])


def remove_small_components(grid_or_model, threshold: float = 0.0, connectivity: int = 26, min_nodes: Optional[int] = None,
                            keep_largest: Optional[int] = None, fill_density: Optional[float] = None) -> ComponentStats:
    """Empty, in place and under ``no_grad``, every component of ``label_components(grid, threshold, connectivity)`` that is not
    kept.  A component is KEPT iff its size is at least ``min_nodes`` (when given) and its rank -- by size descending, ties by root
    ascending -- is below ``keep_largest`` (when given); at least one of the two must be given, both >= 1.  The nodes of a removed
    component get the raw density ``min(D, fill_density)`` exactly as ``prune_voxel_grid`` writes it (the same rf_prune_grid launch
    with a 0 / 1 mask): the default fill is 0 for ReLU, |.| and identity grids (|.|: 0 is the only fill), a softplus grid must name
    one (e.g. -10).  Kept components, unoccupied nodes, every feature and the padding of bricked storage keep their bits.  One host
    read, of the small ``roots`` / ``sizes`` vectors; nothing is written when nothing is removed.  Afterwards the occupancy mask and
    the split shadow are marked stale.  Returns ComponentStats(components, removed_components, kept_nodes, removed_nodes)."""
    grid = _grid_of(grid_or_model)
    _check_arguments(grid, threshold, connectivity, "remove_small_components")
    if min_nodes is None and keep_largest is None:
        raise ValueError("give min_nodes, keep_largest or both")
    for name, value in (("min_nodes", min_nodes), ("keep_largest", keep_largest)):
        if value is not None and int(value) < 1:
            raise ValueError(f"{name} must be at least 1")
    mode = grid.density_mode
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
        found = label_components(grid, threshold, connectivity)
        roots, sizes = torch.stack([found.roots, found.sizes]).cpu().numpy()  # the one host read
        keep = kept_components(sizes, min_nodes, keep_largest)
        removed = roots[~keep]
        if removed.size:
            # M = 1 for unoccupied nodes and nodes of kept components, 0 for nodes of removed ones; rf_prune_grid empties M <= 0
            dev = found.labels.device
            weight = torch.ones(found.labels.numel() + 1, dtype=torch.float32, device=dev)  # (slot 0: label -1)
            weight[torch.from_numpy(removed).to(dev) + 1] = 0.0
            mask = weight[found.labels.to(torch.int64) + 1]
            ops.prune_grid_raw(grid, mask, 0.0, 0, fill_density)
        # the densities changed behind autograd's back (raw-pointer write): the occupancy mask and the split shadow are stale
        grid.invalidate_occupancy()
    return ComponentStats(int(roots.size), int(removed.size), int(sizes[keep].sum()), int(sizes[~keep].sum()))
