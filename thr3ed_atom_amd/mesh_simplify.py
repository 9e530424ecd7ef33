"""Mesh simplification by vertex clustering with quadric-error representatives (Lindstrom 2000 over Garland and Heckbert's
quadrics): the reduction step between ``extract_mesh`` -- millions of sliver triangles of a Kuhn-tetrahedra surface -- and a mesh
somebody can open.  A lattice of cubic cells is laid over the mesh, the vertices of a cell collapse to ONE representative placed
where the planes of the cell's faces meet (so creases and corners stay sharp where a plain mean rounds them off), and the faces
are rewritten: collapsed ones dropped, duplicates merged, the rest in a canonical order.  One sort per list and one segmented HIP
pass (rf_mesh_cluster_keys / rf_mesh_cluster_vertices of csrc/mesh_simplify_kernels.hip); the sorts, the uniques and the face
rewrite are torch ops on the device.  The result is a function of the input alone -- two runs give the same bits -- and is pinned
index for index by the float64 model of tests/mesh_simplify_model.py.  DESIGN.md section 20 has the contract and the measurements.

Not done here: opposed pairs (a, b, c) and (a, c, b) -- a thin sheet whose two sides fell into the same cells -- both survive;
edge-collapse simplification is another tool (texture baking: thr3ed_atom_amd/texture.py)."""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal, ops
from .mesh import Mesh

MAX_TARGET_RESOLUTION = 4096  # target_faces: the largest number of cells along the longest axis that the bisection tries


class MeshSimplifyStats(NamedTuple):
    cell_size: float            # the float32 cell edge h that was used
    clusters: int               # occupied cells
    vertices: int               # clusters that a kept face references: the output vertices
    input_faces: int
    collapsed_faces: int        # faces with two corners in one cluster
    merged_duplicates: int      # faces that repeated an oriented triple already there
    faces: int                  # input_faces - collapsed_faces - merged_duplicates
    cluster_of_vertex: Tensor   # int64 [V_in]: the output vertex an input vertex went to, -1 when no kept face uses its cluster


class _Lattice(NamedTuple):
    origin: np.ndarray  # float32 [3]
    h: np.float32
    r: np.float32
    cells: np.ndarray   # int64 [3]


def _check_mesh(mesh: Mesh):
    vertices, faces = _marshal.mesh_arrays(mesh, "simplify_mesh")
    if vertices.shape[0] >= 2**31:
        raise ValueError("simplify_mesh takes fewer than 2^31 vertices")
    for name, t in (("colours", mesh.colours), ("normals", mesh.normals)):
        if t is not None and (not torch.is_tensor(t) or t.device != vertices.device or t.dtype != torch.float32 or tuple(t.shape) != tuple(vertices.shape)):
            raise ValueError(f"{name} must be a float32 tensor of the vertices' shape on their device")
    contiguous = lambda t: None if t is None else t.detach().contiguous()
    return Mesh(vertices, faces, contiguous(mesh.colours), contiguous(mesh.normals))


def cell_size_for(extent, resolution: int) -> np.float32:
    """h(n) of ``target_faces``: the float32 nearest to extent / n"""
    return np.float32(float(np.float32(extent)) / int(resolution))


def _lattice(bounds: np.ndarray, cell_size, origin) -> _Lattice:
    """the host side of the cell contract: h, r = fl32(1 / h), the origin and the cell counts n_a = k_a(max vertex) + 1"""
    h = np.float32(cell_size)
    if not (np.isfinite(h) and h > 0):
        raise ValueError(f"cell_size must be a positive finite float32 value, got {cell_size!r}")
    r = np.float32(1.0) / h
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"cell_size {cell_size!r} has no float32 reciprocal")
    low, high = bounds[0], bounds[1]
    if origin is None:
        o = low.copy()
    else:
        o = np.asarray([float(v) for v in origin], dtype=np.float32)
        if o.shape != (3,) or not np.isfinite(o).all():
            raise ValueError("origin must be three finite values")
        if (low < o).any():
            raise ValueError(f"the mesh has vertices below the origin {o.tolist()} (its minimum is {low.tolist()})")
    top = np.floor(((high - o).astype(np.float32) * r).astype(np.float32))  # floor, - and * are monotone: the largest k_a is that of the largest v_a
    if not np.isfinite(top).all() or (top + 1 > _lib.MESH_MAX_CELLS).any():
        raise ValueError(f"cell_size {float(h)} gives more than 2^20 cells along an axis")
    return _Lattice(o, h, r, top.astype(np.int64) + 1)


def _cluster_keys(vertices: Tensor, lattice: _Lattice):
    """(the distinct keys ascending [C], the cluster of every vertex [V]); torch.unique sizes its result on the host"""
    keys = torch.empty(vertices.shape[0], dtype=torch.int64, device=vertices.device)
    status = torch.zeros(1, dtype=torch.int32, device=vertices.device)
    ops.mesh_cluster_keys_raw(vertices, lattice.origin, lattice.r, lattice.cells, keys, status)
    cluster_keys, cluster = torch.unique(keys, return_inverse=True)
    if int(status.item()):
        raise ValueError("the mesh has vertices outside the cells: below the origin, or not finite")
    return cluster_keys, cluster


def _cluster_faces(cluster: Tensor, faces: Tensor, num_clusters: int):
    """the faces over CLUSTER indices in canonical form (collapsed ones dropped, smallest index first, duplicates merged,
    lexicographic order) and the number of faces that survived the collapse"""
    mapped = cluster[faces]
    a, b, c = mapped.unbind(1)
    mapped = mapped[(a != b) & (b != c) & (a != c)]
    kept = mapped.shape[0]
    first = mapped.argmin(dim=1, keepdim=True)  # (three distinct values: one minimum)
    mapped = mapped.gather(1, (first + torch.arange(3, device=mapped.device)) % 3)  # a rotation keeps the orientation
    # lexicographic order from two stable sorts: by the third index, then by the first two as one number (C < 2^31)
    mapped = mapped[torch.sort(mapped[:, 2], stable=True).indices]
    mapped = mapped[torch.sort(mapped[:, 0] * num_clusters + mapped[:, 1], stable=True).indices]
    if kept > 1:
        fresh = torch.ones(kept, dtype=torch.bool, device=mapped.device)
        fresh[1:] = (mapped[1:] != mapped[:-1]).any(dim=1)
        mapped = mapped[fresh]
    return mapped, kept


def _cluster_lists(cluster: Tensor, faces: Tensor, num_clusters: int):
    """(members, member_begin, corners, corner_begin) of rf_mesh_cluster_vertices"""
    def segments(of: Tensor):
        order = torch.sort(of, stable=True).indices
        begin = torch.zeros(num_clusters + 1, dtype=torch.int64, device=of.device)
        torch.cumsum(torch.bincount(of, minlength=num_clusters), dim=0, out=begin[1:])
        return order, begin

    return segments(cluster) + segments(cluster[faces.reshape(-1)])


def _cluster_vertices(mesh: Mesh, lists, cluster_keys: Tensor, lattice: _Lattice, placement: str, regularisation: float):
    count, dev = cluster_keys.numel(), mesh.vertices.device
    out = [torch.empty((count, 3), dtype=torch.float32, device=dev) if t is not None else None for t in (mesh.vertices, mesh.colours, mesh.normals)]
    ops.mesh_cluster_vertices_raw(mesh.vertices, mesh.colours, mesh.normals, mesh.faces, *lists, cluster_keys, lattice.origin, lattice.h, lattice.cells,
                                  placement, regularisation, *out)
    return out


def _host_bounds(mesh: Mesh) -> np.ndarray:
    """[2, 3] float32 (min, max) of the vertices, checked with the face indices: the one host read of the input"""
    V = mesh.vertices.shape[0]
    low, high = torch.aminmax(mesh.vertices, dim=0)  # (NaN propagates through both)
    face_low, face_high = torch.aminmax(mesh.faces)
    packed = torch.cat([low.double(), high.double(), torch.stack([face_low, face_high]).double()]).cpu().numpy()  # (indices < 2^53: exact)
    if packed[6] < 0 or packed[7] >= V:
        raise ValueError(f"faces index outside [0, {V})")
    bounds = packed[:6].astype(np.float32).reshape(2, 3)
    if not np.isfinite(bounds).all():
        raise ValueError("the mesh has vertices that are not finite")
    return bounds


def _resolution_for(mesh: Mesh, bounds: np.ndarray, target_faces: int, origin):
    """the bisection that DEFINES target_faces: the number of cells n along the longest extent E, cell size
    h(n) = float32(E / n); only the key and face stages run in the probes"""
    extent = np.float32((bounds[1] - bounds[0]).astype(np.float32).max())
    if not extent > 0:
        raise ValueError("target_faces needs a mesh with a positive extent")

    def faces_at(n: int) -> int:
        lattice = _lattice(bounds, cell_size_for(extent, n), origin)
        cluster_keys, cluster = _cluster_keys(mesh.vertices, lattice)
        return int(_cluster_faces(cluster, mesh.faces, cluster_keys.numel())[0].shape[0])

    lo, hi = 1, MAX_TARGET_RESOLUTION
    if faces_at(hi) <= target_faces:
        return cell_size_for(extent, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if faces_at(mid) <= target_faces:
            lo = mid
        else:
            hi = mid
    return cell_size_for(extent, lo)


def simplify_mesh(mesh: Mesh, cell_size: Optional[float] = None, *, target_faces: Optional[int] = None, origin=None, placement: str = "quadric",
                  regularisation: float = 1e-3, return_stats: bool = False):
    """Simplify an indexed triangle mesh on a HIP device (``extract_mesh``'s output or any other; ``colours`` / ``normals`` optional) by
    vertex clustering on a lattice of cubic cells of edge ``cell_size`` that starts at ``origin`` (three values; default: the
    per-axis minimum of the vertices).  The cell of vertex v is ``k_a = floor(fl32(fl32(v_a - o_a) * fl32(1 / h)))``.  All vertices of
    a cell become one vertex: under ``placement="quadric"`` the minimiser of the summed squared (area-weighted) distances to the
    planes of the faces that touch the cell, regularised towards the cell's mean vertex by ``regularisation`` (in [1e-6, 1]) times
    the trace of the quadric and clamped to the cell; under ``"mean"`` the mean vertex.  Colours are averaged, normals summed and
    normalised.  Faces with two corners in one cell vanish, each remaining face starts at its smallest index, exact duplicates are
    merged, the faces are sorted, cells that no face uses are dropped; output vertices are in ascending cell order.

    ``target_faces=N`` instead of ``cell_size`` picks the finest lattice of ``n`` cells along the longest extent, ``n`` <= 4096, by
    bisection on the face count: the result has at most N faces whenever n = 1 does (possibly far fewer: the count is not
    monotone in n, and the bisection is the definition).

    Returns the simplified Mesh, with ``return_stats=True`` the pair (Mesh, MeshSimplifyStats).  An empty input gives an empty mesh.
    ValueError: a CPU mesh, vertices below ``origin``, non-finite vertices, faces indexing outside the vertices, more than 2^20 cells
    along an axis."""
    if (cell_size is None) == (target_faces is None):
        raise ValueError("give cell_size or target_faces (one of the two)")
    if placement not in _lib.MESH_PLACEMENTS:
        raise ValueError(f"placement must be one of {sorted(_lib.MESH_PLACEMENTS)}, got {placement!r}")
    regularisation = float(regularisation)
    if not 1e-6 <= regularisation <= 1.0:
        raise ValueError(f"regularisation must lie in [1e-6, 1], got {regularisation!r}")
    if target_faces is not None and (isinstance(target_faces, bool) or not isinstance(target_faces, (int, np.integer)) or int(target_faces) < 0):
        raise ValueError(f"target_faces must be a non-negative integer, got {target_faces!r}")
    if cell_size is not None and not (math.isfinite(float(cell_size)) and float(cell_size) > 0):
        raise ValueError(f"cell_size must be positive and finite, got {cell_size!r}")
    mesh = _check_mesh(mesh)
    dev = mesh.vertices.device
    V, T = mesh.vertices.shape[0], mesh.faces.shape[0]
    with torch.no_grad():
        if V == 0 or T == 0:
            empty = lambda t: None if t is None else torch.empty((0, 3), dtype=torch.float32, device=dev)
            out = Mesh(empty(mesh.vertices), torch.empty((0, 3), dtype=torch.int64, device=dev), empty(mesh.colours), empty(mesh.normals))
            h = float(np.float32(cell_size)) if cell_size is not None else 0.0
            stats = MeshSimplifyStats(h, 0, 0, T, T, 0, 0, torch.full((V,), -1, dtype=torch.int64, device=dev))
            return (out, stats) if return_stats else out
        bounds = _host_bounds(mesh)
        if target_faces is not None:
            cell_size = _resolution_for(mesh, bounds, int(target_faces), origin)
        lattice = _lattice(bounds, cell_size, origin)
        cluster_keys, cluster = _cluster_keys(mesh.vertices, lattice)
        count = cluster_keys.numel()
        faces, kept = _cluster_faces(cluster, mesh.faces, count)
        lists = _cluster_lists(cluster, mesh.faces, count)
        representatives = _cluster_vertices(mesh, lists, cluster_keys, lattice, placement, regularisation)
        # the clusters that a kept face uses, in ascending key order, are the output vertices
        used = torch.zeros(count, dtype=torch.bool, device=dev)
        used[faces.reshape(-1)] = True
        position = torch.cumsum(used, dim=0) - 1
        position = torch.where(used, position, torch.full_like(position, -1))
        out = Mesh(*(None if t is None else t[used] for t in (representatives[0], None, representatives[1], representatives[2])))
        out = out._replace(faces=position[faces])
        stats = MeshSimplifyStats(float(lattice.h), count, int(out.vertices.shape[0]), T, T - kept, kept - int(faces.shape[0]), int(faces.shape[0]), position[cluster])
    return (out, stats) if return_stats else out
