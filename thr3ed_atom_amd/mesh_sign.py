"""Signed distance to a closed mesh, inside / outside, and the way back from a mesh to a field: ``MeshSignGrid`` puts a sign on what
``MeshDistanceGrid.closest`` finds, ``mesh_to_sdf`` samples it on the nodes of a lattice (an identity-mode ``VoxelGrid`` that
``extract_mesh`` and everything after it take as they come), ``signed_mesh_distance`` says which way one surface lies from another.
The sign is the angle-weighted pseudonormal rule of Baerentzen and Aanaes (2005): with q the closest point and F the face, edge or
vertex that holds it, sign((p - q) . N_F) -- exact for a closed, consistently oriented, edge-manifold mesh, which is what
``extract_mesh`` documents its output to be.  Per query it is ONE launch on top of the forward's (rf_mesh_signed_distance,
csrc/mesh_sign_kernels.hip); per mesh, two tables: the faces across every edge (``mesh_topology``: torch, one stable sort) and the
angle-weighted vertex normals (rf_mesh_face_pseudonormals and the gather the mesh render's backward uses: no atomics).
include/relu_field_ext.h has the contract, docs/mesh_sign_errors.md the rule, the error bounds and the decision margin,
tests/mesh_sign_model.py the numpy model, DESIGN.md section 29 the measurements.  There is no CPU path (``mesh_topology`` excepted).

Not done here: generalised winding numbers for open or non-manifold meshes (the clustered thin sheets of ``simplify_mesh``), a fused
kernel that generates the nodes of a volume itself, sparse volumes."""
import math
import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal
from .fusion import _float32_triple, _grid_dims
from .mesh import Mesh, extract_mesh
from .mesh_distance import MeshDistanceGrid, _count, sample_mesh_surface
from .mesh_distance_grad import _check_vertices, _distance
from .mesh_fit import corner_slot_lists, gather_vertex_gradients
from .voxels import VoxelGrid, VoxelGridLocation, VoxelSize

FEATURE_FACE, FEATURE_EDGE, FEATURE_VERTEX, FEATURE_NONE = 0, 1, 2, -1
PARTNER_BOUNDARY, PARTNER_NONMANIFOLD, PARTNER_INCONSISTENT = -1, -2, -3
MAX_FACES = (1 << 31) // 3  # an edge is named 3 face + k in int32
MIN_TRUNCATION_VOXELS = 1.5
SLAB_POINTS = 1 << 20       # mesh_to_sdf queries about this many nodes per call
ORIENTATIONS = ("outward", "inward", "auto")


class MeshTopology(NamedTuple):
    partners: Tensor        # int32 [T, 3]: the face across edge k (0, 1, 2 = v0 v1, v1 v2, v2 v0); -1 boundary, -2 non-manifold, -3 inconsistent
    boundary_edges: int     # undirected edges with one face
    nonmanifold_edges: int  # ... with three faces or more
    inconsistent_edges: int  # ... with two faces that run along it in the same direction
    degenerate_faces: int   # faces with a repeated vertex index or no area (float64)
    closed: bool            # at least one face and none of the three kinds of edges above
    signed_volume: float    # float64 sum of det(v0, v1, v2) / 6: positive when the normals point outward


class SignedClosestPoints(NamedTuple):
    distance: Tensor           # float32 [N]: negative inside; +inf when nothing lies within max_distance
    face: Tensor               # int64 [N]; -1 then
    point: Tensor              # float32 [N, 3]; NaN then
    feature: Optional[Tensor]  # int32 [N, 2]: (kind, index), kind 0 face / 1 edge / 2 vertex / -1 none; index = face, 3 face + edge, vertex
    normal: Optional[Tensor]   # float32 [N, 3]: the pseudonormal the sign was taken against (not normalised)


class SignedDirected(NamedTuple):
    mean: float          # of the signed distances of the source's samples
    inside: float        # share of the samples with a negative distance
    mean_inside: float   # mean over those (NaN without one)
    mean_outside: float  # mean over the others (NaN without one)


class SignedMeshDistance(NamedTuple):
    a_to_b: SignedDirected  # a's samples against b: negative = a lies inside b
    b_to_a: SignedDirected
    volume_a: float
    volume_b: float
    samples: int


def _topology_arrays(mesh) -> Tuple[Tensor, Tensor]:
    vertices, faces = mesh.vertices, mesh.faces
    if not (torch.is_tensor(vertices) and torch.is_tensor(faces)):
        raise ValueError("mesh_topology takes a Mesh of tensors")
    if vertices.device != faces.device:
        raise ValueError(f"vertices are on {vertices.device}, faces on {faces.device}")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.dtype.is_floating_point:
        raise ValueError("vertices must be a floating-point tensor of shape [V, 3]")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
        raise ValueError("faces must be an integer tensor of shape [T, 3]")
    return vertices.detach(), faces.detach().to(torch.int64).contiguous()


def mesh_topology(mesh: Mesh) -> MeshTopology:
    """Who lies across every edge of a mesh, and whether the mesh is a closed oriented surface.  Half-edge k of face f runs from
    corner k to corner k + 1; its undirected key is min V + max.  One stable sort of the 3 T keys puts the half-edges of an edge
    next to each other: an edge with exactly two half-edges that run in OPPOSITE directions makes its two faces partners; every other
    edge gets -1 (one face: a boundary), -2 (three or more: non-manifold) or -3 (two faces, same direction: inconsistently oriented)
    for all its half-edges.  Partners are symmetric.  torch only, on the mesh's device (a CPU mesh is fine); one host read.
    ValueError: other shapes or types, faces indexing outside the vertices, 2^31 / 3 faces or more."""
    vertices, faces = _topology_arrays(mesh)
    V, T, dev = int(vertices.shape[0]), int(faces.shape[0]), faces.device
    if T >= MAX_FACES:
        raise ValueError("mesh_topology takes fewer than 2^31 / 3 faces")
    if T == 0:
        return MeshTopology(torch.empty((0, 3), dtype=torch.int32, device=dev), 0, 0, 0, 0, False, 0.0)
    with torch.no_grad():
        start, end = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
        low, high = int(faces.min()), int(faces.max())  # (the host read the rest depends on)
        if low < 0 or high >= V:
            raise ValueError(f"faces index outside [0, {V})")
        keys = torch.minimum(start, end) * V + torch.maximum(start, end)
        forward = start < end
        keys, order = torch.sort(keys, stable=True)
        _, counts = torch.unique_consecutive(keys, return_counts=True)
        begins = torch.cumsum(counts, 0) - counts
        segment = torch.repeat_interleave(torch.arange(counts.shape[0], device=dev), counts)
        count = counts[segment]
        place = torch.arange(3 * T, device=dev) - begins[segment]
        mate = order[torch.where(count == 2, torch.arange(3 * T, device=dev) + 1 - 2 * place, torch.arange(3 * T, device=dev))]
        opposite = forward[order] != forward[mate]
        partner = torch.where(count == 1, PARTNER_BOUNDARY, torch.where(count > 2, PARTNER_NONMANIFOLD, torch.where(opposite, mate // 3, PARTNER_INCONSISTENT)))
        partners = torch.empty(3 * T, dtype=torch.int64, device=dev)
        partners[order] = partner
        corners = vertices.double()[faces]
        a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
        volume = (a * torch.linalg.cross(b, c)).sum(dim=1).sum() / 6.0
        flat = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0]) | ~(torch.linalg.cross(b - a, c - a).norm(dim=1) > 0)
        first = place == 0
        host = torch.stack([(first & (count == 1)).sum().double(), (first & (count > 2)).sum().double(), (first & (count == 2) & ~opposite).sum().double(),
                            flat.sum().double(), volume]).cpu().tolist()
    boundary, nonmanifold, inconsistent, degenerate = (int(v) for v in host[:4])
    return MeshTopology(partners.view(T, 3).to(torch.int32).contiguous(), boundary, nonmanifold, inconsistent, degenerate,
                        boundary == 0 and nonmanifold == 0 and inconsistent == 0, float(host[4]))


def face_pseudonormals_raw(vertices: Tensor, faces: Tensor, normals: Tensor, records: Tensor, status: Tensor) -> None:
    """Enqueue rf_mesh_face_pseudonormals (include/relu_field_ext.h): per face the unit normal into ``normals`` (float32 [T, 3]) and the
    angle-weighted corner records into ``records`` (float32 [T, 9]).  ``status`` (int32 [1], zeroed by the caller) becomes 1 for a vertex
    index outside the vertices.  One launch, no host synchronisation."""
    T = int(faces.shape[0])
    for t, dtype, shape, name in ((vertices, torch.float32, (int(vertices.shape[0]), 3), "vertices"), (faces, torch.int64, (T, 3), "faces"),
                                  (normals, torch.float32, (T, 3), "normals"), (records, torch.float32, (T, 9), "records"), (status, torch.int32, (1,), "status")):
        if not t.is_cuda or t.device != vertices.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {vertices.device}")
    rc = _lib.load().rf_mesh_face_pseudonormals(vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), T, 0, normals.data_ptr(), records.data_ptr(),
                                                status.data_ptr(), _marshal.stream(vertices.device))
    _lib.check(rc, "rf_mesh_face_pseudonormals")


def signed_distance_raw(vertices: Tensor, faces: Tensor, partners: Tensor, vertex_normals: Tensor, points: Tensor, face: Tensor, signed: Tensor, status: Tensor, *,
                        feature: Optional[Tensor] = None, normal: Optional[Tensor] = None) -> None:
    """Enqueue rf_mesh_signed_distance (include/relu_field_ext.h): per row of ``points`` (float32 [N, 3]) with closest face ``face`` (int64
    [N], -1: none) the signed distance into ``signed`` (float32 [N]), the feature into ``feature`` (int32 [N, 2]) and its pseudonormal
    into ``normal`` (float32 [N, 3]); the last two may be None.  ``status`` (int32 [1], zeroed by the caller) becomes 1 for a face id or a
    vertex index outside its array and 2 for a partner outside the faces; such a query writes nothing.  One launch, no host
    synchronisation."""
    n, T, V = int(points.shape[0]), int(faces.shape[0]), int(vertices.shape[0])
    for t, dtype, shape, name in ((vertices, torch.float32, (V, 3), "vertices"), (faces, torch.int64, (T, 3), "faces"), (partners, torch.int32, (T, 3), "partners"),
                                  (vertex_normals, torch.float32, (V, 3), "vertex_normals"), (points, torch.float32, (n, 3), "points"), (face, torch.int64, (n,), "face"),
                                  (signed, torch.float32, (n,), "signed"), (feature, torch.int32, (n, 2), "feature"), (normal, torch.float32, (n, 3), "normal"),
                                  (status, torch.int32, (1,), "status")):
        if t is None:
            continue
        if not t.is_cuda or t.device != points.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {points.device}")
    rc = _lib.load().rf_mesh_signed_distance(vertices.data_ptr(), V, faces.data_ptr(), T, partners.data_ptr(), vertex_normals.data_ptr(), points.data_ptr(),
                                             face.data_ptr(), n, 0, signed.data_ptr(), _marshal.ptr(feature), _marshal.ptr(normal), status.data_ptr(),
                                             _marshal.stream(points.device))
    _lib.check(rc, "rf_mesh_signed_distance")


def pseudonormal_tables(vertices: Tensor, faces: Tensor) -> Tuple[Tensor, Tensor]:
    """(normals float32 [T, 3], vertex_normals float32 [V, 3]) of a mesh on a HIP device: the unit face normals and, per vertex, the
    sum of angle x unit normal over the corners that name it -- rf_mesh_face_pseudonormals, then the gather launch of the mesh
    render's backward with every face as its own entry.  The sum order is fixed by the mesh: two calls give the same bits.
    One host read (the status word)."""
    T, V, dev = int(faces.shape[0]), int(vertices.shape[0]), vertices.device
    normals = torch.zeros((T, 3), dtype=torch.float32, device=dev)
    if not (T and V):
        return normals, torch.zeros((V, 3), dtype=torch.float32, device=dev)
    with torch.no_grad():
        records = torch.empty((T, 9), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        face_pseudonormals_raw(vertices, faces, normals, records, status)
        entries = torch.arange(T, dtype=torch.int32, device=dev)
        face_offsets = torch.arange(T + 1, dtype=torch.int64, device=dev)
        slots, vertex_offsets = corner_slot_lists(faces, V)
        vertex_normals = gather_vertex_gradients(records, entries, face_offsets, T, slots, vertex_offsets, V, 0, status)
        _marshal.require_faces_in_range(status, V)
    return normals, vertex_normals


class MeshSignGrid:
    """The signed search structure of one mesh, built once: a ``MeshDistanceGrid`` (``grid``), the ``mesh_topology`` (``topology``) and
    the two normal tables (``normals`` [T, 3], ``vertex_normals`` [V, 3]).  The distance is negative INSIDE.  ``orientation``:
    "outward" -- the face normals (v1 - v0) x (v2 - v0) point out of the solid, as ``extract_mesh`` winds its faces; "inward" flips the
    sign; "auto" takes the orientation from the sign of ``topology.signed_volume``.  The sign is guaranteed for a closed, consistently
    oriented, edge-manifold mesh only; any other mesh still gets an answer, computed with a one-sided normal at its open edges, but
    that sign is NOT guaranteed and a warning says so once per grid.  ``cell_size`` is ``MeshDistanceGrid``'s and changes the speed only:
    every result is identical bits for every cell size.
    ValueError: as ``MeshDistanceGrid``; 2^31 / 3 faces or more; an unknown ``orientation``."""

    def __init__(self, mesh: Mesh, cell_size: Optional[float] = None, orientation: str = "outward"):
        if orientation not in ORIENTATIONS:
            raise ValueError(f"orientation must be one of {ORIENTATIONS}, got {orientation!r}")
        self.grid = MeshDistanceGrid(mesh, cell_size)
        self.vertices, self.faces, self.device = self.grid.vertices, self.grid.faces, self.grid.device
        if self.faces.shape[0] >= MAX_FACES:
            raise ValueError("MeshSignGrid takes fewer than 2^31 / 3 faces")
        self.topology = mesh_topology(Mesh(self.vertices, self.faces, None, None))
        self.normals, self.vertex_normals = pseudonormal_tables(self.vertices, self.faces)
        self.orientation = orientation
        self.flip = orientation == "inward" or (orientation == "auto" and self.topology.signed_volume < 0.0)
        if not self.topology.closed and self.faces.shape[0]:
            t = self.topology
            warnings.warn(f"MeshSignGrid: the mesh is not a closed oriented surface ({t.boundary_edges} boundary, {t.nonmanifold_edges} non-manifold, "
                          f"{t.inconsistent_edges} inconsistently oriented edges): the sign of the distance is not guaranteed", RuntimeWarning, stacklevel=2)

    def _sign(self, points: Tensor, face: Tensor, return_features: bool):
        """(signed, feature, normal) for queries whose closest faces are ``face``; one host read (the status word)"""
        N, dev = int(points.shape[0]), self.device
        signed = torch.full((N,), math.inf, dtype=torch.float32, device=dev)
        feature = torch.full((N, 2), FEATURE_NONE, dtype=torch.int32, device=dev) if return_features else None
        normal = torch.zeros((N, 3), dtype=torch.float32, device=dev) if return_features else None
        if N and self.faces.shape[0]:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            signed_distance_raw(self.vertices, self.faces, self.topology.partners, self.vertex_normals, points, face, signed, status, feature=feature, normal=normal)
            if int(status.item()):
                raise ValueError("MeshSignGrid: a face id, a vertex index or a partner lies outside its array")
            if self.flip:
                signed = torch.where(torch.isfinite(signed) & (signed != 0), -signed, signed)
        return signed, feature, normal

    def signed_distance(self, points: Tensor, max_distance: Optional[float] = None, return_features: bool = False) -> SignedClosestPoints:
        """SignedClosestPoints of ``points`` (float32 [N, 3] on the mesh's device): ``face`` and ``point`` are those of
        ``MeshDistanceGrid.closest(points, max_distance)`` and ``abs(distance)`` is its distance, bit for bit; the sign is negative
        inside.  A query on the surface gets +0; one without a face within ``max_distance`` keeps +inf.  ``return_features`` adds the
        feature that holds the closest point and the pseudonormal used.  Two host reads (the two status words)."""
        found = self.grid.closest(points, max_distance)
        with torch.no_grad():
            signed, feature, normal = self._sign(points.detach().contiguous(), found.face, return_features)
        return SignedClosestPoints(signed, found.face, found.point, feature, normal)

    def contains(self, points: Tensor) -> Tensor:
        """bool [N]: ``signed_distance(points).distance < 0``"""
        return self.signed_distance(points).distance < 0


def mesh_signed_distance(points: Tensor, mesh: Mesh, *, max_distance: Optional[float] = None, cell_size: Optional[float] = None, orientation: str = "outward",
                         return_features: bool = False) -> SignedClosestPoints:
    """``MeshSignGrid(mesh, cell_size, orientation).signed_distance(points, max_distance, return_features)`` in one call"""
    return MeshSignGrid(mesh, cell_size, orientation).signed_distance(points, max_distance, return_features)


def mesh_contains(points: Tensor, mesh: Mesh, *, cell_size: Optional[float] = None, orientation: str = "outward") -> Tensor:
    """bool [N]: which rows of ``points`` lie inside the closed mesh"""
    return MeshSignGrid(mesh, cell_size, orientation).contains(points)


def point_mesh_signed_distance(points: Tensor, vertices: Tensor, faces: Tensor, *, max_distance: Optional[float] = None, cell_size: Optional[float] = None,
                               orientation: str = "outward") -> Tensor:
    """float32 [N]: the signed distance of every row of ``points`` to the closed mesh (``vertices`` float32 [V, 3], ``faces`` integer [T, 3],
    all on one HIP device), differentiable with respect to ``points`` and ``vertices``: the detached sign of ``MeshSignGrid`` times
    ``point_mesh_distance``.  Away from the surface the sign is locally constant, so the gradients are those of
    ``point_mesh_distance`` times +-1, bit for bit; there is no backward kernel of its own.  The value has the bits of
    ``MeshSignGrid.signed_distance``."""
    _check_vertices(vertices, "point_mesh_signed_distance")
    if not torch.is_tensor(points) or not points.is_cuda:
        raise ValueError("point_mesh_signed_distance takes points on a HIP device; there is no CPU path")
    signs = MeshSignGrid(Mesh(vertices.detach(), faces, None, None), cell_size, orientation)
    distance, found = _distance(points, vertices, signs.grid, max_distance)
    with torch.no_grad():
        signed, _, _ = signs._sign(points.detach().contiguous(), found.face, False)
        sign = torch.where(signed < 0, -1.0, 1.0).to(torch.float32)
    return sign * distance


class MeshSDF(NamedTuple):
    sdf: Tensor        # [X, Y, Z] float32: signed distance of every node, negative inside; +-truncation where it is not known
    known: Tensor      # [X, Y, Z] bool: the node's distance is the exact one (everywhere without a truncation)
    aabb: tuple        # ((3 floats), (3 floats)): the box of the lattice (float32 values)
    truncation: Optional[float]

    def to_voxel_grid(self, storage: str = "reference", offset: float = 0.0) -> VoxelGrid:
        """The volume as a VoxelGrid with Identity/Identity density callables (mode "identity"): ``densities = offset - sdf`` (positive
        inside the surface ``offset`` away from the mesh's), 3 zero SH-degree-0 features (mid grey), voxel size and location such that
        the grid's nodes are these nodes -- as ``FusedVolume.to_voxel_grid`` does."""
        dims = tuple(int(v) for v in self.sdf.shape)
        lo, hi = self.aabb
        size = VoxelSize(*[(b - a) / n for a, b, n in zip(lo, hi, dims)])
        location = VoxelGridLocation(*[(b + a) / 2 for a, b in zip(lo, hi)])
        features = torch.zeros(dims + (3,), dtype=torch.float32, device=self.sdf.device)
        density = -self.sdf if offset == 0.0 else float(offset) - self.sdf
        grid = VoxelGrid(density[..., None].contiguous(), features, size, location, density_preactivation=torch.nn.Identity(),
                         density_postactivation=torch.nn.Identity(), expected_density_scale=1.0, storage=storage)
        for (a, b), mine_lo, mine_hi in zip(grid.aabb, lo, hi):
            if float(np.float32(a)) != mine_lo or float(np.float32(b)) != mine_hi:
                raise ValueError(f"the box [{mine_lo}, {mine_hi}] is not reproduced by a voxel size and a location ([{a}, {b}])")
        return grid

    def extract_mesh(self, offset: float = 0.0, subdivisions: int = 1) -> Mesh:
        """The remeshed surface, or the surface ``offset`` away from it (positive: outward): the level set ``sdf = offset``, closed and
        wound outward.  It is ``extract_mesh(self.to_voxel_grid(offset=offset), 0.0, subdivisions)``, the level ``-offset`` of
        ``to_voxel_grid()`` with the shift put into the field: ``extract_mesh`` takes the field to be 0 outside the box, which a level
        below 0 would count as inside.  With a truncation, ``abs(offset)`` must stay below it."""
        offset = float(offset)
        if not math.isfinite(offset) or (self.truncation is not None and abs(offset) >= self.truncation):
            raise ValueError(f"offset must be finite and smaller than the truncation, got {offset!r}")
        return extract_mesh(self.to_voxel_grid(offset=offset), 0.0, subdivisions)


def node_coordinates(lo: float, hi: float, dim: int, device) -> Tensor:
    """float32 [dim]: where a VoxelGrid -- and ``fuse_depth_views`` -- puts its nodes on one axis: lo + (hi - lo) ((2 i + 1) / (2 dim)),
    every operation in float32"""
    ext = np.float32(hi) - np.float32(lo)
    i = torch.arange(dim, dtype=torch.int64, device=device)
    frac = (2 * i + 1).to(torch.float32) / torch.full((), float(2 * dim), dtype=torch.float32, device=device)
    return torch.full((), float(np.float32(lo)), dtype=torch.float32, device=device) + torch.full((), float(ext), dtype=torch.float32, device=device) * frac


def _fill_along(sign: Tensor, axis: int) -> Tensor:
    """every unknown node (0) takes the sign of the nearest known node before it on its line along ``axis`` (no change without one)"""
    n = sign.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n
    index = torch.arange(n, device=sign.device).view(shape).expand_as(sign)
    last = torch.cummax(torch.where(sign != 0, index, -1), dim=axis).values
    filled = torch.gather(sign, axis, last.clamp(min=0))
    return torch.where(last >= 0, filled, sign)


def propagate_signs(sign: Tensor) -> Tensor:
    """int8 [X, Y, Z] of -1 / 0 / +1 -> the same with every 0 replaced by the sign of a known node that a path of 6-neighbour steps
    through unknown nodes reaches: scans along z, y and x in both directions, repeated until no 0 is left.  A volume without a known
    node is returned as it is."""
    while True:
        unknown = int((sign == 0).sum())
        if unknown == 0 or unknown == sign.numel():
            return sign
        for axis in (2, 1, 0):
            sign = _fill_along(sign, axis)
            sign = _fill_along(sign.flip(axis), axis).flip(axis)


def mesh_to_sdf(mesh: Mesh, aabb_min, aabb_max, grid_dims, *, truncation: Optional[float] = None, cell_size: Optional[float] = None,
                orientation: str = "outward") -> MeshSDF:
    """Sample the signed distance to a closed mesh on the ``grid_dims`` nodes of the box [``aabb_min``, ``aabb_max``], the nodes placed as
    a VoxelGrid's and as ``fuse_depth_views``' are.  The nodes are queried slab by slab along x (about 2^20 nodes per call), so no
    [X Y Z, 3] tensor of points ever exists.  ``truncation=None``: every node gets its exact distance.  With a ``truncation`` (more than
    1.5 x the longest voxel edge) the queries stop at that distance; a node without a face within it is unknown and gets
    +-``truncation``, its sign propagated from known nodes to 6-neighbours (``propagate_signs``).  That is exact: two adjacent nodes of
    opposite sign have the surface between them on the lattice edge that joins them, so both lie within one voxel edge of it and both
    are known; an unknown node therefore has the sign of every neighbour, known or not.  A volume without any known node takes the
    sign of one unlimited query.  Known values are the bits of the exact call.
    ValueError: as ``MeshSignGrid`` and ``fuse_depth_views`` for the box and the dims; a truncation that is too small."""
    dims = _grid_dims(grid_dims)
    lo, hi = _float32_triple(aabb_min, "aabb_min"), _float32_triple(aabb_max, "aabb_max")
    if not all(b > a and math.isfinite(float(np.float32(b) - np.float32(a))) for a, b in zip(lo, hi)):
        raise ValueError(f"the box must have aabb_max > aabb_min on every axis, got {lo} .. {hi}")
    edge = max((b - a) / n for a, b, n in zip(lo, hi, dims))
    if truncation is not None:
        truncation = float(np.float32(truncation))
        if not (math.isfinite(truncation) and truncation > MIN_TRUNCATION_VOXELS * edge):
            raise ValueError(f"truncation must be finite and exceed {MIN_TRUNCATION_VOXELS} x the longest voxel edge ({edge!r}), got {truncation!r}")
    signs = MeshSignGrid(mesh, cell_size, orientation)
    dev = signs.device
    X, Y, Z = dims
    with torch.no_grad():
        cx, cy, cz = (node_coordinates(lo[a], hi[a], dims[a], dev) for a in range(3))
        sdf = torch.empty(dims, dtype=torch.float32, device=dev)
        step = max(1, SLAB_POINTS // (Y * Z))
        for first in range(0, X, step):
            last = min(first + step, X)
            gx, gy, gz = torch.meshgrid(cx[first:last], cy, cz, indexing="ij")
            points = torch.stack([gx, gy, gz], dim=-1).view(-1, 3).contiguous()
            sdf[first:last] = signs.signed_distance(points, truncation).distance.view(last - first, Y, Z)
        known = torch.isfinite(sdf)
        if truncation is not None:
            sign = torch.where(known, torch.where(sdf < 0, -1, 1), 0).to(torch.int8)
            if not bool(known.any()):
                corner = torch.stack([cx[0], cy[0], cz[0]]).view(1, 3).contiguous()
                sign.fill_(-1 if bool(signs.signed_distance(corner).distance[0] < 0) else 1)
            sign = propagate_signs(sign)
            sdf = torch.where(known, sdf, sign.to(torch.float32) * truncation)
    return MeshSDF(sdf, known, (lo, hi), truncation)


def _signed_directed(d: Tensor):
    d = d.double()
    inside = d < 0
    n_in, n_out = inside.sum(), (~inside).sum()
    nan = torch.full((), math.nan, dtype=torch.float64, device=d.device)
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    return [d.mean(), inside.double().mean(), torch.where(n_in > 0, torch.where(inside, d, zero).sum() / n_in.clamp(min=1), nan),
            torch.where(n_out > 0, torch.where(inside, zero, d).sum() / n_out.clamp(min=1), nan)]


def signed_mesh_distance(mesh_a: Mesh, mesh_b: Mesh, *, samples: int = 1_000_000, seed: int = 0, orientation: str = "outward") -> SignedMeshDistance:
    """Which way two closed surfaces lie from each other: the surface samples of ``mesh_distance`` under the same ``seed``
    (``sample_mesh_surface`` with ``seed`` for a and ``seed + 1`` for b), each with its SIGNED distance to the other mesh.  Per direction:
    the signed mean, the share of samples inside the other mesh, and the mean over the inside and over the outside samples (NaN
    without one); and both signed volumes.  ``a_to_b.mean < 0`` says a lies, on average, inside b.  Reductions are float64 torch ops on
    the device; one host read for them.  ValueError: as ``MeshSignGrid`` and ``sample_mesh_surface``; samples < 1."""
    samples = _count(samples, "samples")
    if samples < 1:
        raise ValueError("samples must be at least 1")
    sign_a, sign_b = MeshSignGrid(mesh_a, None, orientation), MeshSignGrid(mesh_b, None, orientation)
    points_a = sample_mesh_surface(mesh_a, samples, seed=seed)[0]
    points_b = sample_mesh_surface(mesh_b, samples, seed=int(seed) + 1)[0]
    with torch.no_grad():
        host = torch.stack(_signed_directed(sign_b.signed_distance(points_a).distance) + _signed_directed(sign_a.signed_distance(points_b).distance)).cpu().tolist()
    return SignedMeshDistance(SignedDirected(*host[0:4]), SignedDirected(*host[4:8]), sign_a.topology.signed_volume, sign_b.topology.signed_volume, samples)


def signed_mean_against(mesh: Mesh, reference: Mesh, *, samples: int = 1_000_000, seed: int = 0) -> Optional[SignedDirected]:
    """The SignedDirected of ``samples`` surface samples of ``mesh`` (``sample_mesh_surface`` with ``seed``: the samples ``mesh_distance`` takes
    of its first mesh) against ``reference`` -- or None when ``reference`` is not a closed oriented surface, whose sign would not be
    guaranteed.  What the scripts print beside the unsigned distance: negative = ``mesh`` lies inside ``reference``."""
    if not mesh_topology(reference).closed:
        return None
    points = sample_mesh_surface(mesh, _count(samples, "samples"), seed=seed)[0]
    with torch.no_grad():
        return SignedDirected(*torch.stack(_signed_directed(MeshSignGrid(reference).signed_distance(points).distance)).cpu().tolist())


def format_signed_mean(d: SignedDirected, a: str = "output", b: str = "input") -> str:
    """the line the scripts print for ``signed_mean_against``"""
    return f"  {a} -> {b}: signed mean {d.mean:.6g} (negative: inside)  inside {d.inside:.4f}  mean inside {d.mean_inside:.6g}  mean outside {d.mean_outside:.6g}"


def format_signed_mesh_distance(result: SignedMeshDistance, a: str = "a", b: str = "b") -> str:
    """the lines the scripts print"""
    row = lambda name, d: f"  {name}: signed mean {d.mean:.6g}  inside {d.inside:.4f}  mean inside {d.mean_inside:.6g}  mean outside {d.mean_outside:.6g}"  # noqa: E731
    return "\n".join([f"signed surface distance from {result.samples} samples per mesh (negative: inside the other mesh):", row(f"{a} -> {b}", result.a_to_b),
                      row(f"{b} -> {a}", result.b_to_a), f"  signed volume {a} {result.volume_a:.6g}  {b} {result.volume_b:.6g}"])


def signed_mesh_distance_dict(result: SignedMeshDistance) -> dict:
    """``result`` as plain JSON-serialisable data"""
    return {"samples": result.samples, "a_to_b": result.a_to_b._asdict(), "b_to_a": result.b_to_a._asdict(), "volume_a": result.volume_a, "volume_b": result.volume_b}
