"""How far one surface lies from another: the closest point on a triangle mesh for millions of query points, area-weighted surface
samples, and the Chamfer distance, the Hausdorff distance and the F-score of two meshes built on them.  A uniform lattice of cubic
cells over the mesh's box lists, per cell, the faces whose boxes overlap it (one HIP launch, rf_mesh_grid_pairs, between a torch
prefix sum and a torch sort); rf_mesh_closest_points then walks the shells of cells around every query until the best distance is
proven minimal (csrc/mesh_distance_kernels.hip).  The minimum is order-independent, ties go to the lowest face index and every
face goes through one float32 rule, so the result does not depend on the lattice at all: any ``cell_size`` -- a single cell, the
brute force, included -- gives the same bits.  docs/mesh_distance_errors.md has the rule, the error bound and the proof of the stop
test, tests/mesh_distance_model.py the numpy model, DESIGN.md section 27 the measurements.

Gradients of the distance, the Chamfer loss and the fit built on them live in thr3ed_atom_amd/mesh_distance_grad.py, the signed
distance and inside / outside in thr3ed_atom_amd/mesh_sign.py.

Not done here: a BVH for meshes whose face sizes vary by orders of magnitude (one lattice
serves all faces), point-cloud-to-point-cloud distance."""
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal, ops
from .mesh import Mesh
from .mesh_simplify import _host_bounds

MAX_PAIRS_PER_FACE, MAX_PAIRS_SLACK = 16, 1 << 20  # the default cell size doubles until pairs <= 16 faces + 2^20
_LADDER = 8                                        # cell sizes whose pair counts one host read fetches


class ClosestPoints(NamedTuple):
    distance: Tensor  # float32 [N]; +inf when nothing lies within max_distance
    face: Tensor      # int64 [N]; -1 then
    point: Tensor     # float32 [N, 3]; NaN then


class DirectedDistance(NamedTuple):
    mean: float
    rms: float
    max: float        # over the samples AND the source mesh's vertices
    median: float
    q90: float
    q99: float


class ThresholdScore(NamedTuple):
    threshold: float
    precision: float  # share of a's samples within the threshold of b
    recall: float     # share of b's samples within the threshold of a
    fscore: float


class MeshDistance(NamedTuple):
    a_to_b: DirectedDistance
    b_to_a: DirectedDistance
    chamfer_l1: float
    chamfer_l2: float
    hausdorff: float
    thresholds: Tuple[ThresholdScore, ...]
    samples: int


class _Lattice(NamedTuple):
    origin: np.ndarray  # float32 [3]
    h: np.float32
    r: np.float32
    cells: np.ndarray   # int64 [3]


def _lattice(bounds: np.ndarray, h) -> Optional[_Lattice]:
    """the host side of the cell contract (that of ``mesh_simplify._lattice``): r = fl32(1 / h), origin = the minimum,
    n_a = floor(fl32(fl32(max_a - min_a) r)) + 1; None when the lattice is over the limits"""
    h = np.float32(h)
    with np.errstate(all="ignore"):
        r = np.float32(1.0) / h
        if not (np.isfinite(h) and h > 0 and np.isfinite(r) and r > 0):
            raise ValueError(f"cell_size must be a positive finite float32 value with a float32 reciprocal, got {float(h)!r}")
        top = np.floor(((bounds[1] - bounds[0]).astype(np.float32) * r).astype(np.float32))
    if not np.isfinite(top).all() or (top + 1 > _lib.MESH_DISTANCE_MAX_CELLS).any():
        return None
    cells = top.astype(np.int64) + 1
    if int(cells.prod()) + 1 > _lib.MESH_DISTANCE_MAX_TABLE:
        return None
    return _Lattice(bounds[0].copy(), h, r, cells)


def _cells_of(values: Tensor, lattice: _Lattice) -> Tensor:
    """int64 [..., 3]: the clamped cell of every float32 coordinate triple, the kernel's dist_cell in torch (separate float32 ops)"""
    dev = values.device
    origin = torch.from_numpy(lattice.origin).to(dev)
    r = torch.full((), float(lattice.r), dtype=torch.float32, device=dev)
    top = torch.from_numpy((lattice.cells - 1).astype(np.float32)).to(dev)
    t = torch.floor((values - origin) * r)
    return torch.minimum(torch.clamp_min(t, 0.0), top).to(torch.int64)


def _face_cell_counts(corners_low: Tensor, corners_high: Tensor, lattice: _Lattice) -> Tensor:
    return (_cells_of(corners_high, lattice) - _cells_of(corners_low, lattice) + 1).prod(dim=1)


def default_cell_size(mean_area: float, extent: float) -> np.float32:
    """twice the leg of the right isosceles triangle of the mean face area; the largest extent (or 1) for a mesh without area"""
    h = np.float32(2.0 * math.sqrt(2.0 * mean_area)) if math.isfinite(mean_area) and mean_area > 0 else np.float32(0.0)
    if not (np.isfinite(h) and h > 0):
        h = np.float32(extent)
    if not (np.isfinite(h) and h > 0):
        h = np.float32(1.0)
    return h


class MeshDistanceGrid:
    """The search structure of one mesh, built once: ``closest(points)`` answers any number of query batches.  ``cell_size=None`` picks
    h = fl32(2 sqrt(2 mean face area)) and doubles it until the lattice has at most 1024 cells per axis and fewer than 2^25 cells and
    the faces are registered in at most 16 T + 2^20 cells altogether; an explicit ``cell_size`` is used as given (ValueError when the
    lattice is over the first two limits).  The choice changes the speed only: results are identical bits for every cell size.
    Two host reads (bounds and areas; the pair counts).  ValueError: a CPU mesh, faces indexing outside the vertices, non-finite
    vertices, 2^31 faces or more, ``cell_size`` <= 0."""

    def __init__(self, mesh: Mesh, cell_size: Optional[float] = None):
        if cell_size is not None and not (isinstance(cell_size, (int, float, np.floating, np.integer)) and math.isfinite(float(cell_size)) and float(cell_size) > 0):
            raise ValueError(f"cell_size must be positive and finite, got {cell_size!r}")
        vertices, faces = _marshal.mesh_arrays(mesh, "MeshDistanceGrid")
        if vertices.shape[0] >= 2**31 or faces.shape[0] >= 2**31:
            raise ValueError("MeshDistanceGrid takes fewer than 2^31 vertices and faces")
        self.vertices, self.faces, self.device = vertices, faces, vertices.device
        self.lattice: Optional[_Lattice] = None
        self.pairs = 0
        T = faces.shape[0]
        if T == 0:
            return
        with torch.no_grad():
            bounds = _host_bounds(Mesh(vertices, faces, None, None))  # (raises on bad indices and non-finite vertices)
            corners = vertices[faces]
            low, high = corners.amin(dim=1), corners.amax(dim=1)
            budget = MAX_PAIRS_PER_FACE * T + MAX_PAIRS_SLACK
            if cell_size is not None:
                lattice = _lattice(bounds, cell_size)
                if lattice is None:
                    raise ValueError(f"cell_size {float(cell_size)!r} gives more than {_lib.MESH_DISTANCE_MAX_CELLS} cells along an axis or {_lib.MESH_DISTANCE_MAX_TABLE} cells in all")
                counts = _face_cell_counts(low, high, lattice)
            else:
                c64 = corners.double()
                area = 0.5 * torch.linalg.cross(c64[:, 1] - c64[:, 0], c64[:, 2] - c64[:, 0]).norm(dim=1).sum()
                h = default_cell_size(float(area.item()) / T, float((bounds[1] - bounds[0]).astype(np.float32).max()))
                while _lattice(bounds, h) is None:
                    h = np.float32(h * np.float32(2.0))
                lattice = counts = None
                while lattice is None:
                    ladder = [_lattice(bounds, np.float32(h * np.float32(2.0 ** k))) for k in range(_LADDER)]
                    ladder_counts = [_face_cell_counts(low, high, g) for g in ladder]
                    totals = torch.stack([c.sum() for c in ladder_counts]).cpu().tolist()
                    for g, c, total in zip(ladder, ladder_counts, totals):
                        if total <= budget:
                            lattice, counts = g, c
                            break
                    h = np.float32(h * np.float32(2.0 ** _LADDER))
            offsets = torch.zeros(T + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(counts, dim=0, out=offsets[1:])
            pairs = int(offsets[-1].item())
            if pairs >= 2**31:
                raise ValueError(f"cell_size {float(lattice.h)!r} registers the faces in {pairs} cells; the lists take fewer than 2^31")
            keys = torch.empty(pairs, dtype=torch.int64, device=self.device)
            pair_faces = torch.empty(pairs, dtype=torch.int32, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            ops.mesh_grid_pairs_raw(vertices, faces, lattice.origin, lattice.h, lattice.cells, offsets, keys, pair_faces, status)
            if int(status.item()):  # (before the keys are used: a face that wrote nothing left its pairs unset)
                raise RuntimeError("rf_mesh_grid_pairs disagrees with the cell counts of the binding (status %d)" % int(status.item()))
            order = torch.sort(keys, stable=True).indices
            self.cell_faces = pair_faces[order].contiguous()
            self.cell_begin = _marshal.segment_offsets(keys, int(lattice.cells.prod())).to(torch.int32).contiguous()
            self.lattice, self.pairs = lattice, pairs

    @property
    def cell_size(self) -> float:
        return float(self.lattice.h) if self.lattice is not None else 0.0

    def closest(self, points: Tensor, max_distance: Optional[float] = None, *, return_rings: bool = False):
        """ClosestPoints of ``points`` (float32 [N, 3] on the mesh's device): per query the float32 distance to the mesh, the closest
        face (the lowest index among exact ties) and the closest point on it.  With ``max_distance`` (inclusive) a query with no face
        within it gets (+inf, -1, NaN); the others get the bits of the unlimited call.  One host read (the status word).
        ValueError: points of another shape, type or device, non-finite points, a negative or NaN ``max_distance``."""
        if not torch.is_tensor(points) or not points.is_cuda or points.device != self.device:
            raise ValueError(f"points must be a tensor on the mesh's HIP device {self.device}; there is no CPU path")
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise ValueError("points must be a float32 tensor of shape [N, 3]")
        limit = math.inf if max_distance is None else float(max_distance)
        if not limit >= 0.0:
            raise ValueError(f"max_distance must be non-negative, got {max_distance!r}")
        points = points.detach().contiguous()
        N = points.shape[0]
        distance = torch.full((N,), math.inf, dtype=torch.float32, device=self.device)
        face = torch.full((N,), -1, dtype=torch.int64, device=self.device)
        point = torch.full((N, 3), math.nan, dtype=torch.float32, device=self.device)
        rings = torch.zeros(N, dtype=torch.int32, device=self.device) if return_rings else None
        if N and self.lattice is None and not bool(torch.isfinite(points).all()):
            raise ValueError("points are not finite")
        if N and self.lattice is not None:
            with torch.no_grad():
                g = self.lattice
                cell = _cells_of(points, g)  # (NaN lands anywhere in the order; the kernel reports it)
                order = torch.sort((cell[:, 0] * int(g.cells[1]) + cell[:, 1]) * int(g.cells[2]) + cell[:, 2]).indices
                status = torch.zeros(1, dtype=torch.int32, device=self.device)
                ops.mesh_closest_points_raw(self.vertices, self.faces, g.origin, g.h, g.cells, self.cell_begin, self.cell_faces, points, order, limit,
                                            distance, face, point, rings, status)
                code = int(status.item())
            if code == 1:
                raise ValueError("points are not finite (or a face indexes outside the vertices)")
            if code:
                raise RuntimeError("rf_mesh_closest_points met a list entry outside its array")
        out = ClosestPoints(distance, face, point)
        return (out, rings) if return_rings else out


def closest_points_on_mesh(points: Tensor, mesh: Mesh, *, max_distance: Optional[float] = None, cell_size: Optional[float] = None) -> ClosestPoints:
    """``MeshDistanceGrid(mesh, cell_size).closest(points, max_distance)`` in one call"""
    return MeshDistanceGrid(mesh, cell_size).closest(points, max_distance)


def _count(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    return int(value)


def sample_mesh_surface(mesh: Mesh, count: int, *, seed: int = 0):
    """``count`` points on the surface of a mesh on a HIP device, area-weighted and stratified: the float64 prefix sum of the face areas
    (in face order) of total A is cut into ``count`` strata of length A / count, stratum i draws the position (i + u_i) A / count with
    u_i uniform in [0, 1), and the face is the first whose prefix sum exceeds it (``searchsorted``) -- so a face of area a gets within
    one of count a / A samples and a face without area gets none.  Within the face the barycentrics are (1 - sqrt(r1),
    sqrt(r1) (1 - r2), sqrt(r1) r2), uniform over the triangle.  Returns (points float32 [count, 3], faces int64 [count], barycentrics
    float32 [count, 3]).  torch only; the same seed on the same device gives the same bits.  ValueError: a CPU mesh, bad faces,
    non-finite vertices, count > 0 on a mesh without area."""
    count = _count(count, "count")
    vertices, faces = _marshal.mesh_arrays(mesh, "sample_mesh_surface")
    dev = vertices.device
    if count == 0:
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev))
    if faces.shape[0] == 0:
        raise ValueError("sample_mesh_surface needs a mesh with a positive area")
    with torch.no_grad():
        _host_bounds(Mesh(vertices, faces, None, None))
        corners = vertices[faces].double()
        area = 0.5 * torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]).norm(dim=1)
        prefix = torch.cumsum(area, dim=0)
        total = prefix[-1]
        generator = torch.Generator(device=dev)
        generator.manual_seed(int(seed))
        u = torch.rand((count, 3), dtype=torch.float64, device=dev, generator=generator)
        position = (torch.arange(count, dtype=torch.float64, device=dev) + u[:, 0]) * total / count
        last = torch.nonzero(area > 0).max() if bool((total > 0) & torch.isfinite(total)) else None  # (the host read)
        if last is None:
            raise ValueError("sample_mesh_surface needs a mesh with a positive area")
        picked = torch.minimum(torch.searchsorted(prefix, position, right=True), last)
        s = torch.sqrt(u[:, 1])
        bary = torch.stack([1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]], dim=1)
        points = (bary[:, :, None] * corners[picked]).sum(dim=1)
    return points.float(), picked, bary.float()


def _directed(samples: Tensor, vertices: Tensor):
    """(mean, rms, max, q50, q90, q99, mean of squares) of one direction as float64 device scalars: linear-interpolated quantiles of the
    sorted sample distances, the maximum over samples and vertices"""
    d = torch.sort(samples.double()).values
    n = d.numel()
    squares = (d * d).mean()
    quantiles = []
    for q in (0.5, 0.9, 0.99):
        at = q * (n - 1)
        lo = int(math.floor(at))
        hi = min(lo + 1, n - 1)
        quantiles.append(d[lo] + (d[hi] - d[lo]) * (at - lo))
    return [d.mean(), torch.sqrt(squares), torch.maximum(d[-1], vertices.double().max()) if vertices.numel() else d[-1], *quantiles, squares]


def mesh_distance(mesh_a: Mesh, mesh_b: Mesh, *, samples: int = 1_000_000, thresholds: Sequence[float] = (), seed: int = 0) -> MeshDistance:
    """The distance between two surfaces on a HIP device from ``samples`` area-weighted points of each (``sample_mesh_surface`` with
    ``seed`` for a and ``seed + 1`` for b) and their closest points on the other mesh.  Per direction: mean, rms, max and the 50 / 90 /
    99 % quantiles of the sample distances; ``chamfer_l1`` = half the sum of the two means, ``chamfer_l2`` the same over squared
    distances; per threshold t, ``precision`` = the share of a's samples with d <= t, ``recall`` that of b's, ``fscore`` their harmonic
    mean (0 when both are 0).  ``hausdorff`` is the larger of the two maxima, each taken over the samples and the source mesh's
    vertices: the supremum over a finite set of points of the surface, hence a LOWER bound of the true Hausdorff distance, which more
    samples can only raise.  Reductions are float64 torch ops on the device.  ValueError: as ``MeshDistanceGrid`` and
    ``sample_mesh_surface``; samples < 1; a negative or NaN threshold."""
    samples = _count(samples, "samples")
    if samples < 1:
        raise ValueError("samples must be at least 1")
    thresholds = [float(t) for t in thresholds]
    if not all(t >= 0.0 for t in thresholds):
        raise ValueError(f"thresholds must be non-negative, got {thresholds!r}")
    grid_a, grid_b = MeshDistanceGrid(mesh_a), MeshDistanceGrid(mesh_b)
    points_a = sample_mesh_surface(mesh_a, samples, seed=seed)[0]
    points_b = sample_mesh_surface(mesh_b, samples, seed=int(seed) + 1)[0]
    with torch.no_grad():
        d_ab, d_ba = grid_b.closest(points_a).distance, grid_a.closest(points_b).distance
        v_ab, v_ba = grid_b.closest(grid_a.vertices).distance, grid_a.closest(grid_b.vertices).distance
        scalars = _directed(d_ab, v_ab) + _directed(d_ba, v_ba)
        for t in thresholds:
            scalars += [(d_ab <= t).double().mean(), (d_ba <= t).double().mean()]
        host = torch.stack(scalars).cpu().tolist()  # (the one host read of the reductions)
    a_to_b, b_to_a = DirectedDistance(*host[0:6]), DirectedDistance(*host[7:13])
    scores = []
    for k, t in enumerate(thresholds):
        precision, recall = host[14 + 2 * k], host[15 + 2 * k]
        scores.append(ThresholdScore(t, precision, recall, 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0))
    return MeshDistance(a_to_b, b_to_a, 0.5 * (a_to_b.mean + b_to_a.mean), 0.5 * (host[6] + host[13]), max(a_to_b.max, b_to_a.max), tuple(scores), samples)


def format_mesh_distance(result: MeshDistance, a: str = "a", b: str = "b") -> str:
    """the lines the scripts print"""
    row = lambda name, d: f"  {name}: mean {d.mean:.6g}  rms {d.rms:.6g}  median {d.median:.6g}  90% {d.q90:.6g}  99% {d.q99:.6g}  max {d.max:.6g}"  # noqa: E731
    lines = [f"surface distance from {result.samples} samples per mesh:", row(f"{a} -> {b}", result.a_to_b), row(f"{b} -> {a}", result.b_to_a),
             f"  chamfer L1 {result.chamfer_l1:.6g}  chamfer L2 {result.chamfer_l2:.6g}  hausdorff (lower bound) {result.hausdorff:.6g}"]
    lines += [f"  threshold {s.threshold:.6g}: precision {s.precision:.4f}  recall {s.recall:.4f}  F-score {s.fscore:.4f}" for s in result.thresholds]
    return "\n".join(lines)


def mesh_distance_dict(result: MeshDistance) -> dict:
    """``result`` as plain JSON-serialisable data"""
    return {"samples": result.samples, "a_to_b": result.a_to_b._asdict(), "b_to_a": result.b_to_a._asdict(), "chamfer_l1": result.chamfer_l1,
            "chamfer_l2": result.chamfer_l2, "hausdorff": result.hausdorff, "thresholds": [s._asdict() for s in result.thresholds]}
