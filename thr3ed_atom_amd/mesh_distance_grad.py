"""Gradients of the distance between surfaces, and the fit built on them: ``point_mesh_distance`` is ``MeshDistanceGrid.closest`` as a
differentiable function of the queries and of the mesh's vertices, ``mesh_surface_points`` the surface sampler's points as a
differentiable function of the vertices, ``MeshChamferLoss`` half the sum of the two directed mean distances between a moving and a
fixed mesh, ``fit_mesh_to_mesh`` Adam on the vertices against it -- the step that pulls a simplified mesh back onto the surface it
was made from.  The backward of the distance is ONE launch (rf_mesh_closest_gradients, csrc/mesh_distance_grad_kernels.hip): per
query the gradient on the query, G u, and a 9-float record -beta_k G u on the corners of its closest face.  Only when the vertices
want a gradient, one stable sort of the queries by face and the two segmented sums of rf_mesh_geometry_backward_gather follow -- the
gather the mesh render's backward uses, with queries in place of pixels: no atomics, two calls give the same bits.
include/relu_field.h has the contract, docs/mesh_distance_grad_errors.md the envelope argument and the error bounds,
tests/mesh_distance_grad_model.py the numpy model, DESIGN.md section 28 the measurements.  There is no CPU path.

Not done here: warm-starting a query from the previous iteration's face, fusing the sampler's records into the kernel, point clouds
as targets, a normal-consistency term.  (Signed distance: thr3ed_atom_amd/mesh_sign.py.)"""
import math
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, _marshal
from .mesh import Mesh
from .mesh_distance import ClosestPoints, MeshDistanceGrid, _count, sample_mesh_surface
from .mesh_fit import DEFAULT_LAPLACIAN_WEIGHT, DEFAULT_LR_FRACTION, MeshFit, _Laplacian, _weight, corner_slot_lists, gather_vertex_gradients, vertex_normals

MAX_QUERIES = 1 << 31


def closest_gradients_raw(vertices: Tensor, faces: Tensor, points: Tensor, face: Tensor, grad_distance: Tensor, status: Tensor, *, grad_points: Optional[Tensor] = None,
                          records: Optional[Tensor] = None, barycentrics: Optional[Tensor] = None, region: Optional[Tensor] = None) -> None:
    """Enqueue rf_mesh_closest_gradients (include/relu_field.h): per row of ``points`` (float32 [N, 3]) with closest face ``face`` (int64
    [N], -1: none) and upstream ``grad_distance`` (float32 [N]) the gradient on the query into ``grad_points`` (float32 [N, 3]), the
    corner records into ``records`` (float32 [N, 9]; rows of face -1 are NOT written), the barycentrics of the closest point into
    ``barycentrics`` (float32 [N, 3]) and the winning region into ``region`` (int32 [N]); each output may be None, not all.  ``status``
    (int32 [1], zeroed by the caller) becomes 1 for a face id or a vertex index outside its array.  One launch, no host
    synchronisation, no autograd."""
    n = int(points.shape[0])
    for t, dtype, shape, name in ((vertices, torch.float32, (int(vertices.shape[0]), 3), "vertices"), (faces, torch.int64, (int(faces.shape[0]), 3), "faces"),
                                  (points, torch.float32, (n, 3), "points"), (face, torch.int64, (n,), "face"), (grad_distance, torch.float32, (n,), "grad_distance"),
                                  (grad_points, torch.float32, (n, 3), "grad_points"), (records, torch.float32, (n, 9), "records"),
                                  (barycentrics, torch.float32, (n, 3), "barycentrics"), (region, torch.int32, (n,), "region"), (status, torch.int32, (1,), "status")):
        if t is None:
            continue
        if not t.is_cuda or t.device != points.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {points.device}")
    if n >= MAX_QUERIES:
        raise ValueError("rf_mesh_closest_gradients takes fewer than 2^31 queries")
    rc = _lib.load().rf_mesh_closest_gradients(vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), int(faces.shape[0]), points.data_ptr(), face.data_ptr(),
                                               grad_distance.data_ptr(), n, 0, _marshal.ptr(grad_points), _marshal.ptr(records), _marshal.ptr(barycentrics),
                                               _marshal.ptr(region), status.data_ptr(), _marshal.stream(points.device))
    _lib.check(rc, "rf_mesh_closest_gradients")


def face_entry_lists(face: Tensor, num_faces: int) -> Tuple[Tensor, Tensor]:
    """(entries int32 [hits] sorted by face, stably; face offsets int64 [T + 1]): the rows of ``face`` (int64 [N]) that name a face -- the
    first list of rf_mesh_geometry_backward_gather, queries in place of hit pixels"""
    entry = torch.nonzero(face >= 0).view(-1)
    keys, order = torch.sort(face[entry].clamp(max=max(num_faces - 1, 0)), stable=True)
    return entry[order].to(torch.int32).contiguous(), _marshal.segment_offsets(keys, num_faces)


def _sum_records(records: Tensor, face: Tensor, faces: Tensor, V: int, long_segment: int, status: Tensor, lists=None, corner_lists=None) -> Tensor:
    """[V, 3]: the records of the rows that name a face, summed per face and then per vertex, in gather form.  ``lists``: all four
    lists of the gather when the caller holds them; ``corner_lists``: the two that depend on the faces alone"""
    T = int(faces.shape[0])
    if not (T and V and int(records.shape[0])):
        return torch.zeros((V, 3), dtype=torch.float32, device=records.device)
    if lists is None:
        lists = (*face_entry_lists(face, T), *(corner_lists if corner_lists is not None else corner_slot_lists(faces, V)))
    entries, face_offsets, slots, vertex_offsets = lists
    return gather_vertex_gradients(records, entries, face_offsets, T, slots, vertex_offsets, V, long_segment, status)


class _Distance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points: Tensor, vertices: Tensor, grid: MeshDistanceGrid, limit: Optional[float], long_segment: int, holder: list, corner_lists):
        found = grid.closest(points.detach(), limit)
        ctx.grid, ctx.long_segment, ctx.corner_lists = grid, long_segment, corner_lists
        ctx.save_for_backward(points.detach().contiguous(), found.face)
        holder.append(ClosestPoints(found.distance.detach(), found.face, found.point))  # (the returned tensor itself joins the graph; its detached view does not)
        return found.distance

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_distance: Tensor):
        points, face = ctx.saved_tensors
        grid = ctx.grid
        vertices, faces = grid.vertices, grid.faces
        N, V, dev = int(points.shape[0]), int(vertices.shape[0]), points.device
        want_points, want_vertices = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_points = torch.zeros((N, 3), dtype=torch.float32, device=dev) if want_points else None
        grad_vertices = torch.zeros((V, 3), dtype=torch.float32, device=dev) if want_vertices else None
        if N and int(faces.shape[0]) and (want_points or want_vertices):
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            records = torch.empty((N, 9), dtype=torch.float32, device=dev) if want_vertices else None
            closest_gradients_raw(vertices, faces, points, face, grad_distance.to(torch.float32).contiguous(), status, grad_points=grad_points, records=records)
            if want_vertices:
                grad_vertices = _sum_records(records, face, faces, V, ctx.long_segment, status, corner_lists=ctx.corner_lists)
            if int(status.item()):  # (the one host read of the backward: a mesh that changed under the grid since the forward)
                raise ValueError("point_mesh_distance: a face id or a vertex index lies outside its array")
        return grad_points, grad_vertices, None, None, None, None, None


def _distance(points: Tensor, vertices: Tensor, grid: MeshDistanceGrid, limit: Optional[float] = None, long_segment: int = 0,
              corner_lists=None) -> Tuple[Tensor, ClosestPoints]:
    """the distance of ``points`` to the mesh ``grid`` was built over (``vertices``: the tensor the gradient goes to) and the forward's
    ClosestPoints; ``corner_lists``: ``corner_slot_lists`` of the grid's faces when the caller holds them (they depend on the faces
    alone), else the backward builds them"""
    holder: list = []
    distance = _Distance.apply(points, vertices, grid, limit, long_segment, holder, corner_lists)
    return distance, holder[0]


def _check_vertices(vertices, what: str) -> None:
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise ValueError(f"{what} takes vertices on a HIP device; there is no CPU path")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("vertices must be a float32 tensor of shape [V, 3]")


def point_mesh_distance(points: Tensor, vertices: Tensor, faces: Tensor, *, max_distance: Optional[float] = None, cell_size: Optional[float] = None) -> Tensor:
    """float32 [N]: the distance of every row of ``points`` (float32 [N, 3]) to the mesh (``vertices`` float32 [V, 3], ``faces`` integer
    [T, 3], all on one HIP device), differentiable with respect to ``points`` and ``vertices``.  The forward is
    ``MeshDistanceGrid(Mesh(vertices, faces), cell_size).closest(points, max_distance).distance`` bit for bit; that call's whole
    ClosestPoints (the closest face ids are the non-differentiable state of the backward) is readable as
    ``point_mesh_distance.last`` until the next call: three detached tensors of N rows, which hold no autograd graph and no grid
    (set it to None to release them).  Backward: dL/dp = G u and dL/d(corner k) = -beta_k G u with u the unit vector
    from the closest point to the query (0 on the surface: the subgradient) and beta the closest point's barycentrics -- one launch
    of rf_mesh_closest_gradients; when ``vertices`` wants a gradient, one stable sort of the queries by face and the gather launch of
    the mesh render's backward follow.  A query without a face within ``max_distance`` has distance +inf and gets and gives zero
    gradient.  The gradient does not depend on ``cell_size``, is not itself differentiable (a second backward raises), and two calls
    give the same bits.  One host read in the backward (the status word).
    ValueError: as ``MeshDistanceGrid`` and its ``closest``; CPU tensors."""
    _check_vertices(vertices, "point_mesh_distance")
    if not torch.is_tensor(points) or not points.is_cuda:
        raise ValueError("point_mesh_distance takes points on a HIP device; there is no CPU path")
    grid = MeshDistanceGrid(Mesh(vertices, faces, None, None), cell_size)
    distance, found = _distance(points, vertices, grid, max_distance)
    point_mesh_distance.last = found
    return distance


point_mesh_distance.last = None


class _SurfacePoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices: Tensor, faces: Tensor, sample_faces: Tensor, barycentrics: Tensor, long_segment: int, lists):
        corners = vertices.detach()[faces[sample_faces]]  # [N, 3, 3]
        b = barycentrics
        ctx.faces, ctx.V, ctx.long_segment, ctx.lists = faces, int(vertices.shape[0]), long_segment, lists
        ctx.save_for_backward(sample_faces, barycentrics)
        return (b[:, 0:1] * corners[:, 0] + b[:, 1:2] * corners[:, 1]) + b[:, 2:3] * corners[:, 2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad: Tensor):
        sample_faces, barycentrics = ctx.saved_tensors
        records = (barycentrics[:, :, None] * grad.to(torch.float32)[:, None, :]).reshape(-1, 9).contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=grad.device)  # (the gather wants one; the forward's callers checked the lists' ranges, so it stays 0 and is not read)
        return _sum_records(records, sample_faces, ctx.faces, ctx.V, ctx.long_segment, status, ctx.lists), None, None, None, None, None


def mesh_surface_points(vertices: Tensor, faces: Tensor, sample_faces: Tensor, barycentrics: Tensor) -> Tensor:
    """float32 [N, 3]: the points ``(b0 v0 + b1 v1) + b2 v2`` of the faces ``sample_faces`` (int64 [N]) at ``barycentrics`` (float32 [N, 3])
    -- what ``sample_mesh_surface`` draws -- in float32, differentiable with respect to ``vertices``.  The backward forms the [N, 9]
    records b_k g with one elementwise op and sums them per face and per vertex with one stable sort and the gather launch
    ``point_mesh_distance`` uses (``index_add_`` would add with atomics in an order that changes from run to run): two calls give the
    same bits; a second backward raises.  One host read (the range of ``sample_faces``).
    ValueError: CPU tensors, other shapes or types, a sample face outside the faces, a face outside the vertices."""
    _check_vertices(vertices, "mesh_surface_points")
    _, faces = _marshal.mesh_arrays(Mesh(vertices, faces, None, None), "mesh_surface_points")
    dev, N = vertices.device, int(sample_faces.shape[0]) if torch.is_tensor(sample_faces) and sample_faces.dim() == 1 else -1
    if N < 0 or sample_faces.dtype != torch.int64 or sample_faces.device != dev:
        raise ValueError(f"sample_faces must be an int64 tensor of shape [N] on {dev}")
    if not torch.is_tensor(barycentrics) or barycentrics.device != dev or barycentrics.dtype != torch.float32 or tuple(barycentrics.shape) != (N, 3):
        raise ValueError(f"barycentrics must be a float32 tensor of shape [{N}, 3] on {dev}")
    if N >= MAX_QUERIES:
        raise ValueError("mesh_surface_points takes fewer than 2^31 samples")
    if N:
        T, V = int(faces.shape[0]), int(vertices.shape[0])
        low, high, face_low, face_high = torch.stack([sample_faces.min(), sample_faces.max(), faces.min() if T else sample_faces.min(),
                                                       faces.max() if T else sample_faces.min()]).cpu().tolist()
        if low < 0 or high >= T:
            raise ValueError(f"sample_faces index outside [0, {T})")
        if face_low < 0 or face_high >= V:
            raise ValueError(f"faces index outside [0, {V})")
    return _SurfacePoints.apply(vertices, faces, sample_faces.detach().contiguous(), barycentrics.detach().contiguous(), 0, None)


class MeshChamferLoss:
    """The symmetric Chamfer distance between a moving mesh (``faces`` integer [T, 3], its vertices given per call) and a fixed
    ``target`` Mesh, as a differentiable function of the moving vertices.  Built once, it holds the target's ``MeshDistanceGrid``,
    ``samples`` points of the target's surface (``sample_mesh_surface`` with ``seed + 1``) and the moving mesh's sample faces and
    barycentrics, drawn with ``seed`` on the vertices of the first call and redrawn with ``seed + 2 k`` at call k ``resample_every``, 2
    ``resample_every``, ... when that option is set (``seed + 2 k`` never meets the target's ``seed + 1``).
    ``loss(vertices)`` = half the sum of the two directed means -- of the distances from the moving samples
    (``mesh_surface_points``) to the target and from the target's samples to the moving mesh (``point_mesh_distance``); with
    ``squared`` the means are of squared distances.  Each mean is taken in float64 and the value returned as a float32 scalar: at the
    starting vertices it equals ``mesh_distance(moving, target, samples=, seed=).chamfer_l1`` (``chamfer_l2``) to float32 rounding.
    The moving mesh's search structure is rebuilt on every call, from the second call on with the cell size the first call chose
    (which skips the default's ladder of host reads; a lattice that outgrows the limits falls back to the default's choice).
    ``last`` holds the two ClosestPoints (moving samples on the target, target samples on the moving mesh) of the latest call.
    ValueError: as ``MeshDistanceGrid`` and ``sample_mesh_surface``; samples < 1; ``resample_every`` < 1."""

    def __init__(self, faces: Tensor, target: Mesh, *, samples: int = 100_000, seed: int = 0, squared: bool = False, resample_every: Optional[int] = None):
        self.samples = _count(samples, "samples")
        if self.samples < 1:
            raise ValueError("samples must be at least 1")
        if resample_every is not None and _count(resample_every, "resample_every") < 1:
            raise ValueError("resample_every must be at least 1")
        if not torch.is_tensor(faces) or not faces.is_cuda:
            raise ValueError("MeshChamferLoss takes faces on a HIP device; there is no CPU path")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
            raise ValueError("faces must be an integer tensor of shape [T, 3]")
        self.faces = faces.detach().to(torch.int64).contiguous()
        self.seed, self.squared, self.resample_every = int(seed), bool(squared), None if resample_every is None else int(resample_every)
        self.target_grid = MeshDistanceGrid(target)
        self.target_points = sample_mesh_surface(target, self.samples, seed=self.seed + 1)[0]
        self.long_segment = 0  # (the library's default; tools/mesh_chamfer_time.py and the tests set others)
        self.calls, self.cell_size = 0, None
        self.sample_faces = self.barycentrics = self._lists = None
        self.last = None

    def _draw(self, vertices: Tensor, k: int) -> None:
        _, self.sample_faces, self.barycentrics = sample_mesh_surface(Mesh(vertices.detach(), self.faces, None, None), self.samples, seed=self.seed + 2 * k)
        V = int(vertices.shape[0])
        self._lists = (*face_entry_lists(self.sample_faces, int(self.faces.shape[0])), *corner_slot_lists(self.faces, V))

    def _moving_grid(self, vertices: Tensor) -> MeshDistanceGrid:
        mesh = Mesh(vertices.detach(), self.faces, None, None)
        if self.cell_size is not None:
            try:
                return MeshDistanceGrid(mesh, self.cell_size)
            except ValueError:
                _marshal.require_finite_vertices(vertices.detach())  # (a lattice over the limits goes on; anything else is the caller's)
        grid = MeshDistanceGrid(mesh)
        self.cell_size = grid.cell_size if grid.lattice is not None else None
        return grid

    def _mean(self, distance: Tensor) -> Tensor:
        d = distance.double()
        return (d * d).mean() if self.squared else d.mean()

    def __call__(self, vertices: Tensor) -> Tensor:
        _check_vertices(vertices, "MeshChamferLoss")
        if vertices.device != self.faces.device:
            raise ValueError(f"the vertices must be on {self.faces.device}")
        if self.sample_faces is None:
            self._draw(vertices, 0)
        elif self.resample_every is not None and self.calls % self.resample_every == 0:
            self._draw(vertices, self.calls // self.resample_every)
        self.calls += 1
        moving_points = _SurfacePoints.apply(vertices, self.faces, self.sample_faces, self.barycentrics, self.long_segment, self._lists)
        to_target, found_ab = _distance(moving_points, self.target_grid.vertices, self.target_grid, None, self.long_segment)
        to_moving, found_ba = _distance(self.target_points, vertices, self._moving_grid(vertices), None, self.long_segment, self._lists[2:])
        self.last = (found_ab, found_ba)
        return (0.5 * (self._mean(to_target) + self._mean(to_moving))).to(torch.float32)


def _mean_edge_length(vertices: Tensor, edges: Tensor) -> float:
    length = float((vertices[edges[:, 0]] - vertices[edges[:, 1]]).norm(dim=1).mean()) if edges.shape[0] else 1.0
    return length if math.isfinite(length) and length > 0.0 else 1.0


def fit_mesh_to_mesh(mesh: Mesh, target: Mesh, *, iterations: int = 200, lr: Optional[float] = None, samples: int = 100_000, squared: bool = False,
                     laplacian_weight: float = DEFAULT_LAPLACIAN_WEIGHT, max_move: Optional[float] = None, resample_every: Optional[int] = None, seed: int = 0,
                     callback: Optional[Callable[[int, Tensor], None]] = None) -> MeshFit:
    """Move ``mesh.vertices`` onto the surface of ``target``: the loop of ``fit_mesh_to_views`` with ``MeshChamferLoss`` as its data term.
    The loss is Chamfer(v) / e (``squared``: / e^2) + ``laplacian_weight`` mean_i |L(v)_i - L(v_start)_i|^2 / e^2, with e the mean
    edge length of the starting mesh and L(v)_i = v_i - the mean of its edge neighbours: both terms are measured in edge lengths, so
    the weights mean the same at every scale, and the Laplacian is held to the INITIAL mesh's.  ``torch.optim.Adam`` on the vertices;
    ``lr`` defaults to 0.05 e.  ``max_move`` (world units): after each step every vertex is pulled back into the ball of that radius
    round its start.  ``samples``, ``seed``, ``resample_every``: those of ``MeshChamferLoss``.  ``iterations=0`` returns the mesh itself.
    ``callback(iteration, loss)`` gets the device scalar of every iteration.  Faces and colours are unchanged; vertex normals are
    recomputed (area-weighted) when the mesh had them.  Returns MeshFit(mesh, history, moved): ``history`` holds the loss BEFORE each
    step.  Two calls give the same bits.
    ValueError: as ``MeshChamferLoss``; ``iterations`` < 0; ``lr`` or ``max_move`` not positive and finite; a negative weight."""
    vertices, faces = _marshal.mesh_arrays(mesh, "fit_mesh_to_mesh")
    _marshal.mesh_arrays(target, "fit_mesh_to_mesh")
    iterations = _marshal.iteration_count(iterations)
    lr = None if lr is None else _marshal.positive(lr, "lr")
    max_move = None if max_move is None else _marshal.positive(max_move, "max_move")
    laplacian_weight = _weight(laplacian_weight, "laplacian_weight")
    dev, V = vertices.device, int(vertices.shape[0])
    history = torch.zeros(iterations, dtype=torch.float32, device=dev)
    moved = torch.zeros(V, dtype=torch.float32, device=dev)
    if not iterations or not V or not faces.shape[0]:
        return MeshFit(mesh, history, moved)
    chamfer = MeshChamferLoss(faces, target, samples=samples, seed=seed, squared=squared, resample_every=resample_every)
    laplacian = _Laplacian(faces, V)
    edge_length = _mean_edge_length(vertices, laplacian.edges)
    scale = edge_length * edge_length if squared else edge_length
    if lr is None:
        lr = DEFAULT_LR_FRACTION * edge_length
    start = vertices.clone()
    start_laplacian = laplacian(start)
    param = start.clone().requires_grad_(True)
    optimiser = torch.optim.Adam([param], lr=lr)
    losses = []
    for it in range(iterations):
        optimiser.zero_grad(set_to_none=True)
        value = chamfer(param) / scale
        if laplacian_weight > 0.0:
            value = value + laplacian_weight * ((laplacian(param) - start_laplacian) ** 2).sum(1).mean() / (edge_length * edge_length)
        value.backward()
        optimiser.step()
        if max_move is not None:
            with torch.no_grad():
                step = param - start
                length = step.norm(dim=1, keepdim=True)
                param.copy_(start + step * (max_move / length.clamp(min=max_move)))
        losses.append(value.detach())
        if callback is not None:
            callback(it, losses[-1])
    history = torch.stack(losses).to(torch.float32)
    fitted = param.detach()
    normals = vertex_normals(fitted, faces) if mesh.normals is not None else None
    return MeshFit(mesh._replace(vertices=fitted, normals=normals), history, (fitted - start).norm(dim=1))
