"""Fitting the VERTICES of a mesh to posed views: the step between ``simplify_mesh`` and the texture bakes that moves the surface
towards what the field shows from a camera.  ``MeshGeometryRenderer`` turns vertex positions into two images per view that are
differentiable with respect to them -- the depth of ``render_mesh`` (bit for bit) and an anti-aliased coverage in [0, 1], the
edge-crossing rule of nvdiffrast restricted to hit-against-miss pixel pairs -- by one visibility and one coverage launch per view
(rf_mesh_raster_visibility, rf_mesh_raster_coverage), and back by one launch per view that writes a 9-float record per hit pixel
(rf_mesh_geometry_backward_pixels), one stable sort of the hit pixels by face, and two segmented sums without atomics
(rf_mesh_geometry_backward_gather: per face, then per vertex over a corner list built once per mesh).  ``fit_mesh_to_views`` runs
Adam on the vertices against depth and alpha images, ``fit_mesh_to_field_views`` takes both from the field's own median depth and
accumulated weight -- the quantities ``evaluate_mesh_against_field`` scores against.  DESIGN.md section 25 has the contract and the
measurements, docs/mesh_fit_errors.md the error bound, tests/mesh_fit_model.py the float64 model.

Not done here: silhouettes between two HIT pixels (self-occlusion), colour gradients to vertices, topology changes, camera gradients
through the rasteriser."""
import ctypes as C
import math
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib, _marshal
from .constants import EXTRA_ACCUMULATED_WEIGHTS
from .mesh import Mesh
from .texture import _view_chunk

MAX_PIXELS = 1 << 31
# the default step of fit_mesh_to_views is this fraction of the mean edge length (DESIGN.md section 25 has the sweep that chose it)
DEFAULT_LR_FRACTION = 0.05
DEFAULT_LAPLACIAN_WEIGHT = 1.0


class MeshFit(NamedTuple):
    mesh: Mesh       # the mesh with the fitted vertices (faces and colours are the input's; normals recomputed when it had them)
    history: Tensor  # [iterations] float32 on the device: the loss BEFORE each step
    moved: Tensor    # [V] float32: how far each vertex went from its start


def corner_slot_lists(faces: Tensor, V: int) -> Tuple[Tensor, Tensor]:
    """(corner slots int32 [3 T], vertex offsets int64 [V + 1]) of int64 ``faces`` [T, 3]: the slots 3 face + corner sorted by the vertex
    they name (stable) -- the second list of rf_mesh_geometry_backward_gather"""
    flat = faces.view(-1)
    _, order = torch.sort(flat, stable=True)
    return order.to(torch.int32).contiguous(), _marshal.segment_offsets(flat.clamp(0, max(V - 1, 0)), V)


def gather_vertex_gradients(records: Tensor, entries: Tensor, face_offsets: Tensor, num_faces: int, slots: Tensor, vertex_offsets: Tensor, V: int,
                            long_segment: int, status: Tensor) -> Tensor:
    """[V, 3] float32 from 9-float ``records`` [P, 9]: rf_mesh_geometry_backward_gather, the two segmented sums without atomics
    (``entries`` int32: the rows that count, sorted by face, stably; ``face_offsets`` int64 [T + 1]).  What the mesh render's and the
    mesh distance's backward share."""
    dev = records.device
    face_grads = torch.empty((num_faces, 9), dtype=torch.float32, device=dev)
    grad = torch.empty((V, 3), dtype=torch.float32, device=dev)
    rc = _lib.load().rf_mesh_geometry_backward_gather(records.data_ptr(), int(records.shape[0]), entries.data_ptr(), int(entries.shape[0]), face_offsets.data_ptr(), num_faces,
                                                      slots.data_ptr(), vertex_offsets.data_ptr(), V, long_segment, 0, face_grads.data_ptr(), grad.data_ptr(),
                                                      status.data_ptr(), _marshal.stream(dev))
    _lib.check(rc, "rf_mesh_geometry_backward_gather")
    return grad


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices: Tensor, renderer: "MeshGeometryRenderer"):
        depth, coverage, face_ids = renderer._forward(vertices.detach().contiguous())
        ctx.renderer, ctx.vertices = renderer, vertices.detach().contiguous()
        ctx.save_for_backward(coverage, face_ids)
        ctx.mark_non_differentiable(face_ids)
        return depth, coverage, face_ids

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_depth, grad_coverage, _grad_ids):
        coverage, face_ids = ctx.saved_tensors
        return ctx.renderer._backward(ctx.vertices, face_ids, coverage, grad_depth, grad_coverage), None


class MeshGeometryRenderer:
    """The depth and the anti-aliased coverage of ``faces`` over ``poses`` as a differentiable function of the vertex positions.
    ``renderer(vertices)`` (float32 [V, 3] on the faces' device) returns ``(depth [N, H, W], coverage [N, H, W])``: ``depth`` equals
    ``render_mesh(...).depth`` bit for bit (0 where nothing was hit); ``coverage`` is 1 inside, 0 outside and in between on the two
    pixels either side of a silhouette that runs against the background (include/relu_field.h has the rule).  ``last_face_ids``
    [N, H, W] int32 holds the winning faces of the latest call (-1: nothing).  The gradient goes to ``vertices`` only and is not
    itself differentiable (a second backward raises); two calls give the same bits.  Per call: one visibility and one coverage
    launch per view; per backward: one launch per view, one stable sort, two gather launches.  Zero views, zero faces or views that
    all miss need no backward launch and give zero gradients.
    ValueError: as ``render_mesh`` for the mesh, the intrinsics, the poses and ``near``; N H W >= 2^31."""

    def __init__(self, faces: Tensor, poses: Sequence, camera_intrinsics, *, near: float = 0.0, cull_backfaces: bool = False):
        if not torch.is_tensor(faces) or not faces.is_cuda:
            raise ValueError("MeshGeometryRenderer takes faces on a HIP device; there is no CPU path")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
            raise ValueError("faces must be an integer tensor of shape [T, 3]")
        self.faces = faces.detach().to(torch.int64).contiguous()
        self.device = self.faces.device
        self.near = _marshal.non_negative(near, "near")
        self.flags = _lib.RASTER_CULL_BACKFACES if cull_backfaces else 0
        self.long_segment = 0  # (the library's default; tools/mesh_fit_time.py and the tests set others)
        self.cams = [_marshal.checked_camera(pose, camera_intrinsics) for pose in poses]
        _marshal.checked_camera(_marshal.identity_pose(), camera_intrinsics)  # (the intrinsics' own errors, even with zero views)
        self.N, self.H, self.W = len(self.cams), int(camera_intrinsics[0]), int(camera_intrinsics[1])
        self.P = self.N * self.H * self.W
        if self.P >= MAX_PIXELS:
            raise ValueError(f"{self.N} views of {self.H} x {self.W} pixels are {self.P} pixels: the renderer takes fewer than 2^31")
        self.T = int(self.faces.shape[0])
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.last_face_ids = None
        self._corners = None  # (corner slots, vertex offsets, V): built at the first backward

    def __call__(self, vertices: Tensor) -> Tuple[Tensor, Tensor]:
        if not torch.is_tensor(vertices) or vertices.device != self.device or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError(f"the vertices must be a float32 tensor of shape [V, 3] on {self.device}")
        depth, coverage, face_ids = _Render.apply(vertices, self)
        self.last_face_ids = face_ids
        return depth, coverage

    def _forward(self, vertices: Tensor):
        dev, N, H, W, T, V = self.device, self.N, self.H, self.W, self.T, int(vertices.shape[0])
        depth = torch.zeros((N, H, W), dtype=torch.float32, device=dev)
        coverage = torch.zeros((N, H, W), dtype=torch.float32, device=dev)
        face_ids = torch.full((N, H, W), -1, dtype=torch.int32, device=dev)
        if T and N:
            lib = _lib.load()
            _marshal.require_finite_vertices(vertices)
            stream = _marshal.stream(dev)
            visibility = torch.empty((H, W), dtype=torch.int64, device=dev)
            for k, cam in enumerate(self.cams):
                _marshal.raster_visibility(cam, vertices, self.faces, self.near, self.flags, visibility, self.status)
                rc = lib.rf_mesh_raster_coverage(C.byref(cam), vertices.data_ptr(), V, self.faces.data_ptr(), T, visibility.data_ptr(), self.flags, depth[k].data_ptr(),
                                                 coverage[k].data_ptr(), face_ids[k].data_ptr(), stream)
                _lib.check(rc, "rf_mesh_raster_coverage")
            _marshal.require_faces_in_range(self.status, V)
        return depth, coverage, face_ids

    def corner_lists(self, V: int):
        """(corner slots int32 [3 T], vertex offsets int64 [V + 1]): the slots 3 face + corner sorted by the vertex they name (stable)"""
        if self._corners is None or self._corners[2] != V:
            self._corners = (*corner_slot_lists(self.faces, V), V)
        return self._corners[0], self._corners[1]

    def hit_lists(self, face_ids: Tensor):
        """(hit pixels int32 [hits] sorted by face, stably; face offsets int64 [T + 1]) of one forward's face ids"""
        ids = face_ids.view(-1)
        pixel = torch.nonzero(ids >= 0).view(-1)
        face, order = torch.sort(ids[pixel].to(torch.int64), stable=True)
        return pixel[order].to(torch.int32).contiguous(), _marshal.segment_offsets(face, self.T)

    def _records(self, vertices: Tensor, face_ids: Tensor, coverage: Tensor, grad_depth: Tensor, grad_coverage: Tensor) -> Tensor:
        """stage 1: [P, 9] float32, written at the hit pixels only"""
        lib, stream, V = _lib.load(), _marshal.stream(self.device), int(vertices.shape[0])
        records = torch.empty((self.N, self.H * self.W, 9), dtype=torch.float32, device=self.device)
        for k, cam in enumerate(self.cams):
            rc = lib.rf_mesh_geometry_backward_pixels(C.byref(cam), vertices.data_ptr(), V, self.faces.data_ptr(), self.T, face_ids[k].data_ptr(), coverage[k].data_ptr(),
                                                      grad_depth[k].data_ptr(), grad_coverage[k].data_ptr(), self.flags, records[k].data_ptr(), self.status.data_ptr(), stream)
            _lib.check(rc, "rf_mesh_geometry_backward_pixels")
        return records.view(self.P, 9)

    def _gather(self, records: Tensor, hit_pixels: Tensor, face_offsets: Tensor, V: int) -> Tensor:
        """stage 2: [V, 3] float32"""
        slots, vertex_offsets = self.corner_lists(V)
        return gather_vertex_gradients(records, hit_pixels, face_offsets, self.T, slots, vertex_offsets, V, self.long_segment, self.status)

    def _backward(self, vertices: Tensor, face_ids: Tensor, coverage: Tensor, grad_depth: Tensor, grad_coverage: Tensor) -> Tensor:
        V = int(vertices.shape[0])
        if not (self.T and self.N and V):
            return torch.zeros((V, 3), dtype=torch.float32, device=self.device)
        hit_pixels, face_offsets = self.hit_lists(face_ids)
        if not int(hit_pixels.shape[0]):  # views that all look past the mesh: no launch
            return torch.zeros((V, 3), dtype=torch.float32, device=self.device)
        grad_depth = grad_depth.to(torch.float32).contiguous()
        grad_coverage = grad_coverage.to(torch.float32).contiguous()
        records = self._records(vertices, face_ids, coverage, grad_depth, grad_coverage)
        return self._gather(records, hit_pixels, face_offsets, V)


def _edge_list(faces: Tensor) -> Tensor:
    """the undirected edges [E, 2] of the faces, each once"""
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    e = torch.sort(e, dim=1).values
    e = e[e[:, 0] != e[:, 1]]
    return torch.unique(e, dim=0) if e.shape[0] else e


class _NeighbourMean(torch.autograd.Function):
    """v -> v - the mean of its edge neighbours, as a GATHER over a padded neighbour table in both directions: the adjacency is
    symmetric, so the adjoint is g -> g - sum over the neighbours j of g_j / degree_j, again a gather.  ``index_add`` would add with
    atomics in an order that changes from run to run; this repeats its bits."""

    @staticmethod
    def forward(ctx, vertices: Tensor, table: Tensor, degree: Tensor) -> Tensor:
        ctx.save_for_backward(table, degree)
        padded = torch.cat([vertices, torch.zeros((1, 3), dtype=vertices.dtype, device=vertices.device)])
        return vertices - padded[table].sum(1) / degree

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad: Tensor):
        table, degree = ctx.saved_tensors
        padded = torch.cat([grad / degree, torch.zeros((1, 3), dtype=grad.dtype, device=grad.device)])
        return grad - padded[table].sum(1), None, None


class _Laplacian:
    """v_i - the mean of its edge neighbours, over an edge list built once (a vertex without neighbours gets v_i - 0)"""

    def __init__(self, faces: Tensor, V: int):
        e = self.edges = _edge_list(faces)
        src, dst = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
        src, order = torch.sort(src, stable=True)
        dst = dst[order]
        counts = torch.bincount(src, minlength=V)
        first = torch.cumsum(counts, 0) - counts
        width = int(counts.max()) if src.numel() else 0
        self.table = torch.full((V, max(width, 1)), V, dtype=torch.int64, device=faces.device)  # (V: the zero row appended in the gather)
        if src.numel():
            self.table[src, torch.arange(src.numel(), device=faces.device) - first[src]] = dst
        self.degree = counts.clamp(min=1).to(torch.float32)[:, None]

    def __call__(self, vertices: Tensor) -> Tensor:
        return _NeighbourMean.apply(vertices, self.table, self.degree)


def vertex_normals(vertices: Tensor, faces: Tensor) -> Tensor:
    """area-weighted vertex normals, normalised (0 where they vanish)"""
    v = vertices[faces]
    n = torch.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], dim=1)
    total = torch.zeros_like(vertices)
    for k in range(3):
        total = total.index_add(0, faces[:, k], n)
    length = total.norm(dim=1, keepdim=True)
    return torch.where(length > 0, total / length.clamp(min=1e-30), torch.zeros_like(total))


def _weight(value, name: str) -> float:
    value = float(value)
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f"{name} must be non-negative and finite, got {value!r}")
    return value


def fit_loss(depth: Tensor, coverage: Tensor, face_ids: Tensor, depths: Tensor, alphas: Tensor, depth_weight: float, mask_weight: float) -> Tensor:
    """mask_weight mean((A - alpha)^2) over all pixels + depth_weight mean |D - depth| over the pixels that are hit and have alpha > 1/2
    (0 when there are none)"""
    value = mask_weight * ((coverage - alphas) ** 2).mean() if coverage.numel() else coverage.sum()
    both = (face_ids >= 0) & (alphas > 0.5)
    count = both.sum()
    residual = torch.where(both, (depth - depths).abs(), torch.zeros((), dtype=torch.float32, device=depth.device))
    return value + depth_weight * residual.sum() / count.clamp(min=1).to(torch.float32)


def fit_mesh_to_views(mesh: Mesh, depths, alphas, poses: Sequence, camera_intrinsics, *, iterations: int = 200, lr: Optional[float] = None, depth_weight: float = 1.0,
                      mask_weight: float = 1.0, laplacian_weight: float = DEFAULT_LAPLACIAN_WEIGHT, max_move: Optional[float] = None, near: float = 0.0,
                      cull_backfaces: bool = False, callback: Optional[Callable[[int, Tensor], None]] = None, target_mesh: Optional[Mesh] = None,
                      chamfer_weight: float = 0.0, chamfer_samples: int = 100_000) -> MeshFit:
    """Move ``mesh.vertices`` so that ``MeshGeometryRenderer``'s images match posed targets.  ``depths`` [N, H, W] (or N [H, W]): the
    ray-parameter depth per pixel, as ``RenderOut.depth`` holds it; ``alphas`` [N, H, W]: the coverage in [0, 1]; ``poses`` N CameraPose
    of one ``camera_intrinsics``.  The loss is ``mask_weight`` mean((A - alpha)^2) over all pixels + ``depth_weight`` mean |D - depth|
    over the pixels that are hit and have alpha > 1/2 + ``laplacian_weight`` mean_i |L(v)_i - L(v_start)_i|^2 / (mean edge length)^2
    with L(v)_i = v_i - the mean of its edge neighbours: the Laplacian is held to the INITIAL mesh's, so a mesh that already fits is
    a fixed point, and it is measured in edge lengths, so the weight means the same at every scale.  With ``target_mesh`` and a
    positive ``chamfer_weight`` the loss gains ``chamfer_weight`` x ``MeshChamferLoss(faces, target_mesh, samples=chamfer_samples)(v)`` /
    (mean edge length), the data term of ``fit_mesh_to_mesh``; with ``target_mesh=None`` or weight 0 nothing is built or launched for it.

    ``torch.optim.Adam`` on the vertices; ``lr`` defaults to 0.05 x the mean edge length.  ``max_move`` (world units): after each step
    every vertex is pulled back into the ball of that radius round its start.  ``iterations=0`` returns the mesh itself.
    ``callback(iteration, loss)`` gets the device scalar of every iteration (reading it synchronises; nothing else in the loop does
    but the rasteriser's own checks).  Faces and colours are unchanged; vertex normals are recomputed (area-weighted) when the mesh
    had them.  Returns MeshFit(mesh, history, moved).  Two calls give the same bits.
    ValueError: as ``MeshGeometryRenderer``; counts or sizes of depths, alphas and poses that do not match; ``iterations`` < 0; ``lr`` or
    ``max_move`` not positive and finite; a weight that is negative or not finite."""
    vertices, faces = _marshal.mesh_arrays(mesh, "fit_mesh_to_views")
    poses = list(poses)
    N = len(poses)
    if len(depths) != N or len(alphas) != N:
        raise ValueError(f"{len(depths)} depths, {len(alphas)} alphas, {N} poses: the counts must match")
    iterations = _marshal.iteration_count(iterations)
    lr = None if lr is None else _marshal.positive(lr, "lr")
    max_move = None if max_move is None else _marshal.positive(max_move, "max_move")
    depth_weight, mask_weight, laplacian_weight = _weight(depth_weight, "depth_weight"), _weight(mask_weight, "mask_weight"), _weight(laplacian_weight, "laplacian_weight")
    chamfer_weight = _weight(chamfer_weight, "chamfer_weight")
    H, W = int(camera_intrinsics[0]), int(camera_intrinsics[1])
    dev, V = vertices.device, int(vertices.shape[0])
    renderer = MeshGeometryRenderer(faces, poses, camera_intrinsics, near=near, cull_backfaces=cull_backfaces)
    targets = []
    for name, given in (("depths", depths), ("alphas", alphas)):
        given = _view_chunk(given, 0, N, None, name) if N else torch.zeros((0, H, W))
        if given.dim() == 4 and given.shape[-1] == 1:
            given = given[..., 0]
        if tuple(given.shape) != (N, H, W):
            raise ValueError(f"the {name} of {N} views of {H} x {W} pixels must have shape {(N, H, W)}, got {tuple(given.shape)}")
        targets.append(given.detach().to(dev, torch.float32).contiguous())
    depths, alphas = targets
    history = torch.zeros(iterations, dtype=torch.float32, device=dev)
    moved = torch.zeros(V, dtype=torch.float32, device=dev)
    if not iterations or not V or not faces.shape[0] or not N:
        return MeshFit(mesh, history, moved)
    laplacian = _Laplacian(faces, V)
    edges = laplacian.edges
    edge_length = float((vertices[edges[:, 0]] - vertices[edges[:, 1]]).norm(dim=1).mean()) if edges.shape[0] else 1.0
    if not (math.isfinite(edge_length) and edge_length > 0.0):
        edge_length = 1.0
    if lr is None:
        lr = DEFAULT_LR_FRACTION * edge_length
    start = vertices.clone()
    start_laplacian = laplacian(start)
    param = start.clone().requires_grad_(True)
    optimiser = torch.optim.Adam([param], lr=lr)
    chamfer = None
    if target_mesh is not None and chamfer_weight > 0.0:
        from .mesh_distance_grad import MeshChamferLoss  # (it imports this module)
        chamfer = MeshChamferLoss(faces, target_mesh, samples=chamfer_samples)
    losses = []
    for it in range(iterations):
        optimiser.zero_grad(set_to_none=True)
        depth, coverage = renderer(param)
        value = fit_loss(depth, coverage, renderer.last_face_ids, depths, alphas, depth_weight, mask_weight)
        if chamfer is not None:
            value = value + chamfer_weight * chamfer(param) / edge_length
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


def fit_mesh_to_field_views(mesh: Mesh, vol_mod, poses: Sequence, camera_intrinsics, *, render_overrides: Optional[dict] = None, **kw) -> MeshFit:
    """``fit_mesh_to_views`` against the field's own geometry: for every pose ``vol_mod.render_geometry(pose, camera_intrinsics,
    quantile=0.5)`` gives the target depth (the median depth) and its accumulated weight the target alpha -- the two quantities
    ``evaluate_mesh_against_field`` scores ``depth_l1`` and ``mask_iou`` against.  ``render_overrides`` are passed on to the render
    (``white_bkgd`` concerns colour only and is dropped); the other keywords are those of ``fit_mesh_to_views``."""
    overrides = {k: v for k, v in dict(render_overrides or {}).items() if k != "white_bkgd"}
    dev = mesh.vertices.device
    depths, accs = [], []
    with torch.no_grad():
        for pose in poses:
            geometry = vol_mod.render_geometry(pose, camera_intrinsics, quantile=0.5, **overrides)
            depths.append(geometry.depth[..., 0].to(dev, torch.float32))
            accs.append(geometry.extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].to(dev, torch.float32))
    return fit_mesh_to_views(mesh, depths, accs, list(poses), camera_intrinsics, **kw)
