"""Fitting a baked texture to posed views: the step after ``bake_texture`` / ``bake_texture_from_views`` that minimises what
``evaluate_mesh_against_field`` measures, the image-space error of ``render_mesh`` against the views.  With mesh, atlas and cameras
fixed a view's colour image is a fixed sparse linear map of the texture -- four bilinear taps per hit pixel -- so nothing is
rasterised per iteration: ``MeshTextureSampler`` rasterises every view ONCE (rf_mesh_raster_visibility and rf_mesh_raster_taps of
csrc/mesh_raster_kernels.hip), keeps one 16-byte tap record per pixel and the transposed list (per texel, its pixels and weights),
and is then a ``torch.autograd.Function`` whose forward is one gather launch (rf_texture_sample: the colours of ``render_mesh`` bit
for bit) and whose backward is one gather launch over the transposed list (rf_texture_sample_backward: no atomics, two calls give
the same bits).  ``fit_texture`` runs Adam on the texture under an L2 or L1 (+ D-SSIM, ``rf.ssim``) loss.  DESIGN.md section 24 has
the contract and the measurements, docs/texture_fit_errors.md the error bound, tests/texture_fit_model.py the float64 model.

Only the texture gets a gradient.  Not done here: gradients to geometry, UVs, cameras or vertex colours (they need anti-aliased
silhouettes), mini-batches of views, a conjugate-gradient solver for the L2 case, per-view exposure, seam blending, mip-mapped
atlases."""
import ctypes as C
from typing import Callable, NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from . import _lib, _marshal
from .constants import EXTRA_ACCUMULATED_WEIGHTS
from .mesh import Mesh
from .mesh_raster import _check_raster_mesh
from .metrics import ssim
from .texture import TextureBake, _view_chunk

NO_TAP = _lib.TEXTURE_NO_TAP
MAX_PIXELS = 1 << 31
DEFAULT_LR = 0.03  # chosen among 1e-3 .. 1e-1 on the scene of DESIGN.md sections 21-24 (the loss curves are there)


class TextureFit(NamedTuple):
    bake: TextureBake  # the bake with the fitted texture (layout, UVs and opacity are the input's)
    history: Tensor    # [iterations] float32 on the device: the loss BEFORE each step
    coverage: Tensor   # [Ht, Wt] int32: the taps per texel over all views (texels with 0 keep the input's bits)


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture: Tensor, sampler: "MeshTextureSampler") -> Tensor:
        ctx.sampler = sampler
        return sampler._forward(texture.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_colour: Tensor):
        return ctx.sampler._backward(grad_colour), None


class MeshTextureSampler:
    """The colour images of ``render_mesh(mesh, pose, camera_intrinsics, bake)`` over ``poses`` as a differentiable function of the
    texture alone.  Only ``bake.uvs`` and the SHAPE of ``bake.texture`` are used.  Construction runs one visibility and one taps
    launch per view and one stable sort; ``sampler(texture)`` ([Ht, Wt, 3] float32 on the mesh's device) returns [N, H, W, 3], equal to
    the stack of ``render_mesh(...).colour`` bit for bit, with ``background`` (any non-negative value) at the pixels nothing covers.
    The gradient goes to ``texture`` only and is not itself differentiable (a second backward raises).

    ``mask`` [N, H, W] bool: the hit pixels.  ``coverage`` [Ht, Wt] int32: the taps per texel (a tap clamped at the atlas edge counts
    twice).  ``num_entries``: 4 x the hit pixels.  ``taps`` [N H W, 4] int32: the raw RFTextureTap records.  Zero views or an empty
    mesh need no launch and give a zero gradient.  ValueError: as ``render_mesh`` for the mesh, the bake, the intrinsics, the poses
    and ``near``; a ``background`` that is negative or not finite; N H W >= 2^31."""

    def __init__(self, mesh: Mesh, bake: TextureBake, poses: Sequence, camera_intrinsics, *, near: float = 0.0, cull_backfaces: bool = False,
                 background: float = 0.0):
        if bake is None:
            raise ValueError("MeshTextureSampler needs a bake (its UVs and the shape of its texture)")
        self.vertices, self.faces, self.uvs, texture, _ = _check_raster_mesh(mesh, bake)
        self.near = _marshal.non_negative(near, "near")
        self.background = _marshal.non_negative(background, "background")
        self.long_segment = 0  # (the library's default; tools/texture_fit_time.py sets others for its A/B)
        poses = list(poses)
        cams = [_marshal.checked_camera(pose, camera_intrinsics) for pose in poses]
        _marshal.checked_camera(_marshal.identity_pose(), camera_intrinsics)  # (the intrinsics' own errors, even with zero views)
        self.N, self.H, self.W = len(poses), int(camera_intrinsics[0]), int(camera_intrinsics[1])
        self.Ht, self.Wt = int(texture.shape[0]), int(texture.shape[1])
        self.P = self.N * self.H * self.W
        if self.P >= MAX_PIXELS:
            raise ValueError(f"{self.N} views of {self.H} x {self.W} pixels are {self.P} pixels: the sampler takes fewer than 2^31")
        dev = self.device = self.vertices.device
        T, V = self.faces.shape[0], self.vertices.shape[0]
        self.taps = torch.empty((self.P, 4), dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        texels = self.Ht * self.Wt
        with torch.no_grad():
            if T and self.N:
                lib = _lib.load()
                _marshal.require_finite_vertices(self.vertices)
                flags = _lib.RASTER_CULL_BACKFACES if cull_backfaces else 0
                stream = _marshal.stream(dev)
                visibility = torch.empty((self.H, self.W), dtype=torch.int64, device=dev)
                per_view = self.taps.view(self.N, self.H * self.W, 4)
                for k, cam in enumerate(cams):
                    _marshal.raster_visibility(cam, self.vertices, self.faces, self.near, flags, visibility, self.status)
                    rc = lib.rf_mesh_raster_taps(C.byref(cam), self.vertices.data_ptr(), V, self.faces.data_ptr(), T, visibility.data_ptr(), self.uvs.data_ptr(),
                                                 self.Ht, self.Wt, flags, per_view[k].data_ptr(), stream)
                    _lib.check(rc, "rf_mesh_raster_taps")
                _marshal.require_faces_in_range(self.status, V)
            else:
                self.taps[:, :2] = -1  # x0 = x1 = y0 = y1 = 0xFFFF: no hit
                self.taps[:, 2:] = 0
            self.mask = ((self.taps[:, 0] & 0xFFFF) != NO_TAP).view(self.N, self.H, self.W)
            self.offsets, self.entries, coverage = _transpose_taps(self.taps, self.Wt, texels)
            self.coverage = coverage.view(self.Ht, self.Wt)
        self.num_entries = int(self.entries.shape[0])

    def __call__(self, texture: Tensor) -> Tensor:
        if not torch.is_tensor(texture) or texture.device != self.device or texture.dtype != torch.float32 or tuple(texture.shape) != (self.Ht, self.Wt, 3):
            raise ValueError(f"the texture must be a float32 tensor of shape {(self.Ht, self.Wt, 3)} on {self.device}")
        return _Sample.apply(texture, self)

    def _forward(self, texture: Tensor) -> Tensor:
        colour = torch.empty((self.N, self.H, self.W, 3), dtype=torch.float32, device=self.device)
        if self.P and self.Ht and self.Wt:
            texture = texture.contiguous()
            rc = _lib.load().rf_texture_sample(self.taps.data_ptr(), self.P, texture.data_ptr(), self.Ht, self.Wt, self.background, 0, colour.data_ptr(),
                                               self.status.data_ptr(), _marshal.stream(self.device))
            _lib.check(rc, "rf_texture_sample")
        else:
            colour.fill_(self.background)
        return colour

    def _backward(self, grad_colour: Tensor) -> Tensor:
        if not self.num_entries:  # zero views, an empty mesh, or views that all look past it: no launch
            return torch.zeros((self.Ht, self.Wt, 3), dtype=torch.float32, device=self.device)
        grad = torch.empty((self.Ht, self.Wt, 3), dtype=torch.float32, device=self.device)
        grad_colour = grad_colour.to(torch.float32).contiguous()
        rc = _lib.load().rf_texture_sample_backward(grad_colour.data_ptr(), self.P, self.offsets.data_ptr(), self.entries.data_ptr(), self.num_entries, self.Ht, self.Wt,
                                                    self.long_segment, 0, grad.data_ptr(), self.status.data_ptr(), _marshal.stream(self.device))
        _lib.check(rc, "rf_texture_sample_backward")
        return grad


def tap_fields(taps: Tensor):
    """RFTextureTap records as int32 words [P, 4] -> (x0, x1, y0, y1 int64 [P], fx, fy float32 [P])"""
    xs, ys = taps[:, 0].to(torch.int64), taps[:, 1].to(torch.int64)
    frac = taps[:, 2:4].contiguous().view(torch.float32)
    return xs & 0xFFFF, (xs >> 16) & 0xFFFF, ys & 0xFFFF, (ys >> 16) & 0xFFFF, frac[:, 0], frac[:, 1]


def _transpose_taps(taps: Tensor, Wt: int, texels: int):
    """The transposed tap list of rf_texture_sample_backward: (offsets int64 [texels + 1], entries int32 [E, 2] = (pixel, weight bits),
    coverage int32 [texels]).  Every hit pixel gives four entries in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1) with the weights
    (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; a stable sort by texel keeps ties in ascending pixel order."""
    x0, x1, y0, y1, fx, fy = tap_fields(taps)
    pixel = torch.nonzero(x0 != NO_TAP).view(-1)
    x0, x1, y0, y1, fx, fy = (a[pixel] for a in (x0, x1, y0, y1, fx, fy))
    texel = torch.stack([y0 * Wt + x0, y0 * Wt + x1, y1 * Wt + x0, y1 * Wt + x1], dim=1).view(-1)
    gx, gy = 1.0 - fx, 1.0 - fy
    weight = torch.stack([gx * gy, fx * gy, gx * fy, fx * fy], dim=1).view(-1)
    texel, order = torch.sort(texel, stable=True)
    entries = torch.stack([pixel.to(torch.int32).repeat_interleave(4)[order], weight[order].view(torch.int32)], dim=1).contiguous()
    offsets = _marshal.segment_offsets(texel, texels)
    return offsets, entries, torch.diff(offsets).to(torch.int32)


def fit_texture(mesh: Mesh, bake: TextureBake, images, poses: Sequence, camera_intrinsics, *, alphas=None, background: float = 0.0, iterations: int = 200,
                lr: float = DEFAULT_LR, loss: str = "l2", dssim_weight: float = 0.0, near: float = 0.0, cull_backfaces: bool = False,
                callback: Optional[Callable[[int, Tensor], None]] = None) -> TextureFit:
    """Fit ``bake.texture`` to posed images by gradient descent through ``render_mesh``'s shading (``MeshTextureSampler``).  ``images``
    [N, H, W, 3] (or N [H, W, 3]), ``poses`` N CameraPose of one ``camera_intrinsics``; ``alphas`` None or [N, H, W] coverages m.  The
    prediction at a hit pixel is m s + (1 - m) ``background`` with s the sampled colour -- the image model of ``bake_texture_from_views``
    -- and the loss the mean over the hit pixels of all views and their channels of the squared (``loss="l2"``) or absolute
    (``"l1"``) residual.  With ``dssim_weight`` = lambda the loss is (1 - lambda) loss + lambda mean_views(1 - rf.ssim(frame, image)),
    the frame holding ``background`` at missed pixels ("same" padding below 11 pixels, as ``evaluate_mesh_against_field``).

    ``torch.optim.Adam`` on the texture; after each step the texels some pixel taps are clamped to [0, 1], and the texels no pixel
    taps keep the bake's bits exactly.  ``iterations=0`` returns the bake bit for bit.  ``callback(iteration, loss)`` is called with
    the device scalar of every iteration (reading it synchronises; nothing else does).  Returns TextureFit(bake, history, coverage):
    ``history`` [iterations] holds the loss before each step, on the device.  Two calls give the same bits.
    ValueError: as ``MeshTextureSampler``; counts or sizes of images, poses and alphas that do not match; ``iterations`` < 0; ``lr`` not
    positive and finite; ``dssim_weight`` outside [0, 1]; a ``loss`` other than "l1" and "l2"."""
    N = len(poses)
    if len(images) != N or (alphas is not None and len(alphas) != N):
        raise ValueError(f"{len(images)} images, {N} poses" + ("" if alphas is None else f", {len(alphas)} alphas") + ": the counts must match")
    iterations = _marshal.iteration_count(iterations)
    lr = _marshal.positive(lr, "lr")
    if loss not in ("l1", "l2"):
        raise ValueError(f"loss must be 'l1' or 'l2', got {loss!r}")
    dssim_weight = float(dssim_weight)
    if not 0.0 <= dssim_weight <= 1.0:
        raise ValueError(f"dssim_weight must be in [0, 1], got {dssim_weight!r}")
    H, W = int(camera_intrinsics[0]), int(camera_intrinsics[1])
    images = _view_chunk(images, 0, N, 3, "images") if N else torch.zeros((0, H, W, 3))
    if tuple(images.shape) != (N, H, W, 3):
        raise ValueError(f"the images of {N} views of {H} x {W} pixels must have shape {(N, H, W, 3)}, got {tuple(images.shape)}")
    if alphas is not None:
        alphas = _view_chunk(alphas, 0, N, None, "alphas") if N else torch.zeros((0, H, W))
        if tuple(alphas.shape) != (N, H, W):
            raise ValueError(f"the alphas of {N} views of {H} x {W} pixels must have shape {(N, H, W)}, got {tuple(alphas.shape)}")
    dev = bake.texture.device if torch.is_tensor(bake.texture) else None
    history = torch.zeros(iterations, dtype=torch.float32, device=dev)
    sampler = MeshTextureSampler(mesh, bake, poses, camera_intrinsics, near=near, cull_backfaces=cull_backfaces, background=background)
    if not iterations or not sampler.num_entries:  # (no pixel taps any texel: every gradient is zero)
        return TextureFit(bake, history, sampler.coverage)
    start = bake.texture.detach().contiguous()
    images = images.detach().to(dev, torch.float32).contiguous()
    mask = sampler.mask[..., None]
    m = None if alphas is None else alphas.detach().to(dev, torch.float32)[..., None]
    covered = (sampler.coverage > 0)[..., None]
    terms = 3.0 * float(sampler.num_entries // 4)
    padding = "valid" if min(H, W) >= 11 else "same"
    texture = start.clone().requires_grad_(True)
    optimiser = torch.optim.Adam([texture], lr=lr)
    losses = []
    for it in range(iterations):
        optimiser.zero_grad(set_to_none=True)
        sampled = sampler(texture)
        pred = sampled if m is None else m * sampled + (1.0 - m) * sampler.background
        residual = torch.where(mask, pred - images, torch.zeros((), dtype=torch.float32, device=dev))
        value = (residual * residual if loss == "l2" else residual.abs()).sum() / terms
        if dssim_weight > 0.0:
            frame = torch.where(mask, pred, torch.full((), sampler.background, dtype=torch.float32, device=dev))
            dssim = torch.stack([1.0 - ssim(frame[k], images[k], padding=padding) for k in range(N)]).mean()
            value = (1.0 - dssim_weight) * value + dssim_weight * dssim
        value.backward()
        optimiser.step()
        with torch.no_grad():
            texture.copy_(torch.where(covered, texture.clamp(0.0, 1.0), start))
        losses.append(value.detach())
        if callback is not None:
            callback(it, losses[-1])
    history = torch.stack(losses).to(torch.float32)
    return TextureFit(bake._replace(texture=texture.detach()), history, sampler.coverage)


def fit_texture_to_field_views(mesh: Mesh, bake: TextureBake, vol_mod, poses: Sequence, camera_intrinsics, *, render_overrides: Optional[dict] = None,
                               **kw) -> TextureFit:
    """``fit_texture`` against the field's own renders, obtained exactly as ``bake_texture_from_field_views`` obtains them: every pose
    is rendered by ``vol_mod.render`` (``render_overrides`` are passed on), the accumulated weight of ``vol_mod.render_geometry`` is the
    view's alpha plane and the model's background the background.  The other keywords are those of ``fit_texture``."""
    overrides = dict(render_overrides or {})
    cfg = getattr(vol_mod, "render_config", None)
    white = bool(overrides.get("white_bkgd", getattr(cfg, "white_bkgd", False)))
    for given in ("alphas", "background"):
        if given in kw:
            raise TypeError(f"fit_texture_to_field_views takes the {given} from the field")
    geometry_overrides = {k: v for k, v in overrides.items() if k != "white_bkgd"}
    dev = bake.texture.device
    colours, accs = [], []
    with torch.no_grad():
        for pose in poses:
            colours.append(vol_mod.render(pose, camera_intrinsics, **overrides).colour.to(dev, torch.float32))
            accs.append(vol_mod.render_geometry(pose, camera_intrinsics, **geometry_overrides).extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].to(dev, torch.float32))
    return fit_texture(mesh, bake, colours, list(poses), camera_intrinsics, alphas=accs, background=1.0 if white else 0.0, **kw)
