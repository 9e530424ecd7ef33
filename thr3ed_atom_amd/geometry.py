"""Consumers of the geometry pass (ops.render_geometry / VolumetricModel.render_geometry): the normal map of a frame as an image,
and an oriented, coloured point cloud back-projected from the quantile depth of posed views."""
from typing import Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .constants import EXTRA_ACCUMULATED_WEIGHTS, EXTRA_NORMALS
from .mesh import to8b


def normal_map_image(normals, acc, background=(0.0, 0.0, 0.0), min_acc: float = 0.5) -> np.ndarray:
    """uint8 [H, W, 3] of a frame's composited normals [H, W, 3] and accumulated weights [H, W, 1]:
    to8b((N / max(|N|, 1e-10)) * 0.5 + 0.5), pixels with acc < ``min_acc`` set to ``background`` (a colour in [0, 1])."""
    n = np.asarray(normals.detach().cpu().numpy() if isinstance(normals, Tensor) else normals, dtype=np.float32)
    a = np.asarray(acc.detach().cpu().numpy() if isinstance(acc, Tensor) else acc, dtype=np.float32).reshape(n.shape[:-1])
    unit = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-10)
    image = unit * 0.5 + 0.5
    image[a < min_acc] = np.asarray(background, dtype=np.float32)
    return to8b(image)


def back_project_points(model, poses: Sequence, intrinsics, *, quantile: float = 0.5, min_acc: float = 0.5, stride: int = 1) -> Tuple[Tensor, Tensor, Tensor]:
    """An oriented, coloured point cloud of a VolumetricModel from posed views: per view one geometry pass and one ordinary render;
    every ``stride``-th pixel (rows and columns) whose quantile depth z_q is non-zero and whose accumulated weight is at least
    ``min_acc`` gives the point o + d z_q, the renormalised composited normal and the rendered colour.  Both passes sample without
    jitter, whatever the model's config says, so that the depth and the colour of a pixel come from the same samples.
    Returns (points [M, 3], normals [M, 3], colours [M, 3]) on the model's device, views concatenated in order.  No gradient."""
    from .volumetric_model import cast_rays

    if isinstance(stride, bool) or int(stride) < 1:
        raise ValueError(f"stride must be a positive integer, got {stride!r}")
    step = int(stride)
    points, normals, colours = [], [], []
    with torch.no_grad():
        for pose in poses:
            # (without jitter in both passes: with it each would draw a key of its own, and depth and colour would come from different samples)
            geo = model.render_geometry(pose, intrinsics, quantile=quantile, perturb_sampled_points=False)
            colour = model.render(pose, intrinsics, perturb_sampled_points=False).colour
            rays = cast_rays(intrinsics, pose, geo.depth.device)
            z = geo.depth[::step, ::step].reshape(-1, 1)
            acc = geo.extra[EXTRA_ACCUMULATED_WEIGHTS][::step, ::step].reshape(-1)
            n = geo.extra[EXTRA_NORMALS][::step, ::step].reshape(-1, 3)
            keep = (z[:, 0] != 0) & (acc >= min_acc)
            o, d = rays.origins[::step, ::step].reshape(-1, 3), rays.directions[::step, ::step].reshape(-1, 3)
            points.append((o + d * z)[keep])
            normals.append((n / n.norm(dim=-1, keepdim=True).clamp_min(1e-10))[keep])
            colours.append(colour[::step, ::step].reshape(-1, 3)[keep])
    if not points:
        dev = model.device
        return tuple(torch.zeros((0, 3), dtype=torch.float32, device=dev) for _ in range(3))
    return torch.cat(points), torch.cat(normals), torch.cat(colours)


def write_point_cloud_ply(points, normals, colours, path: str) -> None:
    """Binary little-endian PLY of a point cloud: vertex x y z, nx ny nz (float), red green blue (uchar, to8b of colours in [0, 1]);
    no face element.  ``normals`` / ``colours`` may be None (written as 0 / 255)."""
    as_np = lambda t: np.asarray(t.detach().cpu().numpy() if isinstance(t, Tensor) else t)  # noqa: E731
    v = as_np(points).astype("<f4").reshape(-1, 3)
    n = len(v)
    nrm = np.zeros((n, 3), "<f4") if normals is None else as_np(normals).astype("<f4").reshape(-1, 3)
    rgb = np.full((n, 3), 255, np.uint8) if colours is None else to8b(as_np(colours).reshape(-1, 3))
    if len(nrm) != n or len(rgb) != n:
        raise ValueError("points, normals and colours must have one row per point")
    vdt = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    vert = np.empty(n, vdt)
    vert["p"], vert["n"], vert["c"] = v, nrm, rgb
    header = (
        "ply\nformat binary_little_endian 1.0\n"
        f"element vertex {n}\n"
        "property float x\nproperty float y\nproperty float z\n"
        "property float nx\nproperty float ny\nproperty float nz\n"
        "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        "end_header\n"
    )
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
