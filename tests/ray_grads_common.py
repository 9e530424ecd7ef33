"""Shared inputs of the ray / pose gradient tests: the cases of the golden fixture g16_ray_pose_grads.npz (written from the reference
by tools/gen_golden_ray_grads.py) and the oracle's differentiable cast_rays -> render -> L1."""
import numpy as np
import torch

from oracle import relu_field_oracle as orc
from tests.helpers import hash_uniform, hotdog_like_camera, sparse_scene_grid

# a 16^3 / F = 27 sparse scene and the 5 x 6 x 7 anisotropic grid, both sampling modes, both backgrounds
GOLDEN_CASES = [
    dict(dims=dims, aabb=aabb, white=white)
    for dims in ((16, 16, 16), (5, 6, 7))
    for aabb in (False, True)
    for white in (False, True)
]


def golden_inputs(case):
    dims = case["dims"]
    dens, feat = sparse_scene_grid(dims, 27, 160 + dims[0])
    voxel = (3.0 / 16,) * 3 if dims == (16, 16, 16) else (0.6, 0.5, 0.45)
    cam = hotdog_like_camera()
    H = W = 12
    yaw, pitch = 30.0, -30.0
    p, y = np.deg2rad(pitch), np.deg2rad(yaw)
    # pose_spherical (imaging_utils.py:185-191) in float32, built here so that the reference and this package start from the same bits
    lift = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, cam["radius"]], [0, 0, 0, 1]], np.float32)
    tilt = np.array([[1, 0, 0, 0], [0, np.cos(p), -np.sin(p), 0], [0, np.sin(p), np.cos(p), 0], [0, 0, 0, 1]], np.float32)
    spin = np.array([[np.cos(y), -np.sin(y), 0, 0], [np.sin(y), np.cos(y), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    c2w = spin @ (tilt @ lift)
    return {
        "dens": dens, "feat": feat, "voxel": voxel, "rho": 10.0, "num_samples": 32, "intrinsics": (H, W, 14.0),
        "bounds": (float(np.float32(cam["near"])), float(np.float32(cam["far"]))),
        "rotation": torch.from_numpy(np.ascontiguousarray(c2w[:3, :3])), "translation": torch.from_numpy(np.ascontiguousarray(c2w[:3, 3:])),
        "target": torch.from_numpy(hash_uniform((H * W, 3), 170 + dims[0], 0.0, 1.0)),
    }


def oracle_pose_grads(inp, aabb_sampling, white, dtype):
    """(dL/dR, dL/dt, dL/d origins, dL/d directions, colour) of the oracle's cast_rays -> render -> L1, in ``dtype``."""
    H, W, focal = inp["intrinsics"]
    R = inp["rotation"].to(dtype).clone().requires_grad_(True)
    t = inp["translation"].to(dtype).clone().requires_grad_(True)
    xs = ((torch.arange(W, dtype=dtype) + 0.5) - W * 0.5) / focal
    ys = -(((torch.arange(H, dtype=dtype) + 0.5) - H * 0.5) / focal)
    cx, cy = xs[None, :].expand(H, W).reshape(-1), ys[:, None].expand(H, W).reshape(-1)
    dirs = torch.stack([(R[a, 0] * cx + R[a, 1] * cy) + R[a, 2] * -1.0 for a in range(3)], dim=-1)  # the kernel's / oracle's order
    origins = t.reshape(1, 3).expand(H * W, 3)
    dirs.retain_grad()
    origins.retain_grad()
    near, far = inp["bounds"]
    aabb = orc.make_aabb(inp["dens"].shape[:3], inp["voxel"])
    out = orc.render(inp["dens"].to(dtype), inp["feat"].to(dtype), origins, dirs, aabb, near, far, inp["num_samples"], inp["rho"], "relu",
                     white_bkgd=white, optimized_sampling=aabb_sampling)
    torch.nn.functional.l1_loss(out["colour"], inp["target"].to(dtype)).backward()
    return R.grad, t.grad, origins.grad, dirs.grad, out["colour"].detach()
