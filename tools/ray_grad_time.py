#!/usr/bin/env python
"""Time of the ray adjoint (rf_render_backward_rays) next to the forward render of the same batch, and of one
refine_camera_pose iteration.  HIP events around each launch, three warm-up calls, median of N timed calls; one JSON line each.

Batch: 16384 rays x 256 samples through a 128^3 SH-degree-2 sparse scene (tests.helpers.sparse_scene_grid), split storage, the
AABB sampler, colour + depth upstream gradients.  The pose iteration: cast_rays -> render_rays -> L1 -> backward -> Adam at 100 x 100
pixels, 128 samples per ray, frozen field.

    python tools/ray_grad_time.py [timed calls]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd import ops  # noqa: E402
from tests.helpers import hash_uniform, hotdog_like_camera, sparse_scene_grid  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, N, S = 128, 16384, 256
dens, feat = sparse_scene_grid((G, G, G), 27, 3)
grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                    density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False, storage="split")
cam = hotdog_like_camera()
near, far = float(np.float32(cam["near"])), float(np.float32(cam["far"]))
pose = rf.pose_spherical(30.0, -30.0, cam["radius"])
rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(128, 128, 140.0), pose, dev))
o, d = rays.origins[:N].contiguous(), rays.directions[:N].contiguous()
flags = ops.render_flags(True, False, True, False)
gc = torch.from_numpy(hash_uniform((N, 3), 1)).to(dev)
gdp = torch.from_numpy(hash_uniform((N, 1), 2)).to(dev)


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


fwd_ms = timed(lambda: ops.render_forward_raw(grid, o, d, None, S, near, far, flags, save=False))
fwd_save_ms = timed(lambda: ops.render_forward_raw(grid, o, d, None, S, near, far, flags, save=True))
caches = ops.render_forward_raw(grid, o, d, None, S, near, far, flags, save=True)[4]
bwd_ms = timed(lambda: ops.render_backward_rays_raw(grid, o, d, None, S, near, far, flags, caches, gc, gdp, None))
print(json.dumps({"what": "rf_render_backward_rays", "grid": G, "sh_degree": 2, "rays": N, "samples": S, "forward_ms": round(fwd_ms[0], 4),
                  "forward_save_ms": round(fwd_save_ms[0], 4), "backward_rays_ms": round(bwd_ms[0], 4), "backward_rays_min_ms": round(bwd_ms[1], 4),
                  "ratio_to_forward": round(bwd_ms[0] / fwd_ms[0], 2)}), flush=True)

cfg = rf.SHVoxGridRenderConfig(128, rf.CameraBounds(near, far), perturb_sampled_points=False, white_bkgd=True, optimized_sampling=True)
model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
intr = rf.CameraIntrinsics(100, 100, 110.0)
target = torch.from_numpy(hash_uniform((100, 100, 3), 4, 0.0, 1.0)).to(dev)
it_ms = timed(lambda: rf.refine_camera_pose(model, target, intr, pose, num_iterations=1))
print(json.dumps({"what": "refine_camera_pose iteration", "pixels": "100x100", "samples": 128, "median_ms": round(it_ms[0], 3),
                  "min_ms": round(it_ms[1], 3)}), flush=True)
