"""Golden ray / pose gradients of the reference -- runs ONLY in the build container, where /root/reference exists.

Imports the reference (akanimax/thr3ed_atom) as a Python package, the way oracle/gen_golden.py does, and differentiates its own
cast_rays -> render_sh_voxel_grid -> L1(colour) with respect to the camera pose (R, t) and the flat rays.  Only arrays are stored:
tests/golden/g16_ray_pose_grads.npz, one set per case of tests/ray_grads_common.GOLDEN_CASES (grid, sampling, background).  The grids
and targets are regenerated from tests/helpers.py by the tests, so only the gradients (and the case parameters) are kept.

    python tools/gen_golden_ray_grads.py

The reference imports ``easydict`` for one type annotation; a three-line stand-in is registered in THIS process only.
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

_easydict = types.ModuleType("easydict")
_easydict.EasyDict = dict
sys.modules.setdefault("easydict", _easydict)

from tests.helpers import GOLDEN_DIR  # noqa: E402
from tests.ray_grads_common import GOLDEN_CASES, golden_inputs  # noqa: E402

from thre3d_atom.rendering.volumetric.render_interface import Rays  # noqa: E402
from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays  # noqa: E402
from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize  # noqa: E402
from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, CameraPose  # noqa: E402

META = np.array([f"torch={torch.__version__}", f"numpy={np.__version__}", "reference=akanimax/thr3ed_atom@v1"])


def main():
    out = {}
    for i, case in enumerate(GOLDEN_CASES):
        inp = golden_inputs(case)
        grid = VoxelGrid(densities=inp["dens"].clone(), features=inp["feat"].clone(), voxel_size=VoxelSize(*inp["voxel"]),
                         grid_location=VoxelGridLocation(0.0, 0.0, 0.0), tunable=False, density_preactivation=torch.nn.Identity(),
                         density_postactivation=torch.nn.ReLU(), expected_density_scale=inp["rho"])
        R = inp["rotation"].clone().requires_grad_(True)
        t = inp["translation"].clone().requires_grad_(True)
        H, W, f = inp["intrinsics"]
        rays = flatten_rays(cast_rays(CameraIntrinsics(H, W, f), CameraPose(R, t), torch.device("cpu")))
        rays.origins.retain_grad()
        rays.directions.retain_grad()
        near, far = inp["bounds"]
        cfg = SHVoxGridRenderConfig(inp["num_samples"], CameraBounds(near, far), perturb_sampled_points=False,
                                    optimized_sampling=case["aabb"], white_bkgd=case["white"])
        colour = render_sh_voxel_grid(grid, Rays(rays.origins, rays.directions), cfg).colour
        torch.nn.functional.l1_loss(colour, inp["target"]).backward()
        for k, v in (("R_grad", R.grad), ("t_grad", t.grad), ("origins_grad", rays.origins.grad), ("directions_grad", rays.directions.grad),
                     ("colour", colour)):
            out[f"c{i}_{k}"] = v.detach().numpy()
        print(f"case {i} {case}: max |dL/dR| {R.grad.abs().max().item():.4g}, max |dL/dt| {t.grad.abs().max().item():.4g}")
    path = os.path.join(GOLDEN_DIR, "g16_ray_pose_grads.npz")
    np.savez_compressed(path, meta=META, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
