"""Golden G14: what integration/renderers_hip.py relies on in the REFERENCE package, recorded as data -- run once against a checkout of
the reference; the binding's CPU test (tests/test_integration_binding.py) then needs no reference at all.

    python oracle/gen_golden_binding.py <reference checkout>      ->  tests/golden/g14_binding_api.npz

    grid_attributes    names of everything a reference VoxelGrid instance holds (instance attributes, parameters, submodules)
                       and of the properties of its class
    grid_aabb          float64 [3, 2]: its AABB for dims 4 x 5 x 6, VoxelSize(0.1, 0.2, 0.3), VoxelGridLocation(0.5, 0.0, -0.25)
    grid_points        float32 [N, 3] world points in and around that AABB ...
    grid_normalized    ... and the reference's own VoxelGrid._normalize_points of them (adjust_dynamic_range, slack=True)
    rays_fields / render_out_fields   the dataclass fields of render_interface.Rays / RenderOut
    extra_disparity / extra_accumulated_weights   the keys of utils/constants.py the binding fills in RenderOut.extra
"""
import dataclasses
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def main(reference: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.abspath(reference))
    _easydict = types.ModuleType("easydict")  # imported by the reference for a type annotation only
    _easydict.EasyDict = dict
    sys.modules.setdefault("easydict", _easydict)

    from tests.helpers import GOLDEN_DIR, hash_uniform
    from thre3d_atom.rendering.volumetric.render_interface import Rays, RenderOut
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize
    from thre3d_atom.utils.constants import EXTRA_ACCUMULATED_WEIGHTS, EXTRA_DISPARITY

    g = VoxelGrid(torch.zeros(4, 5, 6, 1), torch.zeros(4, 5, 6, 27), VoxelSize(0.1, 0.2, 0.3), VoxelGridLocation(0.5, 0.0, -0.25),
                  density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=7.0, tunable=True)
    module_own = set(vars(torch.nn.Module()))
    names = (set(vars(g)) - module_own) | set(g._parameters) | set(g._modules)
    names |= {n for n in dir(type(g)) if isinstance(getattr(type(g), n, None), property)}
    aabb = np.array([[float(lo), float(hi)] for lo, hi in g.aabb], dtype=np.float64)
    lo, hi = aabb[:, 0], aabb[:, 1]
    u = hash_uniform((64, 3), 1401, -0.25, 1.25).astype(np.float64)
    points = np.concatenate([u * (hi - lo) + lo, aabb.T]).astype(np.float32)  # (the two corners exactly)
    with torch.no_grad():
        normalized = g._normalize_points(torch.from_numpy(points)).numpy()
    out = os.path.join(GOLDEN_DIR, "g14_binding_api.npz")
    np.savez(
        out,
        grid_attributes=np.array(sorted(names)),
        grid_aabb=aabb,
        grid_points=points,
        grid_normalized=normalized.astype(np.float32),
        rays_fields=np.array([f.name for f in dataclasses.fields(Rays)]),
        render_out_fields=np.array([f.name for f in dataclasses.fields(RenderOut)]),
        extra_disparity=np.array(EXTRA_DISPARITY),
        extra_accumulated_weights=np.array(EXTRA_ACCUMULATED_WEIGHTS),
    )
    print(f"wrote {out}: {len(names)} grid names, {len(points)} points")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python oracle/gen_golden_binding.py <reference checkout>")
    main(sys.argv[1])
