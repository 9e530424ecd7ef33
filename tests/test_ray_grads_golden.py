"""The oracle's ray and pose gradients against the reference's own (tests/golden/g16_ray_pose_grads.npz, written by
tools/gen_golden_ray_grads.py from the reference's cast_rays -> render_sh_voxel_grid -> L1 autograd).  CPU only."""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.ray_grads_common import GOLDEN_CASES, golden_inputs, oracle_pose_grads

KEYS = ("R_grad", "t_grad", "origins_grad", "directions_grad", "colour")


@pytest.mark.parametrize("i", range(len(GOLDEN_CASES)))
def test_oracle_ray_and_pose_grads_match_reference(i):
    g = load_golden("g16_ray_pose_grads.npz")
    case = GOLDEN_CASES[i]
    ours = oracle_pose_grads(golden_inputs(case), case["aabb"], case["white"], torch.float32)
    for key, mine in zip(KEYS, ours):
        ref = torch.from_numpy(g[f"c{i}_{key}"])
        err = (mine - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"case {i} {key}: max err {err:.3e} of max {scale:.3e}")
        assert mine.shape == ref.shape
        assert err <= 1e-5 * scale + 1e-9, (key, err, scale)
    assert np.abs(g[f"c{i}_R_grad"]).max() > 0 and np.abs(g[f"c{i}_t_grad"]).max() > 0
