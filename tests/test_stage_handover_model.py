"""The conditions of tests/test_hip_stage_handover.py on the CPU: the exact comparisons of the chain cannot flip on rounding, and the
chain decides what the test says it decides."""
import numpy as np

from tests import node_weights_model as nm
from tests import resample_model as rm
from tests import stage_handover_model as sh


def test_no_comparison_of_the_chain_sits_on_a_rounding():
    c = sh.chain()
    gap = np.abs(c["M"] - nm.SCENE_TAU).min()
    print(f"handover conditions: smallest |M64 - tau| = {gap:.3e} (bar {sh.M_BAR:.0e}); kept {c['counts'][0]}, pruned {c['counts'][1]}")
    assert gap > sh.M_BAR  # no model value of M within the kernel's bar of tau: float32 and float64 keep the same nodes
    # no node's activated density within 1e-6 relative of the tighten threshold (0: relative to the unit the activation works in) --
    # a node passes by far or is an exact zero / a negative (sigma = +0 under the ReLU)
    for dens in (nm.scene_grid()[0].numpy(), c["pruned_densities"]):
        sigma = rm.activated(dens, nm.SCENE_RHO, "relu")
        assert ((sigma == 0.0) | (np.abs(sigma - sh.TIGHTEN_THRESHOLD) > 1e-6 * np.maximum(1.0, sh.TIGHTEN_THRESHOLD))).all()
    assert not c["outside"].any()  # every destination node lies inside the cropped box


def test_the_order_of_prune_and_tighten_decides_the_box():
    c = sh.chain()
    shell, blob, speck = nm.scene_regions()
    assert c["box"][:2] == ((5, 5, 5), (18, 18, 18)) and c["box"][2] == int(shell.sum())  # the speck and the blob are gone
    assert (c["first"], c["last"]) == ([4, 4, 4], [19, 19, 19])
    assert c["box_unpruned"][0] == (2, 5, 5) and c["box_unpruned"][1] == (18, 18, 18)  # without pruning the speck's node sets x
    assert not c["keep"][blob].any() and not c["keep"][speck].any() and (c["pruned_densities"][shell] == np.float32(nm.SHELL_DENSITY)).all()
    assert c["new_dims"] == (20, 20, 20) and c["crop_dims"] == (16, 16, 16)
