"""The reference the GPU tests of rf_label_components compare against (tests/components_model.py), checked on its own: hand-written
cases, scipy.ndimage.label where scipy is installed, the cell property that makes 26-connectivity the default, and the keep rule."""
import numpy as np
import pytest

from tests import components_model as cm
from tests.helpers import hash_uniform


def count(mask, connectivity):
    return len(cm.ranked(cm.label(mask, connectivity))[0])


def test_two_nodes_sharing_only_an_edge():
    mask = np.zeros((3, 3, 3), dtype=bool)
    mask[0, 0, 1] = mask[0, 1, 2] = True
    assert [count(mask, c) for c in (6, 18, 26)] == [2, 1, 1]
    labels = cm.label(mask, 18)
    assert labels[0, 0, 1] == labels[0, 1, 2] == 1 and (labels[~mask] == -1).all()
    assert cm.sizes_of(labels)[1] == 2 and cm.sizes_of(labels).sum() == 2


def test_two_nodes_sharing_only_a_corner():
    mask = np.zeros((3, 3, 3), dtype=bool)
    mask[0, 2, 0] = mask[1, 1, 1] = True
    assert [count(mask, c) for c in (6, 18, 26)] == [2, 2, 1]
    assert cm.label(mask, 26)[1, 1, 1] == 6  # the smaller plain index, (0 * 3 + 2) * 3 + 0


def test_checkerboard():
    x, y, z = np.indices((4, 5, 6))
    mask = (x + y + z) % 2 == 0
    assert count(mask, 6) == mask.sum()  # no two occupied nodes share a face
    assert count(mask, 18) == 1 and count(mask, 26) == 1
    labels = cm.label(mask, 6)
    assert (labels.reshape(-1)[mask.reshape(-1)] == np.flatnonzero(mask.reshape(-1))).all()  # every node its own root


def test_empty_full_and_degenerate_axes():
    assert (cm.label(np.zeros((2, 3, 4), dtype=bool), 26) == -1).all()
    full = cm.label(np.ones((2, 3, 4), dtype=bool), 6)
    assert (full == 0).all() and cm.sizes_of(full)[0] == 24
    line = np.array([1, 1, 0, 1], dtype=bool).reshape(1, 1, 4)
    assert cm.label(line, 26).reshape(-1).tolist() == [0, 0, -1, 3]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_against_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, cm.MAX_L1[connectivity])
    for seed, dims, p in ((1, (7, 6, 9), 0.2), (2, (9, 8, 17), 0.31), (3, (5, 11, 4), 0.6)):
        mask = hash_uniform(dims, seed, 0.0, 1.0) < p
        theirs, n = ndimage.label(mask, structure=structure)
        # canonicalise scipy's 1..n to the smallest plain index of each piece
        first = np.full(n + 1, -1, dtype=np.int64)
        flat = theirs.reshape(-1)
        for i in np.flatnonzero(flat)[::-1]:
            first[flat[i]] = i
        want = np.where(theirs > 0, first[theirs], -1).astype(np.int32)
        got = cm.label(mask, connectivity)
        assert np.array_equal(got, want)
        assert np.array_equal(cm.sizes_of(got), np.bincount(want[want >= 0], minlength=mask.size))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.6])
def test_no_cell_mixes_a_kept_and_a_removed_component_under_26(p):
    """Two occupied corners of one cell differ by at most 1 on every axis: 26-neighbours, hence one component.  So whatever set of
    components is kept, no cell has a corner in a kept one and a corner in a removed one -- and under 6 or 18 such cells exist."""
    dims = (9, 10, 11)
    mixed = {6: 0, 18: 0, 26: 0}
    for seed in (11, 12, 13):
        mask = hash_uniform(dims, seed, 0.0, 1.0) < p
        for connectivity in (6, 18, 26):
            labels = cm.label(mask, connectivity)
            roots, sizes = cm.ranked(labels)
            for keep_roots in (roots[:1], roots[::2], roots[sizes >= 3]):
                mixed[connectivity] += cm.cells_mixing_kept_and_removed(labels, keep_roots)
    assert mixed[26] == 0
    assert mixed[6] > 0  # (the check can see a violation)


def test_a_cell_can_mix_under_6_and_18():
    mask = np.zeros((2, 2, 2), dtype=bool)
    mask[0, 0, 0] = mask[1, 1, 1] = True  # two corners of the one cell that share only a corner
    for connectivity, want in ((6, 1), (18, 1), (26, 0)):
        labels = cm.label(mask, connectivity)
        assert cm.cells_mixing_kept_and_removed(labels, cm.ranked(labels)[0][:1]) == want


def test_keep_rule_and_ties():
    mask = np.zeros((1, 1, 12), dtype=bool)
    mask[0, 0, [0, 1, 3, 4, 6, 8, 9, 10]] = True  # pieces: root 0 (2 nodes), 3 (2), 6 (1), 8 (3)
    labels = cm.label(mask, 6)
    roots, sizes = cm.ranked(labels)
    assert roots.tolist() == [8, 0, 3, 6] and sizes.tolist() == [3, 2, 2, 1]  # equal sizes: the smaller root first
    assert cm.kept(sizes, keep_largest=2).tolist() == [True, True, False, False]  # root 0 wins the tie against root 3
    assert cm.kept(sizes, min_nodes=2).tolist() == [True, True, True, False]
    assert cm.kept(sizes, min_nodes=3, keep_largest=2).tolist() == [True, False, False, False]
    assert cm.kept(sizes, min_nodes=4, keep_largest=1).tolist() == [False] * 4
    dens = np.where(mask, 0.5, -0.25).astype(np.float32)[..., None]
    after, stats = cm.remove(dens, labels, "relu", keep_largest=2)
    assert stats == (4, 2, 5, 3)
    assert after[0, 0, :, 0].tolist() == [0.5, 0.5, -0.25, 0.0, 0.0, -0.25, 0.0, -0.25, 0.5, 0.5, 0.5, -0.25]
    # |.|: negative raw values are occupied, and 0 is the one fill
    labels_abs = cm.label(cm.occupied(dens, 2.0, "abs", 0.75), 6)  # |D| * 2 > 0.75: only the 0.5 nodes
    assert np.array_equal(labels_abs, labels)
    assert cm.remove(dens, labels_abs, "abs", min_nodes=3)[0][0, 0, :, 0].tolist() == [0.0, 0.0, -0.25, 0.0, 0.0, -0.25, 0.0, -0.25, 0.5, 0.5, 0.5, -0.25]
    # a fill above a density never raises it
    assert cm.remove(dens, labels, "identity", min_nodes=3, fill=0.75)[0][0, 0, :2, 0].tolist() == [0.5, 0.5]


def test_occupancy_is_strict_and_float32():
    d = np.array([0.1, 0.3, -0.3, 0.0], dtype=np.float32).reshape(1, 1, 4)
    tau = float(np.float32(0.3) * np.float32(3.0))  # sigma of node 1, exactly
    assert cm.occupied(d, 3.0, "relu", tau).reshape(-1).tolist() == [False, False, False, False]
    assert cm.occupied(d, 3.0, "relu", np.nextafter(np.float32(tau), np.float32(0.0))).reshape(-1).tolist() == [False, True, False, False]
    assert cm.occupied(d, 3.0, "abs", 0.5).reshape(-1).tolist() == [False, True, True, False]
    assert cm.occupied(d, 1.0, "identity", 0.0).reshape(-1).tolist() == [True, True, False, False]
    assert cm.occupied(d, 1.0, "softplus", 0.7).reshape(-1).tolist() == [True, True, False, False]  # softplus(0) = ln 2 = 0.693
