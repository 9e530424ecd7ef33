"""CPU: the float32 replay of tests/segment_sum_model.py against the float64 sums and bounds of the crafted texture list, against a
plain sequential float32 sum where nothing is long, and what the crafted lists of the GPU test cover.  No GPU needed."""
import numpy as np
import pytest

from tests import segment_sum_model as ssm
from tests import texture_fit_model as tfm


@pytest.mark.parametrize("threshold", ssm.THRESHOLDS)
def test_replay_lies_within_the_float64_bound_of_the_crafted_texture_list(threshold):
    offsets, pixel, weight, grad_colour = tfm.crafted_list()
    ref, bound = tfm.crafted_reference(offsets, pixel, weight, grad_colour)
    got = ssm.replay(offsets, ssm.texture_terms(pixel, weight, grad_colour), threshold)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert (got[np.diff(offsets) == 0] == 0.0).all()


def test_replay_of_short_segments_is_the_sequential_sum_and_the_tree_is_another_order():
    offsets, pixel, weight, grad_colour = tfm.crafted_list()
    terms = ssm.texture_terms(pixel, weight, grad_colour)
    lengths = np.diff(offsets)
    sequential = np.zeros((len(lengths), 3), np.float32)
    np.add.at(sequential, np.repeat(np.arange(len(lengths)), lengths), terms)  # (unbuffered: one float32 addition after another)
    assert np.array_equal(ssm.replay(offsets, terms, 1 << 30), sequential)
    tree = ssm.replay(offsets, terms, 1)
    assert np.array_equal(tree[lengths <= 1], sequential[lengths <= 1]) and not np.array_equal(tree, sequential)
    # a 2^24 and 64 ones: one after another every one is lost; lane 0 loses its own (entry 64) and lane 32's in the tree's first step;
    # the other 62 arrive as 2, 4, 8, 16 and 32
    one_long = np.concatenate([[2.0 ** 24], np.ones(64)]).astype(np.float32)[:, None]
    assert ssm.replay(np.array([0, 65]), one_long, 1 << 30)[0, 0] == 2.0 ** 24 + 0.0
    assert ssm.replay(np.array([0, 65]), one_long, 16)[0, 0] == 2.0 ** 24 + 62.0


def test_what_the_crafted_lists_cover():
    default = 16
    assert not ssm.covers(tfm.CRAFTED_LENGTHS, default)  # (nothing past the first wavefront: why the mesh case extends it)
    assert ssm.FACE_LENGTHS[:len(tfm.CRAFTED_LENGTHS)] == tfm.CRAFTED_LENGTHS
    for threshold in (1, default, 64):
        assert ssm.covers(ssm.FACE_LENGTHS, threshold) and ssm.covers(ssm.VERTEX_LENGTHS, threshold), threshold
    records, hit_pixels, face_offsets, corner_slots, vertex_offsets = ssm.crafted_mesh_lists()
    T, V = len(ssm.FACE_LENGTHS), len(ssm.VERTEX_LENGTHS)
    assert len(hit_pixels) == face_offsets[-1] <= len(records) and 0 <= hit_pixels.min() and hit_pixels.max() < ssm.NUM_RECORDS
    assert sorted(corner_slots.tolist()) == list(range(3 * T)) and vertex_offsets[-1] == 3 * T and len(vertex_offsets) == V + 1
    face_grads, vertex_grads = ssm.replay_mesh(records, hit_pixels, face_offsets, corner_slots, vertex_offsets, default)
    assert face_grads.shape == (T, 9) and vertex_grads.shape == (V, 3)
    assert (face_grads[np.array(ssm.FACE_LENGTHS) == 0] == 0.0).all() and (vertex_grads[np.array(ssm.VERTEX_LENGTHS) == 0] == 0.0).all()
    # within a float64 sum's rounding bound (n + 6 roundings of the sum of magnitudes: sequential is n, the tree n / 64 + 6)
    exact = np.zeros((T, 9))
    mag = np.zeros((T, 9))
    rows = records[hit_pixels].astype(np.float64)
    np.add.at(exact, np.repeat(np.arange(T), ssm.FACE_LENGTHS), rows)
    np.add.at(mag, np.repeat(np.arange(T), ssm.FACE_LENGTHS), np.abs(rows))
    bound = (np.array(ssm.FACE_LENGTHS)[:, None] + 6) * 2.0 ** -24 * mag
    assert (np.abs(face_grads.astype(np.float64) - exact) <= bound).all()
