"""A float32 replay of segment_sum (thr3ed_atom_amd/csrc/segment_sum.h), the segmented sum behind rf_texture_sample_backward and the two
stages of rf_mesh_geometry_backward_gather, and the crafted lists its GPU test runs (not a test module).  The order of the kernel's
additions is a function of the entry list and the threshold alone, so the replay gives its BITS, not a bound:

* a segment of at most ``threshold`` entries: acc = 0, then acc = acc + term for its entries in order;
* a longer one: lane l of 64 sums the entries l, l + 64, ... that way, then for step = 32, 16, ..., 1 every lane adds the value of lane
  l + step (its own where l + step > 63) to its own, all lanes at once; lane 0 holds the result.

A term is the row an entry names, or the float32 product weight * row for the weighted form; nothing is fused (-ffp-contract=off)."""
import numpy as np

from tests.helpers import hash_uniform
from tests.texture_fit_model import CRAFTED_LENGTHS

THRESHOLDS = (1, 16, 64, 1 << 30)  # all long; the library's default; the wavefront's width; all short
LANES = 64

# stage one of the mesh case: CRAFTED_LENGTHS has no segment past the first 64, so the list goes on into a second wavefront
FACE_LENGTHS = CRAFTED_LENGTHS + (0,) * 45 + (3, 70, 0, 17, 130, 1, 2, 0, 5, 65, 9, 0, 31, 16, 4, 1)
# stage two: the 3 T corner slots of those T faces, over V vertices
VERTEX_LENGTHS = (0, 5, 17, 1, 65, 0, 16) + (1,) * 60 + (0, 20, 2, 66)
NUM_RECORDS = 5000


def covers(lengths, threshold) -> bool:
    """what a crafted list has to have at ``threshold``: an empty segment, a long segment on a lane other than 0, a long segment in a
    wavefront other than the first, a segment count that is no multiple of the wavefront"""
    lengths = np.asarray(lengths)
    long_at = np.nonzero(lengths > threshold)[0]
    return bool((lengths == 0).any() and (long_at % LANES != 0).any() and (long_at >= LANES).any() and len(lengths) % LANES != 0)


def replay(offsets, terms, threshold) -> np.ndarray:
    """float32 [K, C]: the kernel's sums of ``terms`` float32 [E, C] (entry order) over the segments of ``offsets`` int64 [K + 1]"""
    terms = np.ascontiguousarray(terms, dtype=np.float32)
    K, C = len(offsets) - 1, terms.shape[1]
    out = np.zeros((K, C), np.float32)
    lane = np.arange(LANES)
    for k in range(K):
        seg = terms[offsets[k]:offsets[k + 1]]
        if len(seg) == 0:
            continue
        if len(seg) <= threshold:
            out[k] = np.add.accumulate(seg, axis=0, dtype=np.float32)[-1]  # (one addition after another; 0 + the first is the first)
            continue
        rounds = -(-len(seg) // LANES)
        padded = np.zeros((rounds * LANES, C), np.float32)  # (a lane that runs out of entries adds nothing: here it adds +0)
        padded[:len(seg)] = seg
        acc = np.add.accumulate(padded.reshape(rounds, LANES, C), axis=0, dtype=np.float32)[-1]
        step = LANES // 2
        while step >= 1:
            acc = acc + acc[np.where(lane + step < LANES, lane + step, lane)]
            step //= 2
        out[k] = acc[0]
    return out


def texture_terms(pixel, weight, grad_colour) -> np.ndarray:
    """the terms of rf_texture_sample_backward: the float32 products weight * grad_colour[pixel]"""
    return weight.astype(np.float32)[:, None] * grad_colour.astype(np.float32)[pixel]


def crafted_mesh_lists(seed=77):
    """The two-level list of rf_mesh_geometry_backward_gather made by hand: (records float32 [P, 9], hit_pixels int32 [E], face_offsets
    int64 [T + 1], corner_slots int32 [3 T], vertex_offsets int64 [V + 1]).  Face k has FACE_LENGTHS[k] hit pixels, all among the
    first NUM_RECORDS records (P = E rows are allocated: the entry point takes no more hits than pixels); the corner slots are a
    permutation of the 3 T rows of the face gradients, cut into VERTEX_LENGTHS."""
    face_offsets = np.concatenate([[0], np.cumsum(FACE_LENGTHS)]).astype(np.int64)
    vertex_offsets = np.concatenate([[0], np.cumsum(VERTEX_LENGTHS)]).astype(np.int64)
    E, T = int(face_offsets[-1]), len(FACE_LENGTHS)
    assert int(vertex_offsets[-1]) == 3 * T
    hit_pixels = np.concatenate([(np.arange(n, dtype=np.int64) * 7 + 13 * k) % NUM_RECORDS for k, n in enumerate(FACE_LENGTHS)]).astype(np.int32)
    records = np.zeros((E, 9), np.float32)
    records[:NUM_RECORDS] = hash_uniform((NUM_RECORDS, 9), seed)
    corner_slots = ((np.arange(3 * T, dtype=np.int64) * 101 + 7) % (3 * T)).astype(np.int32)  # (101 and 3 T = 252 are coprime)
    return records, hit_pixels, face_offsets, corner_slots, vertex_offsets


def replay_mesh(records, hit_pixels, face_offsets, corner_slots, vertex_offsets, threshold):
    """(face gradients float32 [T, 9], vertex gradients float32 [V, 3]) as the two launches give them"""
    face_grads = replay(face_offsets, records[hit_pixels], threshold)
    return face_grads, replay(vertex_offsets, face_grads.reshape(-1, 3)[corner_slots], threshold)
