"""GPU: the shared segmented sum (csrc/segment_sum.h) through its three instantiations -- rf_texture_sample_backward (3 floats, weighted)
and the two launches of rf_mesh_geometry_backward_gather (9 and 3 floats, unit weight) -- on crafted lists, BIT FOR BIT against the
float32 replay of tests/segment_sum_model.py, at thresholds on either side of which every segment is long, short, or mixed."""
import functools

import numpy as np
import pytest
import torch

from tests import segment_sum_model as ssm
from tests import texture_fit_model as tfm
from thr3ed_atom_amd import _lib

pytestmark = pytest.mark.gpu

THRESHOLDS = ssm.THRESHOLDS + (0,)  # 0: the library's default


def effective(threshold, default):
    return threshold if threshold else default


@functools.lru_cache(maxsize=None)
def texture_list():
    return tfm.crafted_list()


@functools.lru_cache(maxsize=None)
def mesh_lists():
    return ssm.crafted_mesh_lists()


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_texture_sample_backward_is_the_replay_bit_for_bit(hip_device, threshold):
    offsets, pixel, weight, grad_colour = texture_list()
    want = ssm.replay(offsets, ssm.texture_terms(pixel, weight, grad_colour), effective(threshold, _lib.TEXTURE_FIT_LONG_SEGMENT))
    K, P, E = len(offsets) - 1, len(grad_colour), len(pixel)
    entries = torch.from_numpy(np.stack([pixel, weight.view(np.int32)], 1).copy()).to(hip_device)
    offsets_dev, g = torch.from_numpy(offsets).to(hip_device), torch.from_numpy(grad_colour).to(hip_device)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    grad = torch.full((1, K, 3), 7.0, dtype=torch.float32, device=hip_device)  # (every texel is written: no 7 survives)
    rc = _lib.load().rf_texture_sample_backward(g.data_ptr(), P, offsets_dev.data_ptr(), entries.data_ptr(), E, 1, K, threshold, 0, grad.data_ptr(), status.data_ptr(),
                                                torch.cuda.current_stream(hip_device).cuda_stream)
    assert rc == 0
    got = grad.cpu().numpy().reshape(K, 3)
    assert int(status.item()) == 0 and np.array_equal(got, want), (threshold, int((got != want).sum()))
    assert (got[np.diff(offsets) == 0] == 0.0).all()


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_mesh_geometry_backward_gather_is_the_replay_bit_for_bit(hip_device, threshold):
    records, hit_pixels, face_offsets, corner_slots, vertex_offsets = mesh_lists()
    want_faces, want_vertices = ssm.replay_mesh(records, hit_pixels, face_offsets, corner_slots, vertex_offsets, effective(threshold, _lib.MESH_FIT_LONG_SEGMENT))
    T, V = len(face_offsets) - 1, len(vertex_offsets) - 1
    dev = [torch.from_numpy(a).to(hip_device) for a in (records, hit_pixels, face_offsets, corner_slots, vertex_offsets)]
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    face_grads = torch.full((T, 9), 7.0, dtype=torch.float32, device=hip_device)  # (every row is written: no 7 survives)
    grad = torch.full((V, 3), 7.0, dtype=torch.float32, device=hip_device)
    rc = _lib.load().rf_mesh_geometry_backward_gather(dev[0].data_ptr(), len(records), dev[1].data_ptr(), len(hit_pixels), dev[2].data_ptr(), T, dev[3].data_ptr(),
                                                      dev[4].data_ptr(), V, threshold, 0, face_grads.data_ptr(), grad.data_ptr(), status.data_ptr(),
                                                      torch.cuda.current_stream(hip_device).cuda_stream)
    assert rc == 0
    got_faces, got_vertices = face_grads.cpu().numpy(), grad.cpu().numpy()
    assert int(status.item()) == 0
    assert np.array_equal(got_faces, want_faces), (threshold, int((got_faces != want_faces).sum()))
    assert np.array_equal(got_vertices, want_vertices), (threshold, int((got_vertices != want_vertices).sum()))
    assert (got_faces[np.diff(face_offsets) == 0] == 0.0).all() and (got_vertices[np.diff(vertex_offsets) == 0] == 0.0).all()
