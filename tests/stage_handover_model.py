"""Float64 model of what the trainer runs at the end of a stage -- visibility statistic, prune, tighten (crop + resample) -- as the CHAIN
of the models the suite already has: tests/node_weights_model.py (model_max_weight, keep_mask, prune), tests/resample_model.py
(node_bounds, resample) and the host rules thr3ed_atom_amd.resampling.tightened_dims / resample_map.  The scene is the end-to-end scene
of tests/node_weights_model.py: 24^3 nodes, six views, a shell on nodes 5..18, a hidden blob, a faint speck outside the shell."""
import functools

import numpy as np
import torch

from oracle import relu_field_oracle as orc
from tests import node_weights_model as nm
from tests import resample_model as rm
from tests.helpers import hotdog_like_camera

TIGHTEN_THRESHOLD = 0.0
MARGIN = 1
DILATE = 1
BUDGET = 20**3  # 16 source nodes -> 20 per axis: the scale 4/5 is not dyadic
M_BAR = 1e-5  # the bar of tests/test_hip_node_weights.py on the statistic


def scene_bounds():
    cam = hotdog_like_camera()
    return float(np.float32(cam["near"])), float(np.float32(cam["far"]))


def view_rays(view):
    (h, w, focal), poses = nm.scene_views()
    pose = poses[view]
    o, d = orc.cast_rays(h, w, focal, torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def crop_box(found, dims, margin=MARGIN):
    lo, hi, _ = found
    return [max(lo[a] - margin, 0) for a in range(3)], [min(hi[a] + margin, dims[a] - 1) for a in range(3)]


@functools.lru_cache(maxsize=None)
def chain():
    """the whole hand-over in float64, computed once, never modified.  Returns a dict: ``M`` [24,24,24]; ``keep``, ``pruned_densities``
    (float32), ``counts`` (kept, pruned); ``box`` / ``box_unpruned``: node_bounds after / without the pruning step; ``first`` / ``last``:
    the crop; ``new_dims``, ``new_voxel``, ``location``, ``new_aabb``; ``densities`` / ``features``: the resampled tensors (float64) and
    ``slope_d`` / ``slope_f`` their sum_a |d value / d s_a|; ``source_max``: max |value| of the cropped densities / features."""
    from thr3ed_atom_amd.resampling import resample_map, tightened_dims

    dens, feat = nm.scene_grid()
    aabb = orc.make_aabb(nm.SCENE_DIMS, nm.SCENE_VOXEL)
    near, far = scene_bounds()
    M = None
    for view in range(len(nm.SCENE_VIEWS)):
        o, d = view_rays(view)
        M, _, _ = nm.model_max_weight(dens, aabb, nm.SCENE_RHO, "relu", o, d, near, far, nm.SCENE_SAMPLES, prefill=M)
    keep, pruned, counts = nm.prune(dens.numpy(), M, nm.SCENE_TAU, DILATE, 0.0, "relu")
    box = rm.node_bounds(pruned, nm.SCENE_RHO, "relu", TIGHTEN_THRESHOLD)
    box_unpruned = rm.node_bounds(dens.numpy(), nm.SCENE_RHO, "relu", TIGHTEN_THRESHOLD)
    first, last = crop_box(box, nm.SCENE_DIMS)
    sl = tuple(slice(first[a], last[a] + 1) for a in range(3))
    crop_d, crop_f = pruned[sl], feat.numpy()[sl]
    crop_dims = tuple(last[a] - first[a] + 1 for a in range(3))
    location = tuple(aabb[a][0] + (first[a] + last[a] + 1) / 2 * nm.SCENE_VOXEL[a] for a in range(3))
    crop_aabb = orc.make_aabb(crop_dims, nm.SCENE_VOXEL, location)
    new_dims = tightened_dims(crop_dims, nm.SCENE_VOXEL, BUDGET)
    new_voxel = tuple(nm.SCENE_VOXEL[a] * crop_dims[a] / new_dims[a] for a in range(3))
    scale, offset = resample_map(crop_aabb, nm.SCENE_VOXEL, location, new_voxel, new_dims)
    d64, f64, (sd, sf) = rm.resample(crop_d, crop_f, new_dims, scale, offset, return_slope=True)
    return {"M": M, "keep": keep, "pruned_densities": pruned, "counts": counts, "box": box, "box_unpruned": box_unpruned, "first": first, "last": last,
            "crop_dims": crop_dims, "new_dims": new_dims, "new_voxel": new_voxel, "location": location, "new_aabb": orc.make_aabb(new_dims, new_voxel, location),
            "densities": d64, "features": f64, "slope_d": sd, "slope_f": sf, "source_max": (float(np.abs(crop_d).max()), float(np.abs(crop_f).max())),
            "outside": rm.outside_mask(new_dims, crop_dims, scale, offset)}
