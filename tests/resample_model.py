"""float64 numpy model of rf_resample_grid and rf_node_bounds (include/relu_field.h), written from the definitions alone.

``resample``: destination node i on axis a sits at the continuous source index s_a = scale_a * i + offset_a; outside
[-0.5, n_a - 0.5] on any axis the node is (fill, 0 ...); otherwise s is clamped to [0, n - 1], i0 = min(floor(s), n - 1),
i1 = min(i0 + 1, n - 1), lambda = s - i0, and every raw channel is the trilinear sum of the 8 corners.  scale / offset are taken as
the float32 values the kernel receives; everything after that is float64 (so s carries no rounding here: for dyadic scales and
offsets the kernel's s is exact too, otherwise it differs by one float32 rounding of s, which ``slope`` prices).

``node_bounds``: the index box and the number of the nodes with post(pre(D * rho)) > threshold.  The product D * rho is rounded to
float32 as the kernel's is (one multiply); the activation and the comparison are float64."""
import numpy as np


def axis_map(n_dst, n_src, scale, offset):
    s = np.float64(np.float32(scale)) * np.arange(n_dst, dtype=np.float64) + np.float64(np.float32(offset))
    outside = (s < -0.5) | (s > n_src - 0.5)
    s = np.clip(s, 0.0, n_src - 1.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, s - i0, outside


def resample(densities, features, dst_dims, scale, offset, fill=0.0, return_slope=False):
    """densities [X,Y,Z,1], features [X,Y,Z,F] (any float dtype) -> (densities64 [X',Y',Z',1], features64 [X',Y',Z',F]); with
    ``return_slope`` also sum_a |d value / d s_a| per element as a pair of the same shapes (0 outside the source box)."""
    vol = np.concatenate([np.asarray(densities, dtype=np.float64), np.asarray(features, dtype=np.float64)], axis=-1)
    src = vol.shape[:3]
    ax = [axis_map(dst_dims[a], src[a], scale[a], offset[a]) for a in range(3)]
    shape = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    w = [[(1.0 - ax[a][2]).reshape(shape[a]), ax[a][2].reshape(shape[a])] for a in range(3)]
    idx = [[ax[a][0].reshape(shape[a]), ax[a][1].reshape(shape[a])] for a in range(3)]
    out = np.zeros((*dst_dims, vol.shape[-1]))
    grad = [np.zeros_like(out) for _ in range(3)]
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                d = (dx, dy, dz)
                val = vol[idx[0][dx], idx[1][dy], idx[2][dz]]
                out += val * (w[0][dx] * w[1][dy] * w[2][dz])[..., None]
                for a in range(3):
                    b, c = [k for k in range(3) if k != a]
                    grad[a] += (1.0 if d[a] else -1.0) * val * (w[b][d[b]] * w[c][d[c]])[..., None]
    outside = ax[0][3].reshape(shape[0]) | ax[1][3].reshape(shape[1]) | ax[2][3].reshape(shape[2])
    empty = np.zeros(vol.shape[-1])
    empty[0] = fill
    out = np.where(outside[..., None], empty, out)
    if not return_slope:
        return out[..., :1], out[..., 1:]
    slope = np.where(outside[..., None], 0.0, sum(np.abs(g) for g in grad))
    return out[..., :1], out[..., 1:], (slope[..., :1], slope[..., 1:])


def outside_mask(dst_dims, src_dims, scale, offset):
    ax = [axis_map(dst_dims[a], src_dims[a], scale[a], offset[a])[3] for a in range(3)]
    return ax[0][:, None, None] | ax[1][None, :, None] | ax[2][None, None, :]


def activated(densities, rho, mode):
    pre = (np.asarray(densities, dtype=np.float32) * np.float32(rho)).astype(np.float64)
    if mode == "abs":
        return np.abs(pre)
    if mode == "relu":
        return np.maximum(pre, 0.0)
    if mode == "softplus":
        return np.where(pre > 20.0, pre, np.log1p(np.exp(np.minimum(pre, 20.0))))
    assert mode == "identity", mode
    return pre


def node_bounds(densities, rho, mode, threshold):
    """densities [X,Y,Z] or [X,Y,Z,1] -> (lo (3), hi (3), count), or None when no node passes"""
    d = np.asarray(densities)
    d = d[..., 0] if d.ndim == 4 else d
    passing = activated(d, rho, mode) > np.float64(np.float32(threshold))
    if not passing.any():
        return None
    idx = np.argwhere(passing)
    return tuple(int(v) for v in idx.min(0)), tuple(int(v) for v in idx.max(0)), int(passing.sum())


def merge_bounds(bounds6, found):
    """what a call adds to the six values a caller holds"""
    if found is None:
        return list(bounds6)
    lo, hi, _ = found
    return [min(bounds6[a], lo[a]) for a in range(3)] + [max(bounds6[3 + a], hi[a]) for a in range(3)]


def node_world_positions(aabb, dims):
    """float64 world coordinates of the nodes per axis: lo + (i + 1/2) (hi - lo) / n"""
    return [np.float64(lo) + (np.arange(n, dtype=np.float64) + 0.5) * (np.float64(hi) - np.float64(lo)) / n for (lo, hi), n in zip(aabb, dims)]
