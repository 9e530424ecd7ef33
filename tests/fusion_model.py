"""Float64 numpy restatement of rf_fuse_depth_views (include/relu_field.h) and of the finalisation of
thr3ed_atom_amd/fusion.py, with the margin of every decision the rule takes and the per-node error bound of docs/fusion_errors.md.

The node positions are INPUTS of the rule: they are defined by float32 operations (``node_positions``), and the model projects
exactly those float32 values, as it takes the float32 poses, focals, depths and thresholds.  Everything after that is float64
(``dtype=np.float32`` evaluates the same expressions in float32 in the kernel's operation order: a CPU stand-in for the kernel)."""
from typing import NamedTuple, Optional

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


class Camera(NamedTuple):
    rotation: np.ndarray     # [3, 3] camera-to-world
    translation: np.ndarray  # [3]
    focal: float


def node_positions(aabb_min, aabb_max, dims) -> np.ndarray:
    """[X, Y, Z, 3] float32: aabb_min + (aabb_max - aabb_min) * ((2i + 1) / (2 dim)) per axis, every operation in float32"""
    axes = []
    for a in range(3):
        lo, hi = np.float32(aabb_min[a]), np.float32(aabb_max[a])
        i = np.arange(dims[a], dtype=np.int64)
        frac = (2 * i + 1).astype(np.float32) / np.float32(2 * dims[a])
        axes.append((lo + (hi - lo) * frac).astype(np.float32))
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32)


class Fused(NamedTuple):
    tsdf_sum: np.ndarray     # [X, Y, Z]
    observed: np.ndarray     # [X, Y, Z] int64
    hidden: np.ndarray       # [X, Y, Z] int64
    colour_sum: Optional[np.ndarray]  # [X, Y, Z, 4]
    margins: dict            # per decision: [X, Y, Z], the smallest margin over the views that reached the decision, DIVIDED by the
    #                          float32 error of the compared quantity (docs/fusion_errors.md): below 1, float32 cannot decide.  "alpha"
    #                          and "depth" compare inputs without arithmetic (error 0): they hold the plain margin and decide always.
    bound: np.ndarray        # [X, Y, Z]: the bound on |float32 tsdf_sum - tsdf_sum| of docs/fusion_errors.md
    colour_bound: Optional[np.ndarray]  # [X, Y, Z]: the same for every component of colour_sum


def errors(L, f, cx, cy, z, W, H):
    """(E_z, E_x, E_y) of docs/fusion_errors.md for nodes at distance L from the camera"""
    e_c = 5.0 * U * L
    with np.errstate(divide="ignore", invalid="ignore"):
        e_x = f * e_c * (1.0 + np.abs(cx) / z) / z + 3.0 * U * (np.abs(f * cx / z) + W)
        e_y = f * e_c * (1.0 + np.abs(cy) / z) / z + 3.0 * U * (np.abs(f * cy / z) + H)
    return e_c, e_x, e_y


def fuse(aabb_min, aabb_max, dims, cameras, height, width, depths, alphas=None, images=None, near=0.0, truncation=1.0, min_alpha=0.5, carve=True,
         dtype=np.float64, initial=None) -> Fused:
    """The rule, views in order.  ``depths`` [n, H, W], ``alphas`` [n, H, W] or None, ``images`` [n, H, W, 3] or None (float32 values);
    ``initial`` = (tsdf_sum, observed, hidden, colour_sum) to continue from."""
    T = dtype
    dims = tuple(int(d) for d in dims)
    H, W = int(height), int(width)
    p = node_positions(aabb_min, aabb_max, dims).astype(T)
    near, trunc, min_alpha = np.float32(near), np.float32(truncation), np.float32(min_alpha)
    total = np.zeros(dims, T) if initial is None else np.array(initial[0], T)
    observed = np.zeros(dims, np.int64) if initial is None else np.array(initial[1], np.int64)
    hidden = np.zeros(dims, np.int64) if initial is None else np.array(initial[2], np.int64)
    colour = None
    if images is not None:
        colour = np.zeros(dims + (4,), T) if initial is None or initial[3] is None else np.array(initial[3], T)
    margins = {k: np.full(dims, np.inf) for k in ("pixel_x", "pixel_y", "edge_x", "edge_y", "near", "sdf", "alpha", "depth")}
    bound = np.zeros(dims)
    colour_bound = np.zeros(dims) if images is not None else None

    def lower(name, mask, value):
        margins[name][mask] = np.minimum(margins[name][mask], value[mask])

    for k, cam in enumerate(cameras):
        R, t, f = np.asarray(cam.rotation, np.float32).astype(T).reshape(3, 3), np.asarray(cam.translation, np.float32).astype(T).reshape(3), T(np.float32(cam.focal))
        d = p - t
        cx = (d[..., 0] * R[0, 0] + d[..., 1] * R[1, 0]) + d[..., 2] * R[2, 0]
        cy = (d[..., 0] * R[0, 1] + d[..., 1] * R[1, 1]) + d[..., 2] * R[2, 1]
        z = -((d[..., 0] * R[0, 2] + d[..., 1] * R[1, 2]) + d[..., 2] * R[2, 2])
        L = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            x = T(W) * T(0.5) + f * cx / z
            y = T(H) * T(0.5) - f * cy / z
        e_z, e_x, e_y = errors(L, float(f), cx.astype(np.float64), cy.astype(np.float64), z.astype(np.float64), W, H)
        live = np.isfinite(z)
        lower("near", live, np.abs(z.astype(np.float64) - float(near)) / e_z)
        live = live & (z > T(near))
        inside = live & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        with np.errstate(invalid="ignore"):
            finite = live & np.isfinite(x64) & np.isfinite(y64)
            lower("edge_x", finite, np.minimum(np.abs(x64), np.abs(x64 - W)) / e_x)
            lower("edge_y", finite, np.minimum(np.abs(y64), np.abs(y64 - H)) / e_y)
            lower("pixel_x", inside, np.abs(x64 - np.rint(x64)) / e_x)
            lower("pixel_y", inside, np.abs(y64 - np.rint(y64)) / e_y)
        j = np.where(inside, np.floor(np.where(inside, x64, 0.0)), 0).astype(np.int64)
        i = np.where(inside, np.floor(np.where(inside, y64, 0.0)), 0).astype(np.int64)
        D = np.asarray(depths[k], np.float32)[i, j]
        known = inside & np.isfinite(D)
        miss = ~(D > 0)
        lower("depth", known, np.abs(D.astype(np.float64)))
        if alphas is not None:
            A = np.asarray(alphas[k], np.float32)[i, j]
            with np.errstate(invalid="ignore"):
                miss = miss | (A < min_alpha)
                lower("alpha", known & (D > 0) & np.isfinite(A), np.abs(A.astype(np.float64) - float(min_alpha)))
        hit = known & ~miss
        with np.errstate(invalid="ignore", over="ignore"):
            sdf = D.astype(T) - z
            sdf64 = sdf.astype(np.float64)
            e_sdf = e_z + U * np.abs(sdf64)
            lower("sdf", hit, np.minimum(np.abs(sdf64 + float(trunc)), np.abs(sdf64 - float(trunc))) / e_sdf)
            behind = hit & (sdf < -T(trunc))
            s = np.minimum(T(1.0), sdf / T(trunc))
        hidden[behind] += 1
        counted = (hit & ~behind) | (known & miss & bool(carve))
        s = np.where(hit, s, T(1.0))
        total = np.where(counted, total + s, total).astype(T)
        observed[counted] += 1
        # the bound: the value added (a hit that is not hidden) + the rounding of the addition
        with np.errstate(invalid="ignore", over="ignore"):
            term = U * (5.0 * L + 2.0 * (np.abs(D.astype(np.float64)) + np.abs(z.astype(np.float64)))) / float(trunc)
        bound = bound + np.where(hit & ~behind, term, 0.0) + np.where(counted, U * np.abs(total.astype(np.float64)), 0.0)
        if images is not None:
            with np.errstate(invalid="ignore"):
                near_surface = hit & (np.abs(sdf) <= T(trunc))
            rgb = np.asarray(images[k], np.float32)[i, j].astype(T)
            add = np.concatenate([rgb, np.ones(dims + (1,), T)], axis=-1)
            colour = np.where(near_surface[..., None], colour + add, colour).astype(T)
            colour_bound = colour_bound + np.where(near_surface, U * np.abs(colour.astype(np.float64)).max(-1), 0.0)
    return Fused(total, observed, hidden, colour, margins, bound, colour_bound)


def undecidable(fused: Fused, with_colour: bool = True) -> np.ndarray:
    """[X, Y, Z] bool: the nodes at which some decision of some view has a margin below its float32 error.  (The pixel edges 0, W and H
    are integers: "edge" is implied by "pixel" for nodes inside the image and matters alone for nodes just outside it.)"""
    m = fused.margins
    out = np.zeros(fused.observed.shape, bool)
    for name in ("pixel_x", "pixel_y", "edge_x", "edge_y", "near", "sdf"):
        out |= m[name] < 1.0
    return out


def finalise(tsdf_sum, observed, hidden) -> np.ndarray:
    """tsdf_sum / observed where observed > 0; -1 where observed == 0 and hidden > 0; +1 elsewhere"""
    tsdf_sum = np.asarray(tsdf_sum, np.float64)
    return np.where(observed > 0, tsdf_sum / np.maximum(observed, 1), np.where(hidden > 0, -1.0, 1.0))


def brute_force(aabb_min, aabb_max, dims, cameras, height, width, depths, alphas=None, images=None, near=0.0, truncation=1.0, min_alpha=0.5, carve=True):
    """The rule once more, node by node and view by view in Python floats (tiny inputs only): (tsdf_sum, observed, hidden, colour_sum)"""
    import math

    dims = tuple(int(d) for d in dims)
    p = node_positions(aabb_min, aabb_max, dims)
    H, W = int(height), int(width)
    near, trunc, min_alpha = float(np.float32(near)), float(np.float32(truncation)), float(np.float32(min_alpha))
    total, observed, hidden = np.zeros(dims), np.zeros(dims, np.int64), np.zeros(dims, np.int64)
    colour = np.zeros(dims + (4,)) if images is not None else None
    for node in np.ndindex(*dims):
        px, py, pz = (float(v) for v in p[node])
        for k, cam in enumerate(cameras):
            R, t, f = np.asarray(cam.rotation, np.float32).astype(np.float64).reshape(3, 3), np.asarray(cam.translation, np.float32).astype(np.float64).reshape(3), float(np.float32(cam.focal))
            c = R.T @ (np.array([px, py, pz]) - t)
            z = -float(c[2])
            if not (math.isfinite(z) and z > near):
                continue
            x, y = W / 2 + f * float(c[0]) / z, H / 2 - f * float(c[1]) / z
            if not (0 <= x < W and 0 <= y < H):
                continue
            j, i = int(math.floor(x)), int(math.floor(y))
            D = float(depths[k][i][j])
            if not math.isfinite(D):
                continue
            miss = D <= 0 or (alphas is not None and float(alphas[k][i][j]) < min_alpha)
            if miss:
                if not carve:
                    continue
                s = 1.0
            else:
                sdf = D - z
                if sdf < -trunc:
                    hidden[node] += 1
                    continue
                s = min(1.0, sdf / trunc)
                if images is not None and abs(sdf) <= trunc:
                    colour[node][:3] += np.asarray(images[k][i][j], np.float64)
                    colour[node][3] += 1
            total[node] += s
            observed[node] += 1
    return total, observed, hidden, colour


# ---- the cases the tests share -------------------------------------------------------------------------------------------------------

def look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)) -> Camera:
    """camera-to-world rotation with the camera looking down its -z axis at ``target`` (the convention of rf_cast_rays)"""
    position, target, up = (np.asarray(v, np.float64) for v in (position, target, up))
    back = position - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    true_up = np.cross(back, right)
    return Camera(np.stack([right, true_up, back], axis=1).astype(np.float32), position.astype(np.float32), 0.0)


def ring(count, radius, elevation, phase=0.0):
    return [(radius * np.cos(elevation) * np.cos(phase + 2 * np.pi * q / count), radius * np.cos(elevation) * np.sin(phase + 2 * np.pi * q / count), radius * np.sin(elevation))
            for q in range(count)]


SPHERE_RADIUS = 0.6
SPHERE_BOX = ((-1.0, -0.9, -0.8), (1.1, 0.95, 0.85))
SPHERE_DIMS = (24, 20, 16)
SPHERE_IMAGE = (32, 40, 36.0)  # H, W, focal


def sphere_cameras(focal=SPHERE_IMAGE[2]):
    """6 cameras on a ring at radius 3.2 and elevation 0.45 rad, 2 at radius 3.0 and -0.2 rad, all looking at the origin"""
    positions = ring(6, 3.2, 0.45) + ring(2, 3.0, -0.2, phase=0.7)
    return [look_at(pos)._replace(focal=float(focal)) for pos in positions]


def pixel_rays(cam: Camera, H, W):
    """(origin [3], directions [H, W, 3]) of rf_cast_rays in float64: pixel (i, j) looks through ((j + 1/2 - W/2) / f, -(i + 1/2 - H/2) / f, -1)"""
    R, f = np.asarray(cam.rotation, np.float64), float(cam.focal)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    local = np.stack([(jj - W / 2) / f, -(ii - H / 2) / f, -np.ones_like(jj)], axis=-1)
    return np.asarray(cam.translation, np.float64), local @ R.T


def sphere_depths(cameras, H, W, radius=SPHERE_RADIUS, centre=(0.0, 0.0, 0.0)):
    """[n, H, W] float32: the ray parameter of the first intersection with the sphere per pixel centre, 0 where the ray misses.  (The
    direction has camera-z -1, so the parameter is the camera-space depth.)"""
    out = np.zeros((len(cameras), H, W), np.float32)
    for k, cam in enumerate(cameras):
        o, d = pixel_rays(cam, H, W)
        oc = o - np.asarray(centre, np.float64)
        a, b, c = (d * d).sum(-1), 2.0 * (d @ oc), float(oc @ oc) - radius * radius
        disc = b * b - 4 * a * c
        t = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2 * a)
        out[k] = np.where((disc > 0) & (t > 0), t, 0.0).astype(np.float32)
    return out


def sphere_case(dims=SPHERE_DIMS, image=SPHERE_IMAGE, views=8, box=SPHERE_BOX):
    """the base case: (aabb_min, aabb_max, dims, cameras, H, W, depths, alphas, images, truncation)"""
    H, W, focal = image
    cameras = sphere_cameras(focal)[:views] if views <= 8 else (sphere_cameras(focal) * ((views + 7) // 8))[:views]
    depths = sphere_depths(cameras, H, W)
    alphas = (depths > 0).astype(np.float32) * np.float32(0.75) + np.float32(0.125)  # 0.875 on the sphere, 0.125 off it
    rng = np.random.default_rng(7)
    images = rng.random((len(cameras), H, W, 3), dtype=np.float32)
    truncation = float(np.float32(3.0 * max((hi - lo) / n for lo, hi, n in zip(np.float32(box[0]).astype(float), np.float32(box[1]).astype(float), dims))))
    return box[0], box[1], tuple(dims), cameras, H, W, depths, alphas, images, truncation


# the exact cases: a one-node-thick slab facing a camera 4 away on the axis it is thin along, 16 x 16 pixels, focal 16.  Node (a, b) of
# the slab's 8 x 8 projects onto the CENTRE of pixel (i, j) = (11 - b, 4 + a) with exact float32 arithmetic (x = 8 + 4 c_x with
# c_x = -0.875 + 0.25 a) at camera depth exactly 4.  Columns 4 .. 11 of views 0 and 1 hold the depth 4 + EXACT_DELTAS[a]; with the
# truncation 1/2 a node of column a therefore gets EXACT_S[a] from each of them (None: hidden).  View 2 sees nothing (depth 0) and
# view 3 knows nothing (NaN).
EXACT_DELTAS = (1.0, 0.5, 0.25, 0.125, 0.0, -0.25, -0.5, -1.0)
EXACT_S = (1.0, 1.0, 0.5, 0.25, 0.0, -0.5, -1.0, None)
EXACT_TRUNCATION = 0.5
# per column a with carving: tsdf_sum = 2 s + 1 (the carve of view 2), observed 3; the hidden column: the carve alone
EXACT_SUM_CARVE = (3.0, 3.0, 2.0, 1.5, 1.0, 0.0, -1.0, 1.0)
EXACT_OBSERVED_CARVE = (3, 3, 3, 3, 3, 3, 3, 1)
# ... and without: tsdf_sum = 2 s, observed 2; the hidden column is seen by nobody
EXACT_SUM_PLAIN = (2.0, 2.0, 1.0, 0.5, 0.0, -1.0, -2.0, 0.0)
EXACT_OBSERVED_PLAIN = (2, 2, 2, 2, 2, 2, 2, 0)
EXACT_HIDDEN = (0, 0, 0, 0, 0, 0, 0, 2)
# the finalised tsdf: sum / observed; the hidden-only column stays solid (-1) without the carve
EXACT_TSDF_CARVE = (1.0, 1.0, 2.0 / 3.0, 0.5, 1.0 / 3.0, 0.0, -1.0 / 3.0, 1.0)
EXACT_TSDF_PLAIN = (1.0, 1.0, 0.5, 0.25, 0.0, -0.5, -1.0, -1.0)
# the colour: views 0 and 1 hold the constant colours (0.25, 0.5, 0.75) and (0.75, 0.5, 0.25); |sdf| <= 1/2 in columns 1 .. 6
EXACT_COLOUR_COUNT = (0, 2, 2, 2, 2, 2, 2, 0)
EXACT_COLOUR_SUM = (1.0, 1.0, 1.0)


def exact_case(axis: int):
    """The slab thin along ``axis`` (2: dims (8, 8, 1), 0: (1, 8, 8), 1: (8, 1, 8)) and its camera on that axis: (aabb_min, aabb_max, dims,
    cameras, H, W, depths, images, truncation, (a_axis, b_axis)): the lattice axes the columns a and the rows b of the table run along."""
    rotations = {2: ((1, 0, 0), (0, 1, 0), (0, 0, 1)),   # columns right, up, back: c_x = d_x, c_y = d_y
                 0: ((0, 0, 1), (1, 0, 0), (0, 1, 0)),   # c_x = d_y, c_y = d_z
                 1: ((0, 1, 0), (0, 0, 1), (1, 0, 0))}   # c_x = d_z, c_y = d_x
    ab = {2: (0, 1), 0: (1, 2), 1: (2, 0)}[axis]
    dims = [8, 8, 8]
    dims[axis] = 1
    t = [0.0, 0.0, 0.0]
    t[axis] = 4.0
    cam = Camera(np.array(rotations[axis], np.float32), np.array(t, np.float32), 16.0)
    H = W = 16
    depths = np.zeros((4, H, W), np.float32)
    depths[0:2, :, 4:12] = np.float32(4.0) + np.array(EXACT_DELTAS, np.float32)
    depths[0:2, :, :4] = 9.0
    depths[0:2, :, 12:] = 9.0
    depths[3] = np.nan
    images = np.zeros((4, H, W, 3), np.float32)
    images[0], images[1], images[2], images[3] = (0.25, 0.5, 0.75), (0.75, 0.5, 0.25), (0.125, 0.125, 0.125), (0.5, 0.5, 0.5)
    return (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), tuple(dims), [cam] * 4, H, W, depths, images, EXACT_TRUNCATION, ab


def exact_expected(axis: int, table) -> np.ndarray:
    """``table`` (one value per column a) spread over the slab of ``exact_case(axis)``: [X, Y, Z]"""
    dims = [8, 8, 8]
    dims[axis] = 1
    a_axis = {2: 0, 0: 1, 1: 2}[axis]
    shape = [1, 1, 1]
    shape[a_axis] = 8
    return np.broadcast_to(np.array(table).reshape(shape), dims).copy()
