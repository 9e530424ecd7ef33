"""The numpy model of thr3ed_atom_amd/mesh_distance.py and csrc/mesh_distance_kernels.hip (not a test module): the distance rule of
docs/mesh_distance_errors.md as a brute force over all faces (float64 for reference values; float32 restates closest_on_face of
csrc/mesh_distance.h operation for operation -- numpy rounds every float32 operation and fuses none), the lattice with its default
cell size and its pair lists, the ring search with its stop test, the error bound B(p, mesh), the sampler's strata rule and the
reductions of ``mesh_distance``."""
import math

import numpy as np

U = 2.0 ** -24  # the unit roundoff of float32
MAX_CELLS, MAX_TABLE, MAX_PAIRS_PER_FACE, MAX_PAIRS_SLACK = 1024, 1 << 25, 16, 1 << 20


# ---------------------------------------------------------------------------------------------------------------- the rule
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _candidate(p, q, lo, hi):
    q = np.fmin(np.fmax(q, lo), hi)
    d = p - q
    return _dot(d, d), q


def _segment(p, a, b, lo, hi):
    e, w = b - a, p - a
    l = _dot(e, e)
    with np.errstate(all="ignore"):
        t = np.where(l > 0, np.fmin(np.fmax(_dot(w, e) / l, 0), 1), 0).astype(p.dtype)
    return _candidate(p, a + t[..., None] * e, lo, hi)


def closest_on_face(p, a, b, c, dtype=np.float64):
    """(d2, q) of queries ``p`` against triangles (a, b, c), arrays of [..., 3] that broadcast: THE rule, in ``dtype``"""
    p, a, b, c = (np.asarray(x, dtype=dtype) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    best, point = _segment(p, a, b, lo, hi)
    for s, e in ((b, c), (c, a)):
        d2, q = _segment(p, s, e, lo, hi)
        take = d2 < best
        best, point = np.where(take, d2, best), np.where(take[..., None], q, point)
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    with np.errstate(all="ignore"):
        s = _dot(p - a, n) / nn
        q = p - s[..., None] * n
        inside = (nn > 0) & (_dot(_cross(b - a, q - a), n) >= 0) & (_dot(_cross(c - b, q - b), n) >= 0) & (_dot(_cross(a - c, q - c), n) >= 0)
        d2, q = _candidate(p, q, lo, hi)
        take = inside & (d2 < best)
    return np.where(take, d2, best), np.where(take[..., None], q, point)


def face_distances2(points, vertices, faces, dtype=np.float64, chunk=256):
    """[N, T] squared distances of every query to every face"""
    points = np.asarray(points, dtype=dtype).reshape(-1, 3)
    a, b, c = (np.asarray(vertices, dtype=dtype)[faces[:, k]] for k in range(3))
    out = np.empty((points.shape[0], faces.shape[0]), dtype=dtype)
    for i in range(0, points.shape[0], chunk):
        out[i:i + chunk] = closest_on_face(points[i:i + chunk, None, :], a[None], b[None], c[None], dtype)[0]
    return out


def brute_force(points, vertices, faces, dtype=np.float64, d2=None):
    """(distance [N], face [N], point [N, 3]): the smallest d2 over all faces, the lowest face index on an exact tie"""
    points = np.asarray(points, dtype=dtype).reshape(-1, 3)
    d2 = face_distances2(points, vertices, faces, dtype) if d2 is None else d2
    face = np.argmin(d2, axis=1)  # (the first minimum)
    v = np.asarray(vertices, dtype=dtype)
    best, point = closest_on_face(points, v[faces[face, 0]], v[faces[face, 1]], v[faces[face, 2]], dtype)
    return np.sqrt(best), face, point


# ---------------------------------------------------------------------------------------------------------------- the bound
def face_bounds(points, vertices, faces):
    """b(p, f) [N, T] of docs/mesh_distance_errors.md: |float32 distance of p to face f - its exact distance| <= b"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)[:, None, :]
    a, b, c = (np.asarray(vertices, dtype=np.float64)[faces[:, k]][None] for k in range(3))
    norm = lambda x: np.sqrt((x * x).sum(-1))  # noqa: E731
    S = np.maximum(np.abs(p).max(-1), np.maximum(np.maximum(np.abs(a).max(-1), np.abs(b).max(-1)), np.abs(c).max(-1)))
    W = np.maximum(np.maximum(norm(p - a), norm(p - b)), norm(p - c))
    L = np.maximum(np.maximum(norm(b - a), norm(c - b)), norm(a - c))
    out = U * (12 * W + 10 * L + 2 * S)
    n = norm(np.cross(b - a, c - a))
    with np.errstate(all="ignore"):
        theta = np.where(n > 0, np.minimum(8 * U * norm(b - a) * norm(c - a) / n, 1.0), 0.0)
    return out + np.where(n > 0, 2 * W * theta + U * (8 * W + 4 * S + 4 * L), 0.0)


def bound(points, vertices, faces, d=None):
    """B(p, mesh) [N]: the largest b(p, f) over the faces that can win or bound the float32 minimum, the contenders
    {f : d(f) - b(f) <= min_g (d(g) + b(g))}"""
    d = np.sqrt(face_distances2(points, vertices, faces)) if d is None else d
    b = face_bounds(points, vertices, faces)
    contender = d - b <= (d + b).min(axis=1, keepdims=True)
    return np.where(contender, b, 0.0).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------- the lattice
def lattice(vertices, faces, h):
    """(origin float32 [3], h, r, cells int64 [3]) or None when over the limits: the bounds are those of ALL vertices, as the binding's"""
    v = np.asarray(vertices, dtype=np.float32)
    low, high = v.min(axis=0), v.max(axis=0)
    h = np.float32(h)
    r = np.float32(1.0) / h
    cells = np.floor(((high - low).astype(np.float32) * r).astype(np.float32)).astype(np.int64) + 1
    if (cells > MAX_CELLS).any() or int(cells.prod()) + 1 > MAX_TABLE:
        return None
    return low, h, r, cells


def cells_of(values, grid):
    origin, _, r, cells = grid
    t = np.floor(((np.asarray(values, dtype=np.float32) - origin).astype(np.float32) * r).astype(np.float32))
    return np.minimum(np.maximum(t, 0), (cells - 1).astype(np.float32)).astype(np.int64)


def face_cell_ranges(vertices, faces, grid):
    corners = np.asarray(vertices, dtype=np.float32)[faces]
    return cells_of(corners.min(axis=1), grid), cells_of(corners.max(axis=1), grid)


def default_cell_size(vertices, faces):
    """the rule of MeshDistanceGrid(cell_size=None)"""
    v64 = np.asarray(vertices, dtype=np.float64)
    c = v64[faces]
    mean_area = float((0.5 * np.sqrt((np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]) ** 2).sum(-1))).sum()) / len(faces)
    v32 = np.asarray(vertices, dtype=np.float32)
    h = np.float32(2.0 * math.sqrt(2.0 * mean_area)) if mean_area > 0 else np.float32(0.0)
    if not (np.isfinite(h) and h > 0):
        h = np.float32((v32.max(axis=0) - v32.min(axis=0)).astype(np.float32).max())
    if not (np.isfinite(h) and h > 0):
        h = np.float32(1.0)
    while True:
        grid = lattice(vertices, faces, h)
        if grid is not None:
            lo, hi = face_cell_ranges(vertices, faces, grid)
            if int((hi - lo + 1).prod(axis=1).sum()) <= MAX_PAIRS_PER_FACE * len(faces) + MAX_PAIRS_SLACK:
                return h
        h = np.float32(h * np.float32(2.0))


def pair_lists(vertices, faces, grid, whole_box=True):
    """(cell_begin [cells + 1], cell_faces [P]): the faces of every cell, ascending within a cell (a stable sort of x-major pairs).
    ``whole_box=False`` is the BROKEN variant that registers a face only in the cells of its three corners."""
    cells = grid[3]
    keys, ids = [], []
    if whole_box:
        lo, hi = face_cell_ranges(vertices, faces, grid)
        for f in range(len(faces)):
            x, y, z = np.meshgrid(*(np.arange(lo[f, k], hi[f, k] + 1) for k in range(3)), indexing="ij")
            keys.append(((x * cells[1] + y) * cells[2] + z).reshape(-1))
            ids.append(np.full(keys[-1].size, f))
    else:
        k = cells_of(np.asarray(vertices, dtype=np.float32)[faces], grid)  # [T, 3, 3]
        keys, ids = [((k[..., 0] * cells[1] + k[..., 1]) * cells[2] + k[..., 2]).reshape(-1)], [np.repeat(np.arange(len(faces)), 3)]
    keys, ids = np.concatenate(keys), np.concatenate(ids)
    order = np.argsort(keys, kind="stable")
    begin = np.zeros(int(cells.prod()) + 1, dtype=np.int64)
    begin[1:] = np.cumsum(np.bincount(keys, minlength=int(cells.prod())))
    return begin, ids[order]


# ---------------------------------------------------------------------------------------------------------------- the ring search
def plane_below(o, h, K, slack=True):
    """a float32 <= every float32 coordinate whose cell index is >= K"""
    f = np.float32
    if not slack:
        return f(o + f(f(K) * h))
    x = f(o + f(f(f(K) * h) * f(1.0 - 2.0 ** -21)))
    return f(x - f(abs(x) * f(2.0 ** -22)))


def plane_above(o, h, K, slack=True):
    """a float32 >= every float32 coordinate whose cell index is < K"""
    f = np.float32
    if not slack:
        return f(o + f(f(K) * h))
    x = f(o + f(f(f(K) * h) * f(1.0 + 2.0 ** -21)))
    return f(x + f(abs(x) * f(2.0 ** -22)))


def ring_search(points, vertices, faces, grid, lists, max_distance=np.inf, slack=True):
    """(distance, face, point, rings) in float32: the kernel's walk, query by query"""
    f32 = np.float32
    origin, h, _, cells = grid
    begin, cell_faces = lists
    v = np.asarray(vertices, dtype=f32)
    points = np.asarray(points, dtype=f32).reshape(-1, 3)
    md = f32(max_distance)
    limit2 = f32(f32(md * md) * f32(1.0 + 2.0 ** -21))
    N = points.shape[0]
    out_d, out_f, out_q, out_r = np.full(N, np.inf, f32), np.full(N, -1, np.int64), np.full((N, 3), np.nan, f32), np.zeros(N, np.int64)
    for i, p in enumerate(points):
        c = cells_of(p, grid)
        best, best_face, R = f32(np.inf), -1, 0
        while True:
            lo, hi = np.maximum(c - R, 0), np.minimum(c + R, cells - 1)
            x, y, z = np.meshgrid(*(np.arange(lo[k], hi[k] + 1) for k in range(3)), indexing="ij")
            shell = np.maximum(np.maximum(abs(x - c[0]), abs(y - c[1])), abs(z - c[2])) == R
            seen = []
            for key in ((x * cells[1] + y) * cells[2] + z)[shell]:
                seen.append(cell_faces[begin[key]:begin[key + 1]])
            seen = np.unique(np.concatenate(seen)) if seen else np.zeros(0, np.int64)
            if seen.size:
                d2 = closest_on_face(p, v[faces[seen, 0]], v[faces[seen, 1]], v[faces[seen, 2]], f32)[0]
                k = int(np.argmin(d2))  # (seen ascends: the lowest face among equal d2)
                if d2[k] < best or (d2[k] == best and seen[k] < best_face):
                    best, best_face = d2[k], int(seen[k])
            if (c - R <= 0).all() and (c + R >= cells - 1).all():
                break
            gap = f32(np.inf)
            for k in range(3):
                if c[k] + R + 1 <= cells[k] - 1:
                    gap = min(gap, f32(plane_below(origin[k], h, c[k] + R + 1, slack) - p[k]))
                if c[k] - R >= 1:
                    gap = min(gap, f32(p[k] - plane_above(origin[k], h, c[k] - R, slack)))
            bound2 = f32(gap * gap) if gap > 0 else f32(0.0)
            if best < bound2 or bound2 > limit2:
                break
            R += 1
        out_r[i] = R
        if best_face >= 0 and np.sqrt(best) <= md:
            d2, q = closest_on_face(p, v[faces[best_face, 0]], v[faces[best_face, 1]], v[faces[best_face, 2]], f32)
            out_d[i], out_f[i], out_q[i] = np.sqrt(best), best_face, q
    return out_d, out_f, out_q, out_r


# ---------------------------------------------------------------------------------------------------------------- sampling, reductions
def strata_faces(area, u):
    """the face of every stratum: position (i + u_i) A / count along the float64 prefix sum of ``area``, the first face whose prefix
    exceeds it, never beyond the last face with area"""
    area, u = np.asarray(area, dtype=np.float64), np.asarray(u, dtype=np.float64)
    prefix = np.cumsum(area)
    position = (np.arange(u.size, dtype=np.float64) + u) * prefix[-1] / u.size
    return np.minimum(np.searchsorted(prefix, position, side="right"), np.nonzero(area > 0)[0].max())


def barycentrics(r1, r2):
    s = np.sqrt(np.asarray(r1, dtype=np.float64))
    return np.stack([1.0 - s, s * (1.0 - r2), s * r2], axis=-1)


def directed(samples, vertex_distances):
    d = np.sort(np.asarray(samples, dtype=np.float64))
    top = max(d[-1], np.asarray(vertex_distances, dtype=np.float64).max()) if len(vertex_distances) else d[-1]
    return {"mean": d.mean(), "rms": math.sqrt((d * d).mean()), "max": top, "median": np.quantile(d, 0.5), "q90": np.quantile(d, 0.9), "q99": np.quantile(d, 0.99)}


def reductions(d_ab, d_ba, v_ab, v_ba, thresholds=()):
    a, b = directed(d_ab, v_ab), directed(d_ba, v_ba)
    sq = lambda d: (np.asarray(d, dtype=np.float64) ** 2).mean()  # noqa: E731
    out = {"a_to_b": a, "b_to_a": b, "chamfer_l1": 0.5 * (a["mean"] + b["mean"]), "chamfer_l2": 0.5 * (sq(d_ab) + sq(d_ba)), "hausdorff": max(a["max"], b["max"]),
           "thresholds": []}
    for t in thresholds:
        precision, recall = float((np.asarray(d_ab) <= t).mean()), float((np.asarray(d_ba) <= t).mean())
        out["thresholds"].append({"threshold": t, "precision": precision, "recall": recall,
                                  "fscore": 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0})
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, f


def icosphere(subdivisions=3):
    """20 * 4^subdivisions faces on the unit sphere (1 280 at 3)"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        middle, out = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in middle:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                middle[key] = len(v) - 1
            return middle[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int64)


def perturbed(vertices, amplitude=0.05, seed=3):
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, dtype=np.float64)
    return (v * (1.0 + amplitude * rng.uniform(-1, 1, size=(len(v), 1)))).astype(np.float32)


def soup(h=np.float32(0.25), seed=5):
    """2 000 random triangles in [-1, 1]^3, 20 degenerate faces, one giant triangle across the box and 50 faces with corners exactly on
    the cell planes of the lattice of edge ``h`` from (-1, -1, -1) -- which two corner vertices pin as the mesh's bounds"""
    rng = np.random.default_rng(seed)
    grid32 = lambda x: (np.round(np.asarray(x) * 1024) / 1024).astype(np.float32)  # noqa: E731  (dyadic: differences are exact)
    centre = rng.uniform(-0.9, 0.9, size=(2000, 1, 3))
    tris = [np.clip(centre + rng.uniform(-0.1, 0.1, size=(2000, 3, 3)), -1, 1).astype(np.float32)]
    p, d = grid32(rng.uniform(-0.8, 0.8, size=(20, 3))), grid32(rng.uniform(-0.1, 0.1, size=(20, 3)))
    degenerate = np.stack([p, p, p], axis=1)                    # all three corners equal ...
    degenerate[:7, 2] = p[:7] + d[:7]                           # ... a repeated vertex: a segment ...
    degenerate[7:14, 1], degenerate[7:14, 2] = p[7:14] + d[7:14], p[7:14] + 2 * d[7:14]  # ... collinear corners (c - a = 2 (b - a) exactly)
    tris.append(degenerate.astype(np.float32))
    tris.append(np.array([[[-1, -1, -1], [1, 1, -0.5], [-0.5, 1, 1]]], dtype=np.float32))  # the giant one
    k = rng.integers(0, int(round(2.0 / float(h))) + 1, size=(50, 3, 3))
    snapped = (np.float32(-1.0) + k.astype(np.float32) * np.float32(h)).astype(np.float32)  # h = 2^-2: exact, on the planes
    snapped[:, 1:, :] = np.clip(snapped[:, :1, :] + (k[:, 1:, :] % 3 - 1).astype(np.float32) * np.float32(h), -1, 1)  # short edges, still on planes
    tris.append(snapped)
    tris.append(np.array([[[-1, -1, -1]] * 3, [[1, 1, 1]] * 3], dtype=np.float32))  # the bounds
    tris = np.concatenate(tris)
    return tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3)


def queries(vertices, faces, count, seed=11, h=None):
    """``count`` queries mixed from: inside the box, on vertices, on edge midpoints, exactly on cell planes (with ``h``), far outside
    (10 x the extent)"""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, dtype=np.float32)
    low, high = v.min(axis=0), v.max(axis=0)
    extent = (high - low).max()
    kinds = []
    n = max(count // 5, 1)
    kinds.append(rng.uniform(low - 0.1 * extent, high + 0.1 * extent, size=(count, 3)))
    kinds.append(v[faces[rng.integers(0, len(faces), n), rng.integers(0, 3, n)]])
    e = rng.integers(0, len(faces), n)
    kinds.append(0.5 * (v[faces[e, 0]].astype(np.float64) + v[faces[e, 1]]))
    if h is not None:
        on_plane = rng.uniform(low, high, size=(n, 3)).astype(np.float32)
        axis = rng.integers(0, 3, n)
        k = rng.integers(0, np.maximum(np.floor((high - low) / h), 1).astype(np.int64)[axis] + 1)
        on_plane[np.arange(n), axis] = (low[axis] + k.astype(np.float32) * np.float32(h)).astype(np.float32)
        kinds.append(on_plane)
    direction = rng.normal(size=(n, 3))
    kinds.append(0.5 * (low + high) + 10.0 * extent * direction / np.linalg.norm(direction, axis=1, keepdims=True))
    # the special kinds first, the box filling up the rest
    special = np.concatenate(kinds[1:])
    out = np.concatenate([special, kinds[0]])[:count] if count >= 5 else kinds[0][:count]
    return out.astype(np.float32)
