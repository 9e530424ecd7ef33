"""numpy float64 model of ``rf.simplify_mesh``, written from the contract and not from the kernels, with the
meshes the tests use and the error bound of docs/mesh_simplify_errors.md.

THE CONTRACT.  h = float32(cell_size) > 0, r = float32(1) / h (float32), o = the origin as float32 (default: the per-axis minimum
of the vertices).  Cell of vertex v: k_a = floor(fl32(fl32(v_a - o_a) * r)); n_a = max k_a + 1; key = (k_x n_y + k_y) n_z + k_z.
Clusters = the distinct keys, ascending.  In float64, local to the cell centre m = o + (k + 1/2) h: every face corner (f, j) whose
vertex lies in the cluster adds, with q_i = p_i - m, n = (q1 - q0) x (q2 - q0) and d = n . q0:  A += n n^T, b += d n, c += d^2.
xbar = the mean of the members' q.  placement "mean" or tr A == 0: x = xbar; else x = xbar + (A + lambda tr(A) I)^-1 (b - A xbar)
(adjugate over determinant), clamped per axis to [-h/2, h/2].  Output vertex float32(m + x); colour = the mean of the members'
colours; normal = the members' normal sum over its norm, (0, 0, 0) where the sum is 0.  Faces: map to clusters, drop those with two
equal indices, rotate the smallest index to the front, merge exact duplicates, sort lexicographically; clusters that no kept face
uses are dropped, the rest in ascending key order are the output vertices.

THE BOUND (per output coordinate, against the model's UNROUNDED float64 value; u = 2^-53).  Kernel and model evaluate every
record's terms by the same IEEE float64 operations in the same order, so the terms agree and only the ORDER of the sums differs:
two orders of a sum of L terms differ by at most eps(L) * sum |t_i|, eps(L) = 2 (L + 16) u (the 16: head-room for the handful of
roundings per term, should a compiler evaluate one differently).  With L_c corner and L_m member records, kappa = (1 + lambda) /
lambda >= cond(M), delta the model's unclamped step and R_m = the largest |q| of a member:
    E_mean  = eps(L_m) * R_m                                              (sum |q_a| <= L_m R_m, divided by L_m)
    E_rhs   = sqrt(3) eps(L_c) B + 3 eps(L_c) tr(A) |xbar| + sqrt(3) tr(A) E_mean + 8 u (|b| + tr(A) |xbar|)
              with B = sum |d| |n| over the records  (sum |n_a n_b| <= tr A bounds every entry of A's error by eps(L_c) tr A)
    E_delta = E_rhs / (lambda tr A)  +  2 kappa (9 eps(L_c) + 32 u kappa) |delta|
              (|M^-1| <= 1 / (lambda tr A);  |dM| / |M| <= 3 eps tr A / (tr A / 3);  adjugate / determinant of a 3 x 3 matrix loses at
              most a factor kappa over a backward-stable solve: minors err by O(u |M|^2) against |adj M| = l1 l2)
    E64     = E_mean + E_delta + 4 u (|m| + h)
The clamp is 1-Lipschitz, so it does not enlarge E64.  The float32 result then lies within E64 + 2^-24 (|x64| + E64) of the model's
float64 coordinate (half a float32 ulp of the value that is rounded).  Colours: eps(L_m) * mean |c| + half an ulp.  Normals:
(2 sqrt(3) eps(L_m) max_a sum |n_a| / |s| + 8 u) + half an ulp of 1."""
from typing import NamedTuple, Optional

import numpy as np

U = 2.0 ** -53
HALF_ULP32 = 2.0 ** -24
MAX_CELLS = 1 << 20
MAX_TARGET_RESOLUTION = 4096


# ---------------------------------------------------------------------------------------------------------------- meshes

def uv_sphere(n_lat: int, n_lon: int, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """closed, outward-oriented: two poles and n_lat - 1 rings of n_lon vertices; 2 n_lon (n_lat - 1) faces"""
    theta = np.pi * np.arange(1, n_lat) / n_lat
    phi = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None], np.sin(theta)[:, None] * np.sin(phi)[None], np.cos(theta)[:, None] * np.ones(n_lon)[None]], -1)
    unit = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    at = lambda i, j: 1 + i * n_lon + j % n_lon
    south = 1 + (n_lat - 1) * n_lon
    faces = []
    for j in range(n_lon):
        faces.append((0, at(0, j), at(0, j + 1)))
        for i in range(n_lat - 2):
            faces += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
        faces.append((south, at(n_lat - 2, j + 1), at(n_lat - 2, j)))
    vertices = (unit * radius + np.asarray(centre, dtype=np.float64)).astype(np.float32)
    return vertices, np.asarray(faces, dtype=np.int64), unit.astype(np.float32)


def cube_surface(n: int, low=-1.0, high=1.0, shift=0.0):
    """the welded surface of the cube [low, high]^3 + shift with n x n quads (2 n^2 triangles) per face, outward-oriented"""
    index, points, faces = {}, [], []

    def vertex(ijk):
        if ijk not in index:
            index[ijk] = len(points)
            points.append([low + (high - low) * t / n + shift for t in ijk])
        return index[ijk]

    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        ijk = [0, 0, 0]
                        ijk[axis], ijk[b], ijk[c] = side * n, i + di, j + dj
                        return vertex(tuple(ijk))
                    p00, p10, p11, p01 = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    quads = [(p00, p10, p11), (p00, p11, p01)]  # e_b x e_c = e_axis
                    faces += quads if side else [(x, z, y) for x, y, z in quads]
    return np.asarray(points, dtype=np.float32), np.asarray(faces, dtype=np.int64)


def plane_patch(n: int, normal=(0.3, -0.5, 0.8), offset=0.21, size=1.0):
    """an n x n-quad patch of the plane {x : normal . x = offset |normal|}, tilted against every axis (float32 vertices: each lies
    within float32 rounding of the plane)"""
    nrm = np.asarray(normal, dtype=np.float64)
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    s = size * (np.arange(n + 1) / n - 0.5)
    points = offset * nrm + s[:, None, None] * e1 + s[None, :, None] * e2
    at = lambda i, j: i * (n + 1) + j
    faces = []
    for i in range(n):
        for j in range(n):
            faces += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    return points.reshape(-1, 3).astype(np.float32), np.asarray(faces, dtype=np.int64), nrm


def triangle_fan(k: int, centre=(0.0, 0.0, 0.0), radius=1.0, lift=0.3):
    """k triangles around vertex 0 (k >= 1; a closed umbrella from k >= 3, an open fan below): vertex 0 has exactly k corners"""
    closed = k >= 3
    rim = k if closed else k + 1
    phi = 2 * np.pi * np.arange(rim) / max(rim, 3)
    points = np.concatenate([[[0.0, 0.0, lift]], np.stack([np.cos(phi), np.sin(phi), 0.1 * np.cos(3 * phi)], -1) * radius])
    faces = [(0, 1 + j, 1 + (j + 1) % rim) for j in range(k)]
    return (points + np.asarray(centre, dtype=np.float64)).astype(np.float32), np.asarray(faces, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- the model

class Lattice(NamedTuple):
    origin: np.ndarray  # float32 [3]
    h: np.float32
    r: np.float32
    cells: np.ndarray   # int64 [3]
    k: np.ndarray       # int64 [V, 3]
    keys: np.ndarray    # int64 [V]


class Simplified(NamedTuple):
    vertices: np.ndarray            # float32 [V_out, 3]
    faces: np.ndarray               # int64 [T_out, 3]
    colours: Optional[np.ndarray]   # float32
    normals: Optional[np.ndarray]   # float32
    vertices64: np.ndarray          # the unrounded values, and the bound on |float32 result - them| per coordinate
    vertex_bound: np.ndarray
    colours64: Optional[np.ndarray]
    colour_bound: Optional[np.ndarray]
    normals64: Optional[np.ndarray]
    normal_bound: Optional[np.ndarray]
    cell_size: float
    keys: np.ndarray                # int64 [V_in]
    cluster_keys: np.ndarray        # int64 [C]: every cluster, ascending
    vertex_keys: np.ndarray         # int64 [V_out]: the keys of the output vertices
    clusters: int
    input_faces: int
    collapsed_faces: int
    merged_duplicates: int
    cluster_of_vertex: np.ndarray   # int64 [V_in]
    quadric_c: np.ndarray           # float64 [V_out]: sum d^2 (the constant of the quadric; no output depends on it)
    corner_records: np.ndarray      # int64 [C], member_records likewise: the segment lengths of every cluster
    member_records: np.ndarray
    every_cluster: tuple            # (vertices64, vertex_bound, colours64, colour_bound, normals64, normal_bound) of ALL C clusters


def lattice_of(vertices, cell_size, origin=None) -> Lattice:
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertices")
    h = np.float32(cell_size)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("cell_size")
    r = np.float32(1.0) / h
    o = v.min(axis=0) if origin is None else np.asarray(origin, dtype=np.float32)
    if (v < o).any():
        raise ValueError("vertices below the origin")
    k = np.floor(((v - o).astype(np.float32) * r).astype(np.float32)).astype(np.int64)
    cells = k.max(axis=0) + 1
    if (cells > MAX_CELLS).any():
        raise ValueError("more than 2^20 cells along an axis")
    return Lattice(o, h, r, cells, k, (k[:, 0] * cells[1] + k[:, 1]) * cells[2] + k[:, 2])


def canonical_faces(cluster, faces):
    """(faces over cluster indices in canonical form, number that survived the collapse)"""
    mapped = cluster[faces]
    mapped = mapped[(mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])]
    first = mapped.argmin(axis=1)
    mapped = np.take_along_axis(mapped, (first[:, None] + np.arange(3)) % 3, axis=1)
    unique = np.unique(mapped, axis=0) if len(mapped) else mapped.reshape(0, 3)  # (sorted lexicographically)
    return unique, len(mapped)


def face_count(vertices, faces, cell_size, origin=None) -> int:
    lat = lattice_of(vertices, cell_size, origin)
    return len(canonical_faces(np.unique(lat.keys, return_inverse=True)[1].reshape(-1), faces)[0])


def target_cell_size(vertices, faces, target_faces: int, origin=None) -> np.float32:
    """the bisection that defines ``target_faces``"""
    v = np.asarray(vertices, dtype=np.float32)
    extent = np.float32((v.max(axis=0) - v.min(axis=0)).max())
    assert extent > 0
    size = lambda n: np.float32(float(extent) / n)
    count = lambda n: face_count(v, faces, size(n), origin)
    lo, hi = 1, MAX_TARGET_RESOLUTION
    if count(hi) <= target_faces:
        return size(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= target_faces:
            lo = mid
        else:
            hi = mid
    return size(lo)


def eps(length):
    return 2.0 * (np.asarray(length, dtype=np.float64) + 16.0) * U


def simplify(vertices, faces, cell_size=None, *, target_faces=None, origin=None, placement="quadric", regularisation=1e-3, colours=None,
             normals=None) -> Simplified:
    assert (cell_size is None) != (target_faces is None) and placement in ("quadric", "mean") and 1e-6 <= regularisation <= 1.0
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, T = len(v32), len(faces)
    if T and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("faces index outside the vertices")
    if target_faces is not None:
        cell_size = target_cell_size(v32, faces, target_faces, origin)
    lat = lattice_of(v32, cell_size, origin)
    cluster_keys, cluster = np.unique(lat.keys, return_inverse=True)
    cluster = cluster.reshape(-1)
    C = len(cluster_keys)
    h, lam = float(lat.h), float(np.float32(regularisation))
    kz, rest = cluster_keys % lat.cells[2], cluster_keys // lat.cells[2]
    k = np.stack([rest // lat.cells[1], rest % lat.cells[1], kz], -1)
    m = lat.origin.astype(np.float64) + (k.astype(np.float64) + 0.5) * h  # [C, 3]
    p = v32.astype(np.float64)

    # corner records, in corner order 3 f + j
    rec_cluster = cluster[faces.reshape(-1)]
    rec_face = np.repeat(np.arange(T), 3)
    mc = m[rec_cluster]
    q0, q1, q2 = (p[faces[rec_face, i]] - mc for i in range(3))
    e1, e2 = q1 - q0, q2 - q0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
    d = n[:, 0] * q0[:, 0] + n[:, 1] * q0[:, 1] + n[:, 2] * q0[:, 2]
    A = np.zeros((C, 3, 3))
    b, c, B = np.zeros((C, 3)), np.zeros(C), np.zeros(C)
    np.add.at(A, rec_cluster, n[:, :, None] * n[:, None, :])
    np.add.at(b, rec_cluster, d[:, None] * n)
    np.add.at(c, rec_cluster, d * d)
    np.add.at(B, rec_cluster, np.abs(d) * np.linalg.norm(n, axis=1))
    corner_records = np.bincount(rec_cluster, minlength=C)

    # member records
    q = p - m[cluster]
    member_records = np.bincount(cluster, minlength=C)
    sum_q, R_m = np.zeros((C, 3)), np.zeros(C)
    np.add.at(sum_q, cluster, q)
    np.maximum.at(R_m, cluster, np.linalg.norm(q, axis=1))
    xbar = sum_q / member_records[:, None]
    tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    solve = (tr != 0.0) if placement == "quadric" else np.zeros(C, dtype=bool)
    x, delta = xbar.copy(), np.zeros((C, 3))
    kappa = (1.0 + lam) / lam
    E_mean = eps(member_records) * R_m
    E_delta = np.zeros(C)
    if solve.any():
        As, trs, xs = A[solve], tr[solve], xbar[solve]
        M = As + (lam * trs)[:, None, None] * np.eye(3)
        rhs = b[solve] - np.einsum("cij,cj->ci", As, xs)
        adj = np.empty_like(M)
        adj[:, 0, 0] = M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 1, 2]
        adj[:, 0, 1] = adj[:, 1, 0] = M[:, 0, 2] * M[:, 1, 2] - M[:, 0, 1] * M[:, 2, 2]
        adj[:, 0, 2] = adj[:, 2, 0] = M[:, 0, 1] * M[:, 1, 2] - M[:, 0, 2] * M[:, 1, 1]
        adj[:, 1, 1] = M[:, 0, 0] * M[:, 2, 2] - M[:, 0, 2] * M[:, 0, 2]
        adj[:, 1, 2] = adj[:, 2, 1] = M[:, 0, 1] * M[:, 0, 2] - M[:, 0, 0] * M[:, 1, 2]
        adj[:, 2, 2] = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 0, 1]
        det = M[:, 0, 0] * adj[:, 0, 0] + M[:, 0, 1] * adj[:, 0, 1] + M[:, 0, 2] * adj[:, 0, 2]
        step = np.einsum("cij,cj->ci", adj, rhs) / det[:, None]
        delta[solve] = step
        x[solve] = np.clip(xs + step, -0.5 * h, 0.5 * h)
        ec, norm_x = eps(corner_records[solve]), np.linalg.norm(xs, axis=1)
        E_rhs = np.sqrt(3.0) * ec * B[solve] + 3.0 * ec * trs * norm_x + np.sqrt(3.0) * trs * E_mean[solve] + 8.0 * U * (np.linalg.norm(b[solve], axis=1) + trs * norm_x)
        assert (2.0 * kappa * (9.0 * ec + 32.0 * U * kappa) < 0.5).all()  # the first-order bound is valid (segments under 1e8 records at lambda = 1e-6)
        E_delta[solve] = E_rhs / (lam * trs) + 2.0 * kappa * (9.0 * ec + 32.0 * U * kappa) * np.linalg.norm(step, axis=1)
    E64 = E_mean + E_delta + 4.0 * U * (np.abs(m).max(axis=1) + h)
    out64 = m + x
    bound = E64[:, None] + HALF_ULP32 * (np.abs(out64) + E64[:, None])

    def averaged(values):
        if values is None:
            return None, None
        w = np.asarray(values, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        total, absolute = np.zeros((C, 3)), np.zeros((C, 3))
        np.add.at(total, cluster, w)
        np.add.at(absolute, cluster, np.abs(w))
        return total, absolute

    col64 = col_bound = nrm64 = nrm_bound = None
    if colours is not None:
        total, absolute = averaged(colours)
        col64 = total / member_records[:, None]
        col_bound = eps(member_records)[:, None] * absolute / member_records[:, None] + HALF_ULP32 * np.abs(col64) * (1 + 1e-6)
    if normals is not None:
        total, absolute = averaged(normals)
        length = np.sqrt(total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1] + total[:, 2] * total[:, 2])
        safe = np.where(length == 0.0, 1.0, length)
        nrm64 = np.where((length == 0.0)[:, None], 0.0, total / safe[:, None])
        nrm_bound = np.where(length == 0.0, 0.0, 2.0 * np.sqrt(3.0) * eps(member_records) * absolute.max(axis=1) / safe + 8.0 * U + HALF_ULP32 * (1 + 1e-6))[:, None] * np.ones(3)

    kept_faces, kept = canonical_faces(cluster, faces)
    used = np.zeros(C, dtype=bool)
    used[kept_faces.reshape(-1)] = True
    position = np.where(used, np.cumsum(used) - 1, -1)
    pick = lambda a: None if a is None else a[used]
    f32 = lambda a: None if a is None else a.astype(np.float32)
    return Simplified(out64[used].astype(np.float32), position[kept_faces].reshape(-1, 3), f32(pick(col64)), f32(pick(nrm64)), out64[used], bound[used], pick(col64),
                      pick(col_bound), pick(nrm64), pick(nrm_bound), h, lat.keys, cluster_keys, cluster_keys[used], C, T, T - kept, kept - len(kept_faces),
                      position[cluster], c[used], corner_records, member_records, (out64, bound, col64, col_bound, nrm64, nrm_bound))


# ---------------------------------------------------------------------------------------------------------------- comparison

def compare_values(triples):
    """(name, result, float64 model, bound) rows -> the list of differences"""
    problems = []
    for name, got, want, bound in triples:
        if (got is None) != (want is None):
            problems.append(f"{name}: present in one result only")
        elif got is not None:
            got = np.asarray(got)
            if got.shape != want.shape or got.dtype != np.float32:
                problems.append(f"{name}: shape / dtype {got.shape} {got.dtype}, the model has {want.shape}")
                continue
            err = np.abs(got.astype(np.float64) - want)
            bad = ~(err <= bound)  # (NaN fails)
            if bad.any():
                i = int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0).max(axis=1)))
                problems.append(f"{name}: {int(bad.sum())} coordinates beyond the bound, worst row {i}: error {err[i].tolist()} bound {bound[i].tolist()}")
    return problems


def compare_clusters(model: Simplified, vertices, colours=None, normals=None):
    """the representatives of ALL clusters (used by a face or not) against the model"""
    v64, vb, c64, cb, n64, nb = model.every_cluster
    return compare_values((("cluster vertices", vertices, v64, vb), ("cluster colours", colours, c64, cb), ("cluster normals", normals, n64, nb)))


def compare(model: Simplified, vertices, faces, colours=None, normals=None, cluster_of_vertex=None, counts=None):
    """every way in which a result differs from the model (an empty list: it matches): topology exactly, positions and attributes
    within the model's bound.  ``counts`` = (clusters, vertices, input_faces, collapsed_faces, merged_duplicates, faces)."""
    problems = []
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    if faces.shape != model.faces.shape or faces.dtype != np.int64:
        problems.append(f"faces: shape / dtype {faces.shape} {faces.dtype}, the model has {model.faces.shape} int64")
    elif not np.array_equal(faces, model.faces):
        problems.append(f"faces: first difference in row {int(np.nonzero((faces != model.faces).any(axis=1))[0][0])}")
    if cluster_of_vertex is not None and not np.array_equal(np.asarray(cluster_of_vertex), model.cluster_of_vertex):
        problems.append("cluster_of_vertex differs")
    if counts is not None:
        expected = (model.clusters, len(model.vertices), model.input_faces, model.collapsed_faces, model.merged_duplicates, len(model.faces))
        if tuple(int(v) for v in counts) != expected:
            problems.append(f"counts {tuple(counts)} != {expected}")
    problems += compare_values((("vertices", vertices, model.vertices64, model.vertex_bound), ("colours", colours, model.colours64, model.colour_bound),
                                ("normals", normals, model.normals64, model.normal_bound)))
    return problems


def error_ratio(model: Simplified, vertices) -> float:
    """the largest |result - model| / bound over the coordinates (what docs/mesh_simplify_errors.md tabulates)"""
    if not len(model.vertices64):
        return 0.0
    return float((np.abs(np.asarray(vertices, dtype=np.float64) - model.vertices64) / model.vertex_bound).max())


def directed_edge_balance(faces) -> bool:
    """every directed edge (a, b) occurs exactly as often as (b, a)"""
    faces = np.asarray(faces, dtype=np.int64)
    if not len(faces):
        return True
    edges = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    top = int(faces.max()) + 1
    forward, f_counts = np.unique(edges[:, 0] * top + edges[:, 1], return_counts=True)
    backward, b_counts = np.unique(edges[:, 1] * top + edges[:, 0], return_counts=True)
    return np.array_equal(forward, backward) and np.array_equal(f_counts, b_counts)
