"""The numpy model of thr3ed_atom_amd/mesh_sign.py and csrc/mesh_sign_kernels.hip (not a test module), on top of
tests/mesh_distance_grad_model.py: the angle-weighted pseudonormal rule of docs/mesh_sign_errors.md -- unit normals, corner angles,
vertex sums, the feature that holds the closest point and the sign of s = dot(p - q, N) -- in float32 operation for operation (atan2
in float64 rounded to float32, the vertex sums in the gather's order) and in float64; the partner table by a dictionary of directed
edges; the error bounds and the decision margin; and an independent truth that shares nothing with the rule: the float64 generalised
winding number (Van Oosterom and Strackee's solid angles, brute force).  The fixtures A - D and their queries are built here."""
import functools

import numpy as np

from tests import mesh_distance_grad_model as GM
from tests import mesh_distance_model as M

U = M.U
FACE, EDGE, VERTEX, NONE = 0, 1, 2, -1
ATAN2_ULPS = 6.0  # the accuracy OpenCL asks of atan2 and the device library documents: 6 ulp <= 12 u |value|


# ---------------------------------------------------------------------------------------------------------------- the tables
def unit_normals(vertices, faces, dtype=np.float64):
    """(n^ [T, 3], len [T]) of unit_normal"""
    v = np.asarray(vertices, dtype=dtype)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = M._cross(b - a, c - a)
    nn = M._dot(n, n)
    length = np.sqrt(nn).astype(dtype)
    with np.errstate(all="ignore"):
        unit = np.where((nn > 0)[:, None], n / length[:, None], 0).astype(dtype)
    return unit, length


def corner_angles(vertices, faces, length, dtype=np.float64):
    """[T, 3]: atan2(len, dot(e1_k, e2_k)) at the corners a, b, c; in float32 the atan2 is float64's rounded"""
    v = np.asarray(vertices, dtype=dtype)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    dots = np.stack([M._dot(b - a, c - a), M._dot(c - b, a - b), M._dot(a - c, b - c)], axis=1).astype(dtype)
    return np.arctan2(length[:, None].astype(np.float64), dots.astype(np.float64)).astype(dtype)


def tables(vertices, faces, dtype=np.float64):
    """dict: normals [T, 3], angles [T, 3], records [T, 9] (alpha_k n^, corner-major), vertex_normals [V, 3]"""
    V, T = len(vertices), len(faces)
    unit, length = unit_normals(vertices, faces, dtype)
    alpha = corner_angles(vertices, faces, length, dtype)
    records = (alpha[:, :, None] * unit[:, None, :]).astype(dtype).reshape(T, 9)
    if dtype == np.float32:
        vertex = GM.vertex_sums32(records, np.arange(T), faces, V)
    else:
        vertex = GM.vertex_sums64(records, np.arange(T), faces, V)[0]
    return {"normals": unit, "angles": alpha, "records": records, "vertex_normals": vertex.astype(dtype)}


def partners(faces):
    """int32 [T, 3] by a dictionary of half-edges: the face across edge k where exactly two faces share it in opposite directions; -1
    boundary, -2 non-manifold, -3 inconsistent"""
    users = {}
    for f, tri in enumerate(faces):
        for k in range(3):
            x, y = int(tri[k]), int(tri[(k + 1) % 3])
            users.setdefault((min(x, y), max(x, y)), []).append((f, k, x < y))
    out = np.zeros((len(faces), 3), np.int32)
    for edge in users.values():
        if len(edge) == 1:
            values = [-1]
        elif len(edge) > 2:
            values = [-2] * len(edge)
        elif edge[0][2] != edge[1][2]:
            values = [edge[1][0], edge[0][0]]
        else:
            values = [-3, -3]
        for (f, k, _), value in zip(edge, values):
            out[f, k] = value
    return out


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- the rule
def features(region, beta):
    """(kind [N], corner [N]): region 3 is the face; a segment whose beta at an end is exactly 1 is that end's vertex, else the edge"""
    region, beta = np.asarray(region), np.asarray(beta)
    x, y = np.minimum(region, 2), np.where(region >= 2, 0, region + 1)
    rows = np.arange(len(region))
    at_x, at_y = beta[rows, x] == 1, beta[rows, y] == 1
    kind = np.where(region == 3, FACE, np.where(at_x | at_y, VERTEX, EDGE))
    corner = np.where(region == 3, 0, np.where(at_x, x, np.where(at_y, y, region)))
    return kind, corner


def signed_distance(points, vertices, faces, face, dtype=np.float64, tabs=None, partner=None, region=None):
    """dict of every query against ITS face ``face`` [N] (all >= 0): signed, s, kind, index, normal [N, 3], r [N, 3], d2, region, beta"""
    tabs = tables(vertices, faces, dtype) if tabs is None else tabs
    partner = partners(faces) if partner is None else partner
    p = np.asarray(points, dtype=dtype).reshape(-1, 3)
    v = np.asarray(vertices, dtype=dtype)
    tri = faces[face]
    d2, q, won, beta = GM.face_gradient(p, v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]], dtype, region)
    kind, corner = features(won, beta)
    rows = np.arange(len(p))
    other = partner[face, np.minimum(corner, 2)]
    unit = tabs["normals"]
    edge_normal = np.where((other >= 0)[:, None], unit[face] + unit[np.maximum(other, 0)], unit[face]).astype(dtype)
    normal = np.where((kind == FACE)[:, None], unit[face], np.where((kind == VERTEX)[:, None], tabs["vertex_normals"][tri[rows, corner]], edge_normal)).astype(dtype)
    index = np.where(kind == FACE, face, np.where(kind == VERTEX, tri[rows, corner], 3 * face + corner))
    r = (p - q).astype(dtype)
    s = M._dot(r, normal)
    d = np.sqrt(d2).astype(dtype)
    return {"signed": np.where(s < 0, -d, d).astype(dtype), "s": s, "kind": kind, "index": index, "normal": normal, "r": r, "d2": d2, "region": won, "beta": beta,
            "partner": other}


def brute(points, vertices, faces, dtype=np.float64):
    """(distance [N], face [N]): the smallest d2 of the rule over all faces, the lowest face on an exact tie"""
    d, face, _ = GM.winners(points, vertices, faces, dtype)
    return d, face


def plane_sign(points, vertices, faces, face):
    """the sign the winning face's plane normal alone gives (float64): what the pseudonormal replaces"""
    p, v = np.asarray(points, np.float64), np.asarray(vertices, np.float64)
    a, b, c = v[faces[face, 0]], v[faces[face, 1]], v[faces[face, 2]]
    return np.where(((p - a) * np.cross(b - a, c - a)).sum(-1) < 0, -1, 1)


# ---------------------------------------------------------------------------------------------------------------- the truth
def winding_number(points, vertices, faces, chunk=512):
    """float64 [N]: sum over the faces of the solid angle they subtend at the query / 4 pi (Van Oosterom and Strackee 1983): 1 inside a
    closed outward-wound surface, 0 outside, 0 again inside a cavity"""
    p, v = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(vertices, np.float64)
    out = np.empty(len(p))
    for first in range(0, len(p), chunk):
        q = p[first:first + chunk, None, :]
        a, b, c = v[faces[:, 0]][None] - q, v[faces[:, 1]][None] - q, v[faces[:, 2]][None] - q
        la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
        numerator = (a * np.cross(b, c)).sum(-1)
        denominator = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[first:first + chunk] = (2.0 * np.arctan2(numerator, denominator)).sum(-1) / (4.0 * np.pi)
    return out


def truth_sign(points, vertices, faces):
    """-1 inside, +1 outside, from the winding number alone"""
    return np.where(winding_number(points, vertices, faces) > 0.5, -1, 1)


# ---------------------------------------------------------------------------------------------------------------- the bounds
def _norm(x):
    return np.sqrt((x * x).sum(-1))


def table_bounds(vertices, faces):
    """(e_normal [T], e_angle [T, 3], e_vertex [V]) of docs/mesh_sign_errors.md: per component, |n^32 - n^| <= e_normal,
    |alpha32 - alpha| <= e_angle, |vertex_normals32 - vertex_normals| <= e_vertex"""
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = _norm(np.cross(b - a, c - a))
    product = _norm(b - a) * _norm(c - a)
    with np.errstate(all="ignore"):
        e_normal = np.where(n > 0, np.minimum(8 * U * product / n + 6 * U, 2.0), 0.0)
        sides = np.stack([_norm(b - a) * _norm(c - a), _norm(c - b) * _norm(a - b), _norm(a - c) * _norm(b - c)], axis=1)
        alpha = np.arctan2(n[:, None], np.stack([((b - a) * (c - a)).sum(-1), ((c - b) * (a - b)).sum(-1), ((a - c) * (b - c)).sum(-1)], axis=1))
        e_angle = np.where(sides > 0, (8 * U * product + 3 * U * n)[:, None] / sides + 4 * U * np.minimum(n[:, None] / sides, 1.0), np.pi) + 2 * ATAN2_ULPS * U * alpha
    e_angle = np.minimum(e_angle, np.pi)
    V = len(v)
    per_corner = e_angle + alpha * e_normal[:, None] + U * alpha  # of one record component (|n^| <= 1)
    e_vertex, magnitude, count = np.zeros(V), np.zeros(V), np.zeros(V)
    for k in range(3):
        np.add.at(e_vertex, faces[:, k], per_corner[:, k])
        np.add.at(magnitude, faces[:, k], alpha[:, k])
        np.add.at(count, faces[:, k], 1.0)
    return e_normal, e_angle, e_vertex + (count + 3.0) * U * magnitude


def decision_margin(points, vertices, faces, face, result, bounds=None):
    """[N]: the |s| above which float32 cannot flip the sign for the feature ``result`` (a dict of ``signed_distance``) names:
    m = sum_j (|r_j| e_N + e_r |N_j|) + 3 e_r e_N + 3 u sum_j |r_j N_j| with e_r = b(p, f) + 2 u W the forward's point error and e_N the
    bound of the feature's normal"""
    e_normal, _, e_vertex = table_bounds(vertices, faces) if bounds is None else bounds
    p, v = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(vertices, np.float64)
    tri = faces[face]
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    W = np.maximum(np.maximum(_norm(p - a), _norm(p - b)), _norm(p - c))
    b_face = M.face_bounds(p, v, faces)[np.arange(len(p)), face]
    e_r = b_face + 2 * U * W
    kind, index, other = result["kind"], result["index"], result["partner"]
    e_edge = e_normal[face] + np.where(other >= 0, e_normal[np.maximum(other, 0)], 0.0) + 2 * U
    e_N = np.where(kind == FACE, e_normal[face], np.where(kind == VERTEX, e_vertex[np.where(kind == VERTEX, index, 0)], e_edge))
    r, N = np.abs(np.asarray(result["r"], np.float64)), np.abs(np.asarray(result["normal"], np.float64))
    return (r * e_N[:, None] + e_r[:, None] * N).sum(-1) + 3 * e_r * e_N + 3 * U * (r * N).sum(-1)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _box(low, high, inward=False):
    (x0, y0, z0), (x1, y1, z1) = low, high
    v = np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, (f[:, [0, 2, 1]] if inward else f)


def cube():
    """(A) the unit cube, 12 faces"""
    return _box((0, 0, 0), (1, 1, 1))


def cube_with_cavity():
    """(B) the unit cube with an inverted inner cube [0.25, 0.75]^3 as a cavity, 24 faces"""
    v, f = _box((0, 0, 0), (1, 1, 1))
    w, g = _box((0.25, 0.25, 0.25), (0.75, 0.75, 0.75), inward=True)
    return np.concatenate([v, w]), np.concatenate([f, g + len(v)])


def icosphere():
    """(C) 320 faces on the unit sphere"""
    v, f = M.icosphere(2)
    return (v, f) if signed_volume(v, f) > 0 else (v, f[:, [0, 2, 1]])


def prism_with_spike():
    """(D) an L-shaped prism -- the reflex edge runs from (1, 1, 0) to (1, 1, 1) -- whose top carries one thin spike: a top triangle is
    replaced by a ring of six faces round a small triangle and the three faces from that to an apex one unit above"""
    outline = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    n = len(outline)
    v = [(x, y, 0.0) for x, y in outline] + [(x, y, 1.0) for x, y in outline]
    fans = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]
    f = [(i, k, j) for i, j, k in fans]  # the bottom looks down
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, j + n), (i, j + n, i + n)]
    top = [(i + n, j + n, k + n) for i, j, k in fans]
    A, B, C = top[0]
    centre = (np.array(v[A]) + np.array(v[B]) + np.array(v[C])) / 3.0
    small = [tuple(centre + 0.05 * (np.array(v[k]) - centre)) for k in (A, B, C)]
    a, b, c = len(v), len(v) + 1, len(v) + 2
    v += small + [tuple(centre + np.array([0.03, 0.02, 1.0]))]
    S = len(v) - 1
    f += top[1:] + [(A, B, b), (A, b, a), (B, C, c), (B, c, b), (C, A, a), (C, a, c), (a, b, S), (b, c, S), (c, a, S)]
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int64)


MESHES = {"cube": cube, "cavity": cube_with_cavity, "icosphere": icosphere, "prism": prism_with_spike}
RANDOM, OFFSET = 4096, 0.05


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(vertices, faces, queries float32 [N, 3], groups): 4096 seeded uniform points in 1.5 x the mesh's box, then for every vertex, every
    edge midpoint and every face centroid the point itself and the point +- 0.05 x its unit float64 pseudonormal.  ``groups``: the
    slices "random", "on" (the feature points themselves) and "off" (the offset ones)"""
    v, f = MESHES[name]()
    rng = np.random.default_rng(sum(name.encode()))
    v64 = v.astype(np.float64)
    low, high = v64.min(0), v64.max(0)
    centre, half = (low + high) / 2, 1.5 * (high - low) / 2
    random = rng.uniform(centre - half, centre + half, size=(RANDOM, 3))
    tabs = tables(v, f)
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-300)  # noqa: E731
    partner = partners(f)
    on, normal = [v64, v64[f].mean(1)], [unit(tabs["vertex_normals"]), tabs["normals"]]
    for k in range(3):
        own = partner[:, k] > np.arange(len(f))  # each edge once
        on.append(0.5 * (v64[f[own, k]] + v64[f[own, (k + 1) % 3]]))
        normal.append(unit(tabs["normals"][own] + tabs["normals"][partner[own, k]]))
    on, normal = np.concatenate(on), np.concatenate(normal)
    queries = np.concatenate([random, on, on + OFFSET * normal, on - OFFSET * normal]).astype(np.float32)
    groups = {"random": slice(0, RANDOM), "on": slice(RANDOM, RANDOM + len(on)), "off": slice(RANDOM + len(on), len(queries))}
    for array in (v, f, queries):
        array.setflags(write=False)
    return v, f, queries, groups


@functools.lru_cache(maxsize=None)
def reference(name):
    """per fixture, computed once and left unchanged: dict with the float64 brute force (distance, face), the float64 rule's result
    against it, the winding-number sign, the forward's distance bound B and the decision margin of the float64 result"""
    v, f, q, _ = fixture(name)
    d, face = brute(q, v, f)
    result = signed_distance(q, v, f, face)
    out = {"distance": d, "face": face, "result": result, "truth": truth_sign(q, v, f), "B": M.bound(q, v, f), "margin": decision_margin(q, v, f, face, result)}
    for value in list(out.values()) + list(result.values()):
        if isinstance(value, np.ndarray):
            value.setflags(write=False)
    return out
