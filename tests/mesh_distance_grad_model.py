"""The numpy model of thr3ed_atom_amd/mesh_distance_grad.py and csrc/mesh_distance_grad_kernels.hip (not a test module), on top of
tests/mesh_distance_model.py: which candidate of the distance rule wins (the region), the barycentrics beta of the closest point, the
unit vector u, the gradient on the query and the 9-float corner records of docs/mesh_distance_grad_errors.md -- in float32 operation
for operation (numpy rounds every float32 operation and fuses none, as the kernel built with -ffp-contract=off) and in float64 for
reference values --, the two segmented sums in the gather's order (tests/segment_sum_model.py), the derived error bounds, the Chamfer
loss and the loop of ``fit_mesh_to_mesh`` with Adam.  ``variant`` selects the BROKEN models the CPU tests reject."""
import numpy as np

from tests import mesh_distance_model as M
from tests import segment_sum_model as SEG

U = M.U
TRIANGLE = (np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------- the rule
def _segment(p, s, e, lo, hi):
    """(d2, q, t) of one segment: the operations of dist_segment"""
    g, w = e - s, p - s
    l = M._dot(g, g)
    with np.errstate(all="ignore"):
        t = np.where(l > 0, np.fmin(np.fmax(M._dot(w, g) / l, 0), 1), 0).astype(p.dtype)
    d2, q = M._candidate(p, s + t[..., None] * g, lo, hi)
    return d2, q, t


def face_gradient(p, a, b, c, dtype=np.float64, region=None, variant=None):
    """(d2, q, region, beta [..., 3]) of queries ``p`` against triangles (a, b, c), arrays of [..., 3] that broadcast.  ``region`` None: the
    winner of the forward rule's order with its strict <; an integer array: that candidate is taken whatever its d2 (the float64
    reference is given the kernel's region).  ``variant`` "corner order": beta of the corners rotated by one (BROKEN)."""
    p, a, b, c = (np.asarray(x, dtype=dtype) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    one, zero = dtype(1), np.zeros(p.shape[:-1], dtype)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    forced = None if region is None else np.broadcast_to(np.asarray(region), p.shape[:-1])
    best, point, t = _segment(p, a, b, lo, hi)
    won = np.zeros(p.shape[:-1], np.int64)
    for k, (s, e) in ((1, (b, c)), (2, (c, a))):
        d2, q, tk = _segment(p, s, e, lo, hi)
        take = d2 < best if forced is None else forced == k
        best, point, t, won = np.where(take, d2, best), np.where(take[..., None], q, point), np.where(take, tk, t), np.where(take, k, won)
    s1 = (one - t).astype(dtype)
    beta = np.stack([np.where(won == 0, s1, np.where(won == 2, t, zero)), np.where(won == 1, s1, np.where(won == 0, t, zero)),
                     np.where(won == 2, s1, np.where(won == 1, t, zero))], axis=-1)
    n = M._cross(b - a, c - a)
    nn = M._dot(n, n)
    with np.errstate(all="ignore"):
        s = M._dot(p - a, n) / nn
        q = p - s[..., None] * n
        e_ab, e_bc, e_ca = M._dot(M._cross(b - a, q - a), n), M._dot(M._cross(c - b, q - b), n), M._dot(M._cross(a - c, q - c), n)
        inside = (nn > 0) & (e_ab >= 0) & (e_bc >= 0) & (e_ca >= 0)
        d2, qc = M._candidate(p, q, lo, hi)
        S = (e_ab + e_bc) + e_ca
        take = inside & (d2 < best) & (S > 0) if forced is None else forced == 3
        plane_beta = np.stack([e_bc / S, e_ca / S, e_ab / S], axis=-1)
    best, point, won = np.where(take, d2, best), np.where(take[..., None], qc, point), np.where(take, 3, won)
    beta = np.where(take[..., None], plane_beta, beta).astype(dtype)
    if variant == "corner order":
        beta = np.roll(beta, 1, axis=-1)
    return best, point, won, beta


def gradients(p, a, b, c, G, dtype=np.float64, region=None, variant=None):
    """dict of one query batch against its faces: d2, q, region, beta, u [N, 3], grad_points [N, 3] = G u, records [N, 9] = -beta_k G u
    (corner-major).  ``variant`` "q for r": q in place of p - q (BROKEN)."""
    d2, q, won, beta = face_gradient(p, a, b, c, dtype, region, variant)
    p = np.broadcast_to(np.asarray(p, dtype=dtype), q.shape)
    r = (p - q) if variant != "q for r" else q
    length = np.sqrt(M._dot(r, r))
    with np.errstate(all="ignore"):
        u = np.where((length > 0)[..., None], r / length[..., None], 0).astype(dtype)
    gp = np.where((length > 0)[..., None], np.asarray(G, dtype=dtype)[..., None] * u, 0).astype(dtype)  # (+0 on the surface, whatever G's sign)
    records = (-(beta[..., :, None] * gp[..., None, :])).astype(dtype)
    return {"d2": d2, "q": q, "region": won, "beta": beta, "u": u, "grad_points": gp, "records": records.reshape(*records.shape[:-2], 9)}


def winners(points, vertices, faces, dtype=np.float64):
    """(distance [N], face [N], region [N]) of the brute force over all faces: the smallest d2, the lowest face on an exact tie"""
    points = np.asarray(points, dtype=dtype).reshape(-1, 3)
    v = np.asarray(vertices, dtype=dtype)
    d2, _, region, _ = face_gradient(points[:, None, :], v[faces[:, 0]][None], v[faces[:, 1]][None], v[faces[:, 2]][None], dtype)
    face = np.argmin(d2, axis=1)
    rows = np.arange(len(points))
    return np.sqrt(d2[rows, face]), face, region[rows, face]


def query_gradients(points, vertices, faces, face, G, dtype=np.float64, region=None, variant=None):
    """``gradients`` of every query against ITS face ``face`` [N] (rows with face -1: zeros, region -1)"""
    points = np.asarray(points, dtype=dtype).reshape(-1, 3)
    v = np.asarray(vertices, dtype=dtype)
    has = face >= 0
    f = faces[np.where(has, face, 0)]
    out = gradients(points, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]], G, dtype, region, variant)
    for key in ("beta", "u", "grad_points", "records"):
        out[key] = np.where(has[:, None], out[key], 0).astype(dtype)
    out["region"] = np.where(has, out["region"], -1)
    return out


# ---------------------------------------------------------------------------------------------------------------- the two sums
def gather_lists(face, faces, V):
    """(entries [hits], face_offsets [T + 1], corner_slots [3 T], vertex_offsets [V + 1]): the lists of the binding"""
    T = len(faces)
    entry = np.nonzero(face >= 0)[0]
    entries = entry[np.argsort(face[entry], kind="stable")]
    face_offsets = np.concatenate([[0], np.cumsum(np.bincount(face[entry], minlength=T))]).astype(np.int64)
    flat = faces.reshape(-1)
    slots = np.argsort(flat, kind="stable")
    vertex_offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))]).astype(np.int64)
    return entries, face_offsets, slots, vertex_offsets


def vertex_sums32(records, face, faces, V, threshold=16):
    """float32 [V, 3]: the gather's two segmented sums of float32 ``records`` [N, 9], its additions in its order (the BITS).  The kernel's
    accumulators start from +0, so a sum whose terms are all -0 -- the records of a query on the surface -- is +0; the replay starts
    from its first term, and adding +0 at the end makes the two agree (x + 0 = x for every other x)."""
    entries, face_offsets, slots, vertex_offsets = gather_lists(face, faces, V)
    return SEG.replay_mesh(np.asarray(records, np.float32), entries, face_offsets, slots, vertex_offsets, threshold)[1] + np.float32(0.0)


def vertex_sums64(records, face, faces, V):
    """(float64 [V, 3] sums, [V, 3] sums of magnitudes, [V] the n of the bound): a plain scatter of ``records`` [N, 9] onto the corners"""
    records = np.asarray(records, np.float64).reshape(-1, 3, 3)
    total, magnitude, count = np.zeros((V, 3)), np.zeros((V, 3)), np.bincount(faces.reshape(-1), minlength=V).astype(np.float64)
    has = face >= 0
    for k in range(3):
        np.add.at(total, faces[face[has], k], records[has, k])
        np.add.at(magnitude, faces[face[has], k], np.abs(records[has, k]))
        np.add.at(count, faces[face[has], k], 1.0)
    return total, magnitude, count


def sum_bound(count, magnitude):
    """(n + 3) u sum |terms| per vertex (docs/texture_fit_errors.md); n = the records that reach the vertex + its corner slots"""
    return (np.asarray(count, np.float64)[:, None] + 3.0) * U * magnitude


# ---------------------------------------------------------------------------------------------------------------- the bounds
def bounds(points, vertices, faces, face, region, G, length64, beta64):
    """(e_u [N], e_beta [N], e_points [N], e_records [N, 3]) of docs/mesh_distance_grad_errors.md for queries against THEIR face under
    the given region: |u32 - u64|_inf <= e_u, |beta32 - beta64|_inf <= e_beta, |grad_points32 - grad_points64|_inf <= e_points,
    |records32 - records64|_inf of corner k <= e_records[:, k]"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(vertices, np.float64)
    f = faces[np.maximum(face, 0)]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    norm = lambda x: np.sqrt((x * x).sum(-1))  # noqa: E731
    bq = np.array([M.face_bounds(p[i], v, faces[max(face[i], 0)][None])[0, 0] for i in range(len(p))]) if len(p) else np.zeros(0)
    W = np.maximum(np.maximum(norm(p - a), norm(p - b)), norm(p - c))
    L = np.maximum(np.maximum(norm(b - a), norm(c - b)), norm(a - c))
    with np.errstate(all="ignore"):
        e_u = np.minimum(np.where(length64 > 0, 2.0 * (bq + 2 * U * W) / length64, np.inf) + 8 * U, 2.0)
        g = np.where(region == 0, norm(b - a), np.where(region == 1, norm(c - b), norm(a - c)))
        e_segment = np.where(g > 0, np.minimum(7 * U * (W + L) / g, 1.0), 0.0) + U
        n = norm(np.cross(b - a, c - a))
        theta = np.where(n > 0, np.minimum(8 * U * norm(b - a) * norm(c - a) / n, 1.0), 0.0)
        e_plane = np.where(n > 0, 4 * L * (bq + 2 * L * (theta + 8 * U)) / n, np.inf) + 2 * U
    e_beta = np.where(region == 3, e_plane, e_segment)
    G = np.abs(np.asarray(G, np.float64))
    e_points = G * (e_u + 2 * U)
    e_records = G[:, None] * (e_beta[:, None] + (np.abs(beta64) + e_beta[:, None]) * e_u[:, None] + 3 * U)
    return e_u, e_beta, e_points, e_records


# ---------------------------------------------------------------------------------------------------------------- loss and fit
def surface_points(vertices, faces, sample_faces, barycentrics, dtype=np.float64):
    v = np.asarray(vertices, dtype=dtype)[faces[sample_faces]]
    b = np.asarray(barycentrics, dtype=dtype)
    return ((b[:, 0:1] * v[:, 0] + b[:, 1:2] * v[:, 1]) + b[:, 2:3] * v[:, 2]).astype(dtype)


def surface_points_backward(grad, faces, sample_faces, barycentrics, V):
    """float64 [V, 3] and the sum bound's (magnitude, n): the adjoint of ``surface_points`` as a plain scatter of the records b_k g"""
    records = (np.asarray(barycentrics, np.float64)[:, :, None] * np.asarray(grad, np.float64)[:, None, :]).reshape(-1, 9)
    return vertex_sums64(records, sample_faces, faces, V)


def chamfer(vertices, faces, sample_faces, barycentrics, target_vertices, target_faces, target_points, squared=False):
    """(loss, gradient [V, 3]) of MeshChamferLoss in float64, the closest faces found by brute force"""
    V = len(vertices)
    v, tv = np.asarray(vertices, np.float64), np.asarray(target_vertices, np.float64)
    moving = surface_points(v, faces, sample_faces, barycentrics)
    d_ab, f_ab, _ = winners(moving, tv, target_faces)
    d_ba, f_ba, _ = winners(target_points, v, faces)
    n_ab, n_ba = len(d_ab), len(d_ba)
    if squared:
        loss = 0.5 * ((d_ab * d_ab).mean() + (d_ba * d_ba).mean())
        G_ab, G_ba = d_ab / n_ab, d_ba / n_ba
    else:
        loss = 0.5 * (d_ab.mean() + d_ba.mean())
        G_ab, G_ba = np.full(n_ab, 0.5 / n_ab), np.full(n_ba, 0.5 / n_ba)
    grad_moving = query_gradients(moving, tv, target_faces, f_ab, G_ab)["grad_points"]
    grad = surface_points_backward(grad_moving, faces, sample_faces, barycentrics, V)[0]
    grad += vertex_sums64(query_gradients(target_points, v, faces, f_ba, G_ba)["records"], f_ba, faces, V)[0]
    return loss, grad


def edge_list(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e[e[:, 0] != e[:, 1]], axis=0)


def laplacian_matrix(faces, V):
    """dense [V, V]: v -> v - the mean of its edge neighbours"""
    e = edge_list(faces)
    A = np.zeros((V, V))
    A[e[:, 0], e[:, 1]] = A[e[:, 1], e[:, 0]] = 1.0
    return np.eye(V) - A / np.maximum(A.sum(1, keepdims=True), 1.0)


def fit(vertices, faces, sample_faces, barycentrics, target_vertices, target_faces, target_points, iterations, lr=None, laplacian_weight=1.0, squared=False,
        max_move=None):
    """(vertices, history) of ``fit_mesh_to_mesh`` in float64: torch.optim.Adam's update (betas 0.9 / 0.999, eps 1e-8), the loss BEFORE
    each step; the sampler's draws are arguments"""
    start = np.asarray(vertices, np.float64)
    V = len(start)
    e = edge_list(faces)
    edge_length = np.linalg.norm(start[e[:, 0]] - start[e[:, 1]], axis=1).mean()
    scale = edge_length ** 2 if squared else edge_length
    lr = 0.05 * edge_length if lr is None else lr
    Lm = laplacian_matrix(faces, V)
    start_laplacian = Lm @ start
    v, m, s, history = start.copy(), np.zeros_like(start), np.zeros_like(start), []
    for it in range(1, iterations + 1):
        loss, grad = chamfer(v, faces, sample_faces, barycentrics, target_vertices, target_faces, target_points, squared)
        loss, grad = loss / scale, grad / scale
        if laplacian_weight > 0:
            diff = Lm @ v - start_laplacian
            loss += laplacian_weight * (diff ** 2).sum(1).mean() / edge_length ** 2
            grad += laplacian_weight * 2.0 * (Lm.T @ diff) / (V * edge_length ** 2)
        history.append(loss)
        m, s = 0.9 * m + 0.1 * grad, 0.999 * s + 0.001 * grad * grad
        v = v - lr / (1 - 0.9 ** it) * m / (np.sqrt(s) / np.sqrt(1 - 0.999 ** it) + 1e-8)
        if max_move is not None:
            step = v - start
            length = np.linalg.norm(step, axis=1, keepdims=True)
            v = start + step * (max_move / np.maximum(length, max_move))
    return v, np.array(history)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def box_queries(vertices, count, seed, margin=0.1):
    """``count`` uniform queries in the mesh's box grown by ``margin`` of its largest extent (generic positions: no query sits on a vertex
    or an edge, where the distance has no gradient)"""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float32)
    low, high = v.min(axis=0), v.max(axis=0)
    pad = margin * max(float((high - low).max()), 1.0)
    return rng.uniform(low - pad, high + pad, size=(count, 3)).astype(np.float32)


def offset_queries(vertices, faces, count, seed, reach=0.25):
    """``count`` queries off the surface: area-weighted surface points moved along their face's normal, to either side, by 0.1 .. 1 x
    ``reach`` x the mean edge length.  On a mesh of many small faces a query far from the surface sees an edge or a vertex that several
    faces share, and which of them wins is decided by the last bit; these stay over the face they were drawn from."""
    rng = np.random.default_rng(seed)
    picked, _, points = draws(vertices, faces, count, seed)
    c = np.asarray(vertices, np.float64)[faces[picked]]
    normal = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    e = edge_list(faces)
    edge = np.linalg.norm(np.asarray(vertices, np.float64)[e[:, 0]] - np.asarray(vertices, np.float64)[e[:, 1]], axis=1).mean()
    side = np.where(rng.uniform(size=(count, 1)) < 0.5, -1.0, 1.0)
    return (points + side * rng.uniform(0.1, 1.0, size=(count, 1)) * reach * edge * normal).astype(np.float32)


def fan(blades=20, seed=2):
    """``blades`` triangles round vertex 0 (a shallow cone) and 2 ``blades`` queries over face 0: a face segment and a vertex segment above 16
    entries"""
    angle = 2 * np.pi * np.arange(blades) / blades
    rim = np.stack([np.cos(angle), np.sin(angle), np.full(blades, -0.2)], axis=1)
    v = np.concatenate([[[0, 0, 0]], rim]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % blades] for k in range(blades)], dtype=np.int64)
    rng = np.random.default_rng(seed)
    bary = rng.dirichlet((2, 2, 2), size=2 * blades)
    q = (bary[:, :, None] * v[f[0]].astype(np.float64)).sum(1)
    normal = np.cross(v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]]).astype(np.float64)
    q = q + rng.uniform(0.05, 0.3, size=(2 * blades, 1)) * normal / np.linalg.norm(normal)
    return v, f, q.astype(np.float32)


def sphere_pair(subdivisions=2, scale=1.2, shift=0.1):
    """(moving vertices, faces, target vertices): an icosphere and the same sphere scaled by 1.2 and shifted by 0.1"""
    v, f = M.icosphere(subdivisions)
    return v, f, (v.astype(np.float64) * scale + shift).astype(np.float32)


def draws(vertices, faces, count, seed):
    """(sample faces [count], barycentrics float32 [count, 3], points float32 [count, 3]): a stand-in for the sampler's draws (the strata
    rule of the model, numpy's generator)"""
    rng = np.random.default_rng(seed)
    c = np.asarray(vertices, np.float64)[faces]
    area = 0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1)
    picked = M.strata_faces(area, rng.uniform(size=count))
    bary = M.barycentrics(rng.uniform(size=count), rng.uniform(size=count)).astype(np.float32)
    return picked, bary, surface_points(vertices, faces, picked, bary).astype(np.float32)
