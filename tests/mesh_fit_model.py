"""Float64 numpy model of rf.MeshGeometryRenderer / rf.fit_mesh_to_views (rf_mesh_raster_coverage, rf_mesh_geometry_backward_pixels,
rf_mesh_geometry_backward_gather of include/relu_field.h), restated independently: the depth and the
anti-aliased coverage of a view GIVEN its face ids (which pixel shows which face: the device's own in the GPU test, those of
tests/mesh_raster_model.py on the CPU), both adjoints, the loss, the Laplacian term and Adam.  Next to the values it returns the
error bounds of docs/mesh_fit_errors.md and which pixel pairs are AMBIGUOUS or sit on a KINK.  The inputs the GPU test runs
(``CASES`` / ``make_case``) live here too."""
import numpy as np

from tests import mesh_raster_model as mrm
from tests.helpers import hash_uniform

UNIT = mrm.UNIT
K_EDGE = mrm.K_EDGE          # |fl(e) - e| <= K_EDGE u sum_a C_a D_a (11 u derived in docs/mesh_raster_errors.md)
C_COVERAGE = 2.0             # A: sum of the pairs' tau bounds + (n + C_COVERAGE) u (1 + sum |terms|)
C_GRADIENT = 8.0             # gradient: sum of the terms' propagated bounds + (n + C_GRADIENT) u sum |terms|
K_TERM = 16.0                # the roundings of one gradient term, relative to its magnitude (12 derived)
MAX_AMBIGUOUS = 0.01
KINK = 1.0e-4                # finite differences leave out pairs whose tau is within this of 0, 1/2 or 1 (or of the runner-up's)
WRONG = ("swapped_spill", "no_sigma", "no_wk", "no_clamp")
NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0))  # left, right, up, down as (row, column) steps


def _abs_cross(a, b):
    return np.stack([np.abs(a[..., 1] * b[..., 2]) + np.abs(a[..., 2] * b[..., 1]), np.abs(a[..., 2] * b[..., 0]) + np.abs(a[..., 0] * b[..., 2]),
                     np.abs(a[..., 0] * b[..., 1]) + np.abs(a[..., 1] * b[..., 0])], -1)


def _edges(p, d, D):
    """e [M, 3] of corners p [M, 3, 3] (relative to the camera) and rays d [M, 3], and the bound E [M, 3] (D: the rays' magnitudes)"""
    e, E = [], []
    for k in range(3):
        a, b = p[:, (k + 1) % 3], p[:, (k + 2) % 3]
        e.append((np.cross(a, b) * d).sum(-1))
        E.append(K_EDGE * UNIT * (_abs_cross(a, b) * D).sum(-1))
    return np.stack(e, -1), np.stack(E, -1)


def view_forward(vertices, faces, H, W, focal, R, t, face_ids, wrong=None):
    """One view in float64.  Returns a dict: ``depth``, ``coverage`` [H, W]; ``coverage_bound`` [H, W]; ``pairs``: arrays over the
    (hit pixel a, missed neighbour b) pairs that count -- a, b (flat pixels), m (row of the per-hit arrays), k, tau, tau_bound, ea, eb,
    ambiguous, kink; and the per-hit arrays ``hit`` (flat pixels), ``F``, ``p``, ``e``, ``E``, ``s``, ``w``."""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    ids = np.asarray(face_ids, np.int64).reshape(-1)
    d, D = mrm.rays(H, W, focal, R)
    d, D = d.reshape(-1, 3), D.reshape(-1, 3)
    P = H * W
    hit_mask = ids >= 0
    hit = np.flatnonzero(hit_mask)
    F = ids[hit]
    p = vertices[faces[F]] - t.reshape(1, 1, 3)
    e, E = _edges(p, d[hit], D[hit])
    s = e.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = e / s[:, None]
    zk = -(p @ R[:, 2])
    depth = np.zeros(P)
    depth[hit] = (w * zk).sum(-1)
    gain, loss, terms, tau_sum, count = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    unsure = np.zeros(P, bool)
    parts = []
    i, j = hit // W, hit % W
    for n, (di, dj) in enumerate(NEIGHBOURS):
        bi, bj = i + di, j + dj
        ok = (bi >= 0) & (bi < H) & (bj >= 0) & (bj < W)
        b = np.where(ok, bi * W + bj, 0)
        ok &= ~hit_mask[b]
        m = np.flatnonzero(ok)
        if not len(m):
            continue
        b = b[m]
        eb, Eb = _edges(p[m], d[b], D[b])
        ea, Ea = e[m], E[m]
        sigma = np.ones(len(m)) if wrong == "no_sigma" else np.sign(s[m])
        outside = sigma[:, None] * eb < 0
        q = ea - eb
        with np.errstate(divide="ignore", invalid="ignore"):
            tau_k = np.where(outside, ea / q, np.inf)
        k = np.argmin(tau_k, axis=1)  # (the lowest k on ties)
        rows = np.arange(len(m))
        counts = outside.any(1)
        tau = np.clip(np.where(counts, tau_k[rows, k], 0.0), 0.0, 1.0)
        ea_k, eb_k, Ea_k, Eb_k, q_k = ea[rows, k], eb[rows, k], Ea[rows, k], Eb[rows, k], q[rows, k]
        q_eff = np.maximum(np.abs(q_k) - (Ea_k + Eb_k), 1e-300)
        tau_bound = (Ea_k + tau * (Ea_k + Eb_k)) / q_eff + 3 * UNIT * tau
        # in doubt: an edge value at b that may have the other sign (another set of edges would count), a quotient whose denominator is
        # within its error of 0, a runner-up edge within the errors of the winner
        ambiguous = (np.abs(eb) <= Eb).any(1) | (counts & (np.abs(q_k) <= 4 * (Ea_k + Eb_k)))
        other = np.where(outside & (np.arange(3)[None, :] != k[:, None]), tau_k, np.inf).min(1)
        ambiguous |= counts & (other - tau <= 2 * tau_bound)
        kink = counts & ((np.abs(tau - 0.5) <= KINK) | (tau <= KINK) | (tau >= 1 - KINK) | (other - tau <= KINK))
        c = np.flatnonzero(counts)
        a_pix = hit[m]
        up, down = np.maximum(tau - 0.5, 0.0), np.maximum(0.5 - tau, 0.0)
        if wrong == "swapped_spill":
            up, down = down, up
        np.add.at(gain, b[c], up[c])
        np.add.at(loss, a_pix[c], down[c])
        np.add.at(terms, b[c], up[c])
        np.add.at(terms, a_pix[c], down[c])
        np.add.at(tau_sum, b[c], tau_bound[c])
        np.add.at(tau_sum, a_pix[c], tau_bound[c])
        np.add.at(count, b[c], 1)
        np.add.at(count, a_pix[c], 1)
        unsure[b[ambiguous]] = True
        unsure[a_pix[ambiguous]] = True
        parts.append(dict(a=a_pix[c], b=b[c], m=m[c], k=k[c], tau=tau[c], tau_bound=tau_bound[c], ea=ea_k[c], eb=eb_k[c], ambiguous=ambiguous[c], kink=kink[c],
                          n=np.full(len(c), n)))
    kinds = dict(a=np.int64, b=np.int64, m=np.int64, k=np.int64, n=np.int64, tau=float, tau_bound=float, ea=float, eb=float, ambiguous=bool, kink=bool)
    pairs = {key: (np.concatenate([part[key] for part in parts]) if parts else np.zeros(0, kind)) for key, kind in kinds.items()}
    if wrong == "no_clamp":
        coverage = np.where(hit_mask, 1.0 - loss, gain)
    else:
        coverage = np.where(hit_mask, np.maximum(1.0 - loss, 0.0), np.minimum(gain, 1.0))
    bound = tau_sum + (count + C_COVERAGE) * UNIT * (1.0 + terms)
    return dict(depth=depth.reshape(H, W), coverage=coverage.reshape(H, W), coverage_bound=bound.reshape(H, W), coverage_unsure=unsure.reshape(H, W), pairs=pairs,
                hit=hit, F=F, p=p, e=e, E=E, s=s, w=w, d=d, D=D, raw=(1.0 - loss, gain))


def view_backward(vertices, faces, H, W, focal, R, t, face_ids, grad_depth, grad_coverage, wrong=None, fwd=None):
    """The adjoint of ``view_forward``: (grad [V, 3], bound [V, 3], in doubt [V] bool, kinked [V] bool, per-vertex term count [V]).  The
    saturation of a pixel is decided from the model's own coverage."""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(vertices)
    f = view_forward(vertices, faces, H, W, focal, R, t, face_ids, wrong) if fwd is None else fwd
    gD, gA = np.asarray(grad_depth, np.float64).reshape(-1), np.asarray(grad_coverage, np.float64).reshape(-1)
    A, A_bound = f["coverage"].reshape(-1), f["coverage_bound"].reshape(-1)
    grad, bound, magnitude = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros((V, 3))
    doubt, kinked, count = np.zeros(V, bool), np.zeros(V, bool), np.zeros(V)
    hit, F, p, e, E, s, w = f["hit"], f["F"], f["p"], f["e"], f["E"], f["s"], f["w"]
    corners = faces[F]  # [M, 3]
    # depth: dz/dv_k = w_k n / s
    v = vertices[corners]
    u1, u2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    normal = np.cross(u1, u2)
    normal_bound = 5 * UNIT * _abs_cross(u1, u2)
    Es = E.sum(-1) + 3 * UNIT * np.abs(e).sum(-1)
    s_eff = np.maximum(np.abs(s) - Es, 1e-300)
    for k in range(3):
        wk = np.ones(len(hit)) if wrong == "no_wk" else w[:, k]
        coeff = gD[hit] * wk / s
        dw = (E[:, k] + np.abs(wk) * Es) / s_eff + 2 * UNIT * np.abs(wk)
        dcoeff = np.abs(gD[hit]) * (dw / s_eff + np.abs(wk) * Es / s_eff ** 2 + 3 * UNIT * np.abs(wk / s))
        term = coeff[:, None] * normal
        np.add.at(grad, corners[:, k], term)
        np.add.at(magnitude, corners[:, k], np.abs(term))
        np.add.at(bound, corners[:, k], dcoeff[:, None] * np.abs(normal) + np.abs(coeff)[:, None] * normal_bound)
        np.add.at(count, corners[:, k], (gD[hit] != 0).astype(float))
    # coverage: the pairs
    pr = f["pairs"]
    if len(pr["a"]):
        a, b, m, k, tau = pr["a"], pr["b"], pr["m"], pr["k"], pr["tau"]
        up = (tau > 0.5) & ((A[b] < 1.0) | (wrong == "no_clamp"))
        down = (tau < 0.5) & ((A[a] > 0.0) | (wrong == "no_clamp"))
        if wrong == "swapped_spill":
            G = np.where(tau < 0.5, -gA[b], 0.0) + np.where(tau > 0.5, -gA[a], 0.0)
        else:
            G = np.where(up, gA[b], 0.0) + np.where(down, gA[a], 0.0)
        in_doubt = pr["ambiguous"] | (np.abs(tau - 0.5) <= pr["tau_bound"]) | ((tau > 0.5) & (np.abs(A[b] - 1.0) <= A_bound[b]) & (gA[b] != 0)) \
            | ((tau < 0.5) & (A[a] <= A_bound[a]) & (gA[a] != 0))
        in_doubt |= f["coverage_unsure"].reshape(-1)[a] | f["coverage_unsure"].reshape(-1)[b]
        ea, eb = pr["ea"], pr["eb"]
        Ea, Eb = E[m, k], None
        q = ea - eb
        da, db, Da, Db = f["d"][a], f["d"][b], f["D"][a], f["D"][b]
        pk = p[m]
        rows = np.arange(len(m))
        p1, p2 = pk[rows, (k + 1) % 3], pk[rows, (k + 2) % 3]
        _, Eb_all = _edges(pk, db, Db)
        Eb = Eb_all[rows, k]
        q_eff = np.maximum(np.abs(q) - (Ea + Eb), 1e-300)
        Dv = (ea[:, None] * db - eb[:, None] * da) / (q * q)[:, None]
        D_abs = (np.abs(ea)[:, None] * Db + np.abs(eb)[:, None] * Da) / (q_eff * q_eff)[:, None]
        D_err = (Ea[:, None] * Db + Eb[:, None] * Da) / (q_eff * q_eff)[:, None] + 2 * D_abs * ((Ea + Eb) / q_eff)[:, None]
        g1, g2 = G[:, None] * np.cross(p2, Dv), G[:, None] * np.cross(Dv, p1)
        b1 = np.abs(G)[:, None] * (_abs_cross(p2, D_err) + K_TERM * UNIT * _abs_cross(p2, D_abs))
        b2 = np.abs(G)[:, None] * (_abs_cross(p1, D_err) + K_TERM * UNIT * _abs_cross(p1, D_abs))
        c1, c2 = corners[m, (k + 1) % 3], corners[m, (k + 2) % 3]
        for c, g, bb in ((c1, g1, b1), (c2, g2, b2)):
            np.add.at(grad, c, g)
            np.add.at(magnitude, c, np.abs(g))
            np.add.at(bound, c, bb)
            np.add.at(count, c, (G != 0).astype(float))
        for c in range(3):
            doubt[corners[m[in_doubt], c]] = True
            kinked[corners[m[pr["kink"]], c]] = True
        # a saturation that is close: a kink of the forward as well
        sat = ((tau > 0.5) & (np.abs(A[b] - 1.0) <= KINK)) | ((tau < 0.5) & (A[a] <= KINK))
        for c in range(3):
            kinked[corners[m[sat], c]] = True
    bound = bound + (count[:, None] + C_GRADIENT) * UNIT * magnitude
    return grad, bound, doubt, kinked, count


def forward(case, vertices, face_ids, wrong=None):
    """all views: depth, coverage [N, H, W] and the per-view results"""
    views = [view_forward(vertices, case["faces"], case["H"], case["W"], case["focal"], R, t, face_ids[n], wrong) for n, (R, t) in enumerate(case["views"])]
    shape = (len(views), case["H"], case["W"])
    if not views:
        return np.zeros(shape), np.zeros(shape), views
    return np.stack([v["depth"] for v in views]), np.stack([v["coverage"] for v in views]), views


def backward(case, vertices, face_ids, grad_depth, grad_coverage, wrong=None, views=None):
    V = len(vertices)
    grad, bound, doubt, kinked = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V, bool), np.zeros(V, bool)
    for n, (R, t) in enumerate(case["views"]):
        g, b, a, k, _ = view_backward(vertices, case["faces"], case["H"], case["W"], case["focal"], R, t, face_ids[n], grad_depth[n], grad_coverage[n], wrong,
                                      None if views is None else views[n])
        grad, bound, doubt, kinked = grad + g, bound + b, doubt | a, kinked | k
    return grad, bound + 2 * len(case["views"]) * UNIT * np.abs(grad), doubt, kinked


def model_face_ids(case, vertices=None):
    """the face ids of every view by the float64 rasteriser of tests/mesh_raster_model.py: [N, H, W]"""
    vertices = case["vertices"] if vertices is None else vertices
    out = [mrm.rasterise(vertices, case["faces"], case["H"], case["W"], case["focal"], R, t, near=case["near"], cull=case["cull"])["face_ids"] for R, t in case["views"]]
    return np.stack(out) if out else np.zeros((0, case["H"], case["W"]), np.int64)


# --------------------------------------------------------------------------------------------------------------------- the fit
def loss_and_grads(depth, coverage, face_ids, depths, alphas, depth_weight=1.0, mask_weight=1.0):
    """the image loss of rf.fit_mesh_to_views and its gradients with respect to the two images"""
    depth, coverage, depths, alphas = (np.asarray(x, np.float64) for x in (depth, coverage, depths, alphas))
    both = (np.asarray(face_ids) >= 0) & (alphas > 0.5)
    count = max(int(both.sum()), 1)
    value = mask_weight * ((coverage - alphas) ** 2).mean() + depth_weight * np.abs(depth - depths)[both].sum() / count
    return value, np.where(both, depth_weight * np.sign(depth - depths) / count, 0.0), mask_weight * 2.0 * (coverage - alphas) / coverage.size


def edge_list(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e[e[:, 0] != e[:, 1]], axis=0)


def laplacian(vertices, edges):
    total, degree = np.zeros_like(vertices), np.zeros(len(vertices))
    for a, b in ((0, 1), (1, 0)):
        np.add.at(total, edges[:, a], vertices[edges[:, b]])
        np.add.at(degree, edges[:, a], 1.0)
    return vertices - total / np.maximum(degree, 1.0)[:, None], degree


def laplacian_adjoint(g, edges, degree):
    """the adjoint of v -> v - mean of neighbours applied to g"""
    out = g.copy()
    scaled = g / np.maximum(degree, 1.0)[:, None]
    for a, b in ((0, 1), (1, 0)):
        np.subtract.at(out, edges[:, b], scaled[edges[:, a]])
    return out


def adam_fit(case, start, depths, alphas, iterations, lr, laplacian_weight=1.0, depth_weight=1.0, mask_weight=1.0, max_move=None, betas=(0.9, 0.999), eps=1e-8,
             face_ids_of=None):
    """rf.fit_mesh_to_views in float64, rasterising with tests/mesh_raster_model.py (or ``face_ids_of(vertices)``): (losses before each
    step, vertices)"""
    start = np.asarray(start, np.float64)
    vertices = start.copy()
    edges = edge_list(np.asarray(case["faces"], np.int64))
    length = np.linalg.norm(start[edges[:, 0]] - start[edges[:, 1]], axis=1).mean()
    lap0, degree = laplacian(start, edges)
    m1, m2, losses = np.zeros_like(vertices), np.zeros_like(vertices), []
    for step in range(1, iterations + 1):
        # (the renderer sees float32 vertices: so does the model's rasteriser, or the two would disagree on pixels for no reason)
        seen = vertices.astype(np.float32).astype(np.float64)
        ids = model_face_ids(case, seen) if face_ids_of is None else face_ids_of(seen)
        depth, coverage, views = forward(case, seen, ids)
        value, gD, gA = loss_and_grads(depth, coverage, ids, depths, alphas, depth_weight, mask_weight)
        g = backward(case, seen, ids, gD, gA, views=views)[0]
        diff = laplacian(vertices, edges)[0] - lap0
        value += laplacian_weight * (diff ** 2).sum(1).mean() / length ** 2
        g = g + laplacian_weight * 2.0 * laplacian_adjoint(diff, edges, degree) / (len(vertices) * length ** 2)
        losses.append(value)
        m1 = betas[0] * m1 + (1 - betas[0]) * g
        m2 = betas[1] * m2 + (1 - betas[1]) * g * g
        vertices = vertices - (lr / (1 - betas[0] ** step)) * m1 / (np.sqrt(m2) / np.sqrt(1 - betas[1] ** step) + eps)
        if max_move is not None:
            move = vertices - start
            vertices = start + move * (max_move / np.maximum(np.linalg.norm(move, axis=1, keepdims=True), max_move))
    return np.array(losses), vertices


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test (tests/test_hip_mesh_fit.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _case(name, H, W, focal, views, vertices, faces, near=0.0, cull=False, exact=False):
    return dict(name=name, H=H, W=W, focal=float(np.float32(focal)), views=views, vertices=np.ascontiguousarray(vertices, np.float32),
                faces=np.ascontiguousarray(faces, np.int64), near=near, cull=cull, exact=exact)


def _views(seed, n, away=()):
    from tests.texture_fit_model import _views as views

    return views(seed, n, away)


EXACT_VIEW = [mrm.IDENTITY]


def _builders():
    B = {}

    def one_pixel(seed):
        views = _views(seed, 1)
        return _case("tri-1x1", 1, 1, 1.5, views, *mrm.soup([mrm.unproject([[-3.0, -3.0], [5.0, -2.0], [0.0, 6.0]], [2.0, 2.0, 3.0], 1, 1, 1.5, *views[0])]))
    B["tri-1x1"] = one_pixel

    def two_pixels(seed):
        views = _views(seed, 1)
        return _case("tri-1x2", 1, 2, 1.5, views, *mrm.soup([mrm.unproject([[-3.0, -3.0], [0.8, -2.0], [0.6, 6.0]], [2.0, 2.0, 3.0], 1, 2, 1.5, *views[0])]))
    B["tri-1x2"] = two_pixels

    def small(seed):
        views = _views(seed, 1)
        return _case("tri-5x7", 5, 7, 6.0, views, *mrm.soup([mrm.unproject([[0.7, 0.4], [5.8, 1.1], [2.9, 4.3]], [2.0, 2.5, 3.0], 5, 7, 6.0, *views[0])]))
    B["tri-5x7"] = small

    # identity pose, focal 16, depth 4: pixel coordinates in quarters give dyadic world coordinates and exact edge values
    for label, lo, hi in (("centres", 2.0, 10.0), ("midpoints", 2.5, 10.5), ("quarters", 2.25, 10.0)):
        def exact(seed, label=label, lo=lo, hi=hi):  # the silhouette through pixel centres (tau = 0), midpoints (1/2) and quarters (1/4, 3/4)
            return _case(f"exact-{label}", 16, 16, 16.0, EXACT_VIEW, mrm._exact_points([[lo, lo], [hi, lo], [lo, hi]]), np.array([[0, 1, 2]], np.int64), exact=True)
        B[f"exact-{label}"] = exact

    def sliver(seed):  # thinner than a pixel and between two columns of centres: hit nowhere, coverage 0 everywhere
        return _case("exact-sliver", 16, 16, 16.0, EXACT_VIEW, mrm._exact_points([[4.25, 2.25], [4.75, 2.25], [4.5, 12.75]]), np.array([[0, 1, 2]], np.int64), exact=True)
    B["exact-sliver"] = sliver

    def quad(seed):
        views = _views(seed, 2)
        corners = mrm.unproject([[3.3, 2.2], [19.6, 4.1], [17.2, 14.9], [2.4, 13.3]], [2.0, 2.4, 2.9, 2.2], 18, 24, 20.0, *views[0])
        return _case("quad", 18, 24, 20.0, views, corners, np.array([[0, 1, 2], [0, 2, 3]], np.int64))
    B["quad"] = quad

    for cull, flipped in ((False, False), (True, False), (True, True)):
        def octahedron(seed, cull=cull, flipped=flipped):
            pts = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.5 + 0.03 * hash_uniform((6, 3), 77).astype(np.float64)
            faces = []
            for sx in (0, 1):
                for sy in (2, 3):
                    for sz in (4, 5):
                        outward = ((-1) ** sx) * ((-1) ** sy) * ((-1) ** sz) > 0
                        faces.append([sx, sy, sz] if outward else [sx, sz, sy])
            faces = np.array(faces, np.int64)
            R0, _ = mrm.pose(55)
            views = [(R0, (R0.astype(np.float64) @ np.array([0.05, -0.03, 3.0])).astype(np.float32)), (np.eye(3, dtype=np.float32), np.array([0.1, 0.05, 2.5], np.float32))]
            return _case(f"octahedron-cull{int(cull)}{'-cw' if flipped else ''}", 24, 32, 40.0, views, pts, faces[:, ::-1] if flipped else faces, cull=cull)
        B[f"octahedron-cull{int(cull)}{'-cw' if flipped else ''}"] = octahedron

    def patch(seed):  # 37 faces from 3 views, the last of which looks past the mesh
        H, W, f, views = 24, 32, 30.0, _views(seed, 3, away=(2,))
        tris = np.concatenate([mrm.small_triangles(30, H, W, f, *views[0], seed + 5, 5.0), mrm.large_triangles(7, H, W, f, *views[0], seed + 9, 0.3)])
        return _case("patch37-24x32-v3", H, W, f, views, *mrm.soup(tris))
    B["patch37-24x32-v3"] = patch

    for near in (0.0, 2.6):
        def stacked(seed, near=near):  # two faces behind one another; near = 2.6 rejects the front one (its corners are at depth 2 .. 2.4)
            H, W, f, views = 18, 24, 20.0, _views(4321, 1)
            front = mrm.unproject([[4.3, 3.1], [18.2, 5.4], [9.7, 14.6]], [2.0, 2.2, 2.4], H, W, f, *views[0])
            back = mrm.unproject([[1.2, 1.4], [22.1, 2.7], [11.3, 16.9]], [3.0, 3.3, 3.1], H, W, f, *views[0])
            return _case(f"stacked-near{near}", H, W, f, views, *mrm.soup([front, back]), near=near)
        B[f"stacked-near{near}"] = stacked

    def fills_the_frame(seed):  # coverage 1 everywhere, no pair, zero coverage gradient
        H, W, f, views = 12, 16, 20.0, _views(seed, 1)
        return _case("fills-the-frame", H, W, f, views, *mrm.soup([mrm.unproject([[-200.0, -150.0], [300.0, -100.0], [20.0, 400.0]], [3.0, 2.5, 3.5], H, W, f, *views[0])]))
    B["fills-the-frame"] = fills_the_frame

    def fan(seed):  # a hub shared by 20 faces: its corner segment is longer than the wavefront threshold
        H, W, f, views = 24, 32, 30.0, _views(seed, 2)
        angle = np.arange(20) * (2 * np.pi / 20) + 0.13
        rim = np.stack([16.2 + 10.5 * np.cos(angle), 12.3 + 9.5 * np.sin(angle)], -1)
        pix = np.concatenate([[[15.7, 11.8]], rim])
        depth = 2.5 + 0.3 * hash_uniform((21,), seed + 3).astype(np.float64)
        faces = np.array([[0, 1 + k, 1 + (k + 1) % 20] for k in range(20)], np.int64)
        return _case("fan20", H, W, f, views, mrm.unproject(pix, depth, H, W, f, *views[0]), faces)
    B["fan20"] = fan

    def big_face(seed):  # one face over more than 4096 pixels of a 72 x 72 image, with a silhouette inside the frame
        H, W, f, views = 72, 72, 80.0, _views(seed, 1)
        return _case("big-face-72x72", H, W, f, views, *mrm.soup([mrm.unproject([[-100.3, 130.2], [130.4, -100.1], [300.0, 300.0]], [2.5, 3.0, 3.5], H, W, f, *views[0])]))
    B["big-face-72x72"] = big_face
    return B


BUILDERS = _builders()
CASES = list(BUILDERS)
EXACT_CASES = [name for name in CASES if name.startswith("exact-")]
_MADE = {}


def make_case(name):
    if name not in _MADE:
        _MADE[name] = BUILDERS[name](9000 + 43 * CASES.index(name))
    return _MADE[name]


_IDS = {}


def case_face_ids(name):
    """the float64 rasteriser's face ids of a case, computed once and shared"""
    if name not in _IDS:
        _IDS[name] = model_face_ids(make_case(name))
    return _IDS[name]


def upstream(case, seed=17):
    """the upstream gradients the tests feed: (grad_depth, grad_coverage) [N, H, W] float32"""
    shape = (len(case["views"]), case["H"], case["W"])
    return hash_uniform(shape, seed).astype(np.float32), hash_uniform(shape, seed + 1).astype(np.float32)
