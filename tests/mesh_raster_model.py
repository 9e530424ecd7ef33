"""Float64 numpy model of rf.render_mesh (rf_mesh_raster_visibility / rf_mesh_raster_shade of include/relu_field.h),
restated independently: a brute force over ALL triangles per pixel -- no boxes, no two paths, no visibility buffer -- of the rays of
cast_rays, the coverage rule, the depth rule, the tie rule, the UV convention and the bilinear fetch.  Next to face id, z, w and
colour it returns the per-pixel error bounds of docs/mesh_raster_errors.md and the mask of AMBIGUOUS pixels, those where float32 may
decide a comparison the other way.  The inputs the GPU test runs (``CASES`` / ``make_case``) live here too, so that the CPU tests can
show on exactly those inputs that few pixels are ambiguous and that the comparison can fail."""
import numpy as np

from tests.helpers import hash_uniform
from thr3ed_atom_amd.texture import atlas_layout, corner_uvs

UNIT = 2.0 ** -24  # float32 unit round-off
K_EDGE = 16.0      # |fl(e) - e| <= K_EDGE u sum_a C_a D_a  (11 u derived in docs/mesh_raster_errors.md)
K_DEPTH = 6.0      # |fl(z_k) - z_k| <= K_DEPTH u sum_a |p_ka R_a2|  (4 u derived)
MAX_AMBIGUOUS = 0.01
WRONG = ("exclusive_edges", "higher_index_wins", "v_not_flipped", "integer_centres")


def rays(H, W, focal, R, wrong=None, dtype=np.float64):
    """d [H, W, 3] of cast_rays and D [H, W, 3], the same expression with every term replaced by its magnitude"""
    R = np.asarray(R, dtype)
    half = dtype(0.0 if wrong == "integer_centres" else 0.5)
    j, i = np.meshgrid(np.arange(W, dtype=dtype), np.arange(H, dtype=dtype))
    cx = ((j + half) - dtype(W) * dtype(0.5)) / dtype(focal)
    cy = -(((i + half) - dtype(H) * dtype(0.5)) / dtype(focal))
    d = np.stack([(R[a, 0] * cx + R[a, 1] * cy) + R[a, 2] * dtype(-1.0) for a in range(3)], axis=-1)
    D = np.stack([np.abs(R[a, 0] * cx) + np.abs(R[a, 1] * cy) + np.abs(R[a, 2]) for a in range(3)], axis=-1)
    return d, D


def edge_values(vertices, faces, H, W, focal, R, t, wrong=None, dtype=np.float64):
    """e [T, H W, 3] and its bound E [T, H W, 3]; z_k [T, 3] and its bound [T, 3]"""
    v = np.asarray(vertices, dtype)[np.asarray(faces, np.int64)]  # [T, 3, 3]
    p = v - np.asarray(t, dtype).reshape(1, 1, 3)
    d, D = rays(H, W, focal, R, wrong, dtype)
    d, D = d.reshape(-1, 3), D.reshape(-1, 3)
    e, E = [], []
    for k in range(3):
        a, b = p[:, (k + 1) % 3], p[:, (k + 2) % 3]
        c = np.cross(a, b)
        C = np.stack([np.abs(a[:, 1] * b[:, 2]) + np.abs(a[:, 2] * b[:, 1]), np.abs(a[:, 2] * b[:, 0]) + np.abs(a[:, 0] * b[:, 2]),
                      np.abs(a[:, 0] * b[:, 1]) + np.abs(a[:, 1] * b[:, 0])], axis=-1)
        e.append((c[:, None, 0] * d[None, :, 0] + c[:, None, 1] * d[None, :, 1]) + c[:, None, 2] * d[None, :, 2])
        E.append(K_EDGE * UNIT * (C @ D.T))
    Rm = np.asarray(R, dtype)
    zk = -((p[..., 0] * Rm[0, 2] + p[..., 1] * Rm[1, 2]) + p[..., 2] * Rm[2, 2])
    Zk = K_DEPTH * UNIT * (np.abs(p[..., 0] * Rm[0, 2]) + np.abs(p[..., 1] * Rm[1, 2]) + np.abs(p[..., 2] * Rm[2, 2]))
    return np.stack(e, -1), np.stack(E, -1), zk, Zk


def _texture_fetch(texture, uv, duv, wrong):
    """bilinear fetch at [M, 2] (u, v) with error duv [M, 2]: colour [M, 3] and its bound [M]"""
    tex = np.asarray(texture, np.float64)
    Ht, Wt = tex.shape[:2]
    x = uv[:, 0] * Wt - 0.5
    y = (uv[:, 1] if wrong == "v_not_flipped" else 1.0 - uv[:, 1]) * Ht - 0.5
    dx = Wt * duv[:, 0] + 2 * UNIT * (np.abs(uv[:, 0]) * Wt + 0.5)
    dy = Ht * (duv[:, 1] + 2 * UNIT) + 2 * UNIT * ((np.abs(uv[:, 1]) + 1.0) * Ht + 0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    cl = lambda a, n: np.clip(a, 0, n - 1).astype(np.int64)  # noqa: E731
    xa, xb, ya, yb = cl(x0, Wt), cl(x0 + 1, Wt), cl(y0, Ht), cl(y0 + 1, Ht)
    top = (1 - fx)[:, None] * tex[ya, xa] + fx[:, None] * tex[ya, xb]
    bot = (1 - fx)[:, None] * tex[yb, xa] + fx[:, None] * tex[yb, xb]
    colour = (1 - fy)[:, None] * top + fy[:, None] * bot
    # the local gradient: the largest step between neighbouring texels of the 4 x 4 window around the fetch (clamped)
    gx, gy = np.zeros(len(x)), np.zeros(len(x))
    for oy in range(-1, 3):
        for ox in range(-1, 3):
            here = tex[cl(y0 + oy, Ht), cl(x0 + ox, Wt)]
            gx = np.maximum(gx, np.abs(tex[cl(y0 + oy, Ht), cl(x0 + ox + 1, Wt)] - here).max(-1))
            gy = np.maximum(gy, np.abs(tex[cl(y0 + oy + 1, Ht), cl(x0 + ox, Wt)] - here).max(-1))
    return colour, gx * dx + gy * dy + 8 * UNIT * np.abs(tex).max()


def rasterise(vertices, faces, H, W, focal, R, t, near=0.0, cull=False, white=False, uvs=None, texture=None, colours=None, wrong=None, chunk=128):
    """The whole call in float64.  Returns a dict of [H, W, ...] arrays: ``face_ids`` (-1: nothing), ``mask``, ``depth``, ``bary``, ``colour``
    (None without a source), the bounds ``depth_bound``, ``bary_bound`` [H, W, 3], ``colour_bound``, and ``ambiguous`` [H, W] bool.
    ``wrong``: one of the WRONG models the comparison must reject."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    T, P = len(faces), H * W
    near = float(np.float32(near))
    best_z = np.full(P, np.inf)
    best_dz = np.zeros(P)
    best_id = np.full(P, -1, np.int64)
    best_w, best_dw = np.zeros((P, 3)), np.zeros((P, 3))
    ambiguous = np.zeros(P, bool)

    def candidates(lo, hi):
        e, E, zk, Zk = edge_values(vertices, faces[lo:hi], H, W, focal, R, t, wrong)
        s = e.sum(-1)
        Es = E.sum(-1) + 3 * UNIT * np.abs(e).sum(-1)
        neg_in, pos_in = (e < -E).all(-1), (e > E).all(-1)
        sure_in = (neg_in | (pos_in & (not cull))) & (np.abs(s) > 2 * Es)
        sure_out = ((e > E).any(-1) & (e < -E).any(-1)) | ((e > E).any(-1) if cull else False)
        # a face that names a vertex twice: p_a x p_a is 0 and the two other edge values are e and -e, bit for bit, so s is exactly 0
        f = faces[lo:hi]
        sure_out |= ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))[:, None]
        if wrong == "exclusive_edges":
            hit = ((e < 0).all(-1) | ((e > 0).all(-1) & (not cull))) & (s != 0)
        else:
            hit = ((e <= 0).all(-1) | ((e >= 0).all(-1) & (not cull))) & (s != 0)
        dropped = (zk < near - Zk).any(-1)                 # some corner surely nearer than near: surely not drawn
        kept = (zk >= near + Zk).all(-1)                   # surely drawn
        hit &= ~(zk < near).any(-1)[:, None]
        unsure = ~sure_in & ~sure_out
        unsure |= (~kept & ~dropped)[:, None] & ~sure_out  # the depth rule itself is in doubt
        unsure &= ~dropped[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = e / s[..., None]
            dw = (E + np.abs(w) * Es[..., None]) / np.maximum(np.abs(s) - Es, 1e-300)[..., None] + 2 * UNIT * np.abs(w)
        dz0 = zk[:, None, :] - zk[:, None, :1]               # [Tc, 1, 3]: z_k - z_0
        w, dw = np.where(np.isfinite(w), w, 0.0), np.where(np.isfinite(dw), dw, 1e300)
        z = zk[:, None, 0] + (w[..., 1] * dz0[..., 1] + w[..., 2] * dz0[..., 2])
        dz = Zk[:, None, 0] + 4 * UNIT * (np.abs(zk[:, None, 0]) + np.abs(w[..., 1] * dz0[..., 1]) + np.abs(w[..., 2] * dz0[..., 2]))
        for k in (1, 2):
            dz = dz + dw[..., k] * np.abs(dz0[..., k]) + np.abs(w[..., k]) * (Zk[:, None, k] + Zk[:, None, 0] + UNIT * np.abs(dz0[..., k]))
        hit &= np.isfinite(z) & (z >= 0)
        unsure |= hit & ~(z - dz > 0)  # (the kernel drops a hit whose computed depth is negative)
        return hit, unsure, z, dz, w, dw

    for lo in range(0, T, chunk):  # pass 1: the winner, ties to the lower (or, wrongly, the higher) index
        hit, unsure, z, dz, w, dw = candidates(lo, min(lo + chunk, T))
        ambiguous |= unsure.any(0)
        zz = np.where(hit, z, np.inf)
        order = zz[::-1] if wrong == "higher_index_wins" else zz
        row = np.argmin(order, axis=0)
        if wrong == "higher_index_wins":
            row = len(zz) - 1 - row
        cz = zz[row, np.arange(P)]
        better = (cz <= best_z) & np.isfinite(cz) if wrong == "higher_index_wins" else cz < best_z
        sel = np.arange(P)[better]
        best_z[sel], best_dz[sel], best_id[sel] = cz[sel], dz[row[sel], sel], lo + row[sel]
        best_w[sel], best_dw[sel] = w[row[sel], sel], dw[row[sel], sel]
    for lo in range(0, T, chunk):  # pass 2: any other candidate whose depth interval reaches the winner's
        hi = min(lo + chunk, T)
        hit, unsure, z, dz, w, dw = candidates(lo, hi)
        ids = np.arange(lo, hi)[:, None]
        twin = (faces[np.maximum(best_id, 0)][None, :, :] == faces[lo:hi][:, None, :]).all(-1)  # a literal duplicate: the same bits on the GPU
        ambiguous |= (hit & (ids != best_id[None]) & ~twin & (z - dz <= (best_z + best_dz)[None])).any(0)
    mask = best_id >= 0
    depth = np.where(mask, best_z, 0.0)
    bary = np.where(mask[:, None], best_w, 0.0)
    bary_bound = np.where(mask[:, None], best_dw, 0.0)
    colour = colour_bound = None
    fid = np.maximum(best_id, 0)
    if texture is not None:
        uv_c = np.asarray(uvs, np.float64)[fid]  # [P, 3, 2]
        uv = (bary[..., None] * uv_c).sum(1)
        duv = (bary_bound[..., None] * np.abs(uv_c)).sum(1) + 4 * UNIT * (np.abs(bary)[..., None] * np.abs(uv_c)).sum(1)
        colour, colour_bound = _texture_fetch(texture, uv, duv, wrong)
    elif colours is not None:
        cc = np.asarray(colours, np.float64)[faces[fid]]  # [P, 3 corners, 3]
        colour = (bary[..., None] * cc).sum(1)
        colour_bound = ((bary_bound[..., None] * np.abs(cc)).sum(1) + 4 * UNIT * (np.abs(bary)[..., None] * np.abs(cc)).sum(1)).max(-1)
    if colour is not None:
        colour = np.where(mask[:, None], colour, 1.0 if white else 0.0).reshape(H, W, 3)
        colour_bound = np.where(mask, colour_bound, 0.0).reshape(H, W)
    return dict(face_ids=best_id.reshape(H, W), mask=mask.reshape(H, W), depth=depth.reshape(H, W), bary=bary.reshape(H, W, 3), colour=colour,
                depth_bound=np.where(mask, best_dz, 0.0).reshape(H, W), bary_bound=bary_bound.reshape(H, W, 3), colour_bound=colour_bound,
                ambiguous=ambiguous.reshape(H, W))


def compare(ref, got, exact=False):
    """Assert ``got`` (dict: face_ids, mask, depth [H, W], bary or None, colour or None) against the model's ``ref`` on the pixels that
    are not ambiguous -- on EVERY pixel when ``exact``.  Returns the worst error / bound ratio."""
    take = np.ones_like(ref["ambiguous"]) if exact else ~ref["ambiguous"]
    assert np.array_equal(np.asarray(got["mask"])[take], ref["mask"][take]), "mask"
    assert np.array_equal(np.asarray(got["face_ids"]).astype(np.int64)[take], ref["face_ids"][take]), "face ids"
    worst = 0.0
    pairs = [("depth", "depth_bound")]
    if got.get("bary") is not None:
        pairs.append(("bary", "bary_bound"))
    if ref["colour"] is not None:
        assert got.get("colour") is not None
        pairs.append(("colour", "colour_bound"))
    for name, bound_name in pairs:
        err = np.abs(np.asarray(got[name], np.float64) - ref[name])
        bound = ref[bound_name]
        if err.ndim == 3 and bound.ndim == 2:
            err = err.max(-1)
        t = take if err.ndim == 2 else take[..., None] & np.ones(err.shape, bool)
        assert (err[t] <= bound[t]).all(), f"{name}: worst error {err[t].max():.3e}, over its bound by up to {(err[t] - bound[t]).max():.3e}"
        nz = t & (bound > 0)
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
    return worst


def as_result(ref):
    return dict(face_ids=ref["face_ids"], mask=ref["mask"], depth=ref["depth"], bary=ref["bary"], colour=ref["colour"])


def assert_exact_in_float32(case):
    """the crafted cases: every edge value and corner depth is the same number in float32 and in float64"""
    a = edge_values(case["vertices"], case["faces"], case["H"], case["W"], case["focal"], case["R"], case["t"], dtype=np.float32)
    b = edge_values(case["vertices"], case["faces"], case["H"], case["W"], case["focal"], case["R"], case["t"], dtype=np.float64)
    assert a[0].dtype == np.float32 and np.array_equal(a[0].astype(np.float64), b[0]) and np.array_equal(a[2].astype(np.float64), b[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test (tests/test_hip_mesh_raster.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def pose(seed):
    """a rotation (orthonormal to float32 rounding) and a translation"""
    r = hash_uniform((3, 3), seed).astype(np.float64)
    q, _ = np.linalg.qr(r + 2.0 * np.eye(3))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q.astype(np.float32), (0.5 * hash_uniform((3,), seed + 1)).astype(np.float32)


IDENTITY = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))


def unproject(pix, depth, H, W, focal, R, t):
    """world points (float32) that project to pixel coordinates pix [.., 2] = (column, row) at camera depth ``depth``"""
    pix, depth = np.asarray(pix, np.float64), np.asarray(depth, np.float64)
    cam = np.stack([(pix[..., 0] + 0.5 - W / 2) / focal * depth, -(pix[..., 1] + 0.5 - H / 2) / focal * depth, -depth], axis=-1)
    return (cam @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)).astype(np.float32)


def _uniform(shape, seed, lo=0.0, hi=1.0):
    return lo + (hi - lo) * (hash_uniform(shape, seed).astype(np.float64) * 0.5 + 0.5)


def soup(tris):
    """[T, 3, 3] corner positions -> vertices [3 T, 3], faces [T, 3]"""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    return tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3)


def small_triangles(T, H, W, focal, R, t, seed, size=0.9):
    centre = np.stack([_uniform((T,), seed, -1.0, W), _uniform((T,), seed + 1, -1.0, H)], -1)
    pix = centre[:, None, :] + size * hash_uniform((T, 3, 2), seed + 2).astype(np.float64)
    depth = _uniform((T, 3), seed + 3, 2.0, 4.0)
    return unproject(pix, depth, H, W, focal, R, t)


def large_triangles(T, H, W, focal, R, t, seed, spread=1.0):
    pix = np.stack([_uniform((T, 3), seed, -spread * W, (1 + spread) * W), _uniform((T, 3), seed + 1, -spread * H, (1 + spread) * H)], -1)
    depth = _uniform((T, 3), seed + 2, 2.0, 4.0)
    return unproject(pix, depth, H, W, focal, R, t)


def _case(name, H, W, focal, Rt, vertices, faces, seed, near=0.0, cull=False, white=False, source="colours", patch=None, bary=False, exact=False):
    R, t = Rt
    vertices, faces = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(faces, np.int64)
    made = dict(name=name, H=H, W=W, focal=float(np.float32(focal)), R=R, t=t, vertices=vertices, faces=faces, near=near, cull=cull, white=white, bary=bary,
                exact=exact, uvs=None, texture=None, colours=None, patch=patch)
    if source == "texture":
        lay = atlas_layout(len(faces), patch)
        made["uvs"] = corner_uvs(lay, len(faces))
        made["texture"] = (hash_uniform((lay.height, lay.width, 3), seed + 50) * np.float32(0.5) + np.float32(0.5)).astype(np.float32)
    elif source == "colours":
        made["colours"] = (hash_uniform((len(vertices), 3), seed + 51) * np.float32(0.5) + np.float32(0.5)).astype(np.float32)
    return made


def _exact_points(pix, Z=4.0, H=16, W=16, focal=16.0):
    """identity pose, power-of-two focal and depth: pixel coordinates (column, row) in halves -> dyadic world coordinates"""
    pix = np.asarray(pix, np.float64)
    return np.stack([(pix[..., 0] + 0.5 - W / 2) * Z / focal, -(pix[..., 1] + 0.5 - H / 2) * Z / focal, np.full(pix.shape[:-1], -Z)], -1).astype(np.float32)


def _builders():
    B = {}

    def add(name, fn):
        B[name] = fn

    def fullscreen(seed):
        H, W, f, Rt = 24, 40, 30.0, pose(seed)
        tri = unproject([[-200.0, -150.0], [300.0, -100.0], [20.0, 400.0]], [3.0, 2.5, 3.5], H, W, f, *Rt)
        return _case("fullscreen", H, W, f, Rt, *soup([tri]), seed, bary=True)
    add("fullscreen", fullscreen)

    def one_pixel(seed):
        Rt = pose(seed)
        tris = [unproject([[-3.0, -3.0], [5.0, -2.0], [0.0, 6.0]], [2.0, 2.0, 3.0], 1, 1, 1.5, *Rt), unproject([[3.0, 3.0], [5.0, 3.0], [4.0, 6.0]], [1.0, 1.0, 1.0], 1, 1, 1.5, *Rt)]
        return _case("one_pixel", 1, 1, 1.5, Rt, *soup(tris), seed)
    add("one_pixel", one_pixel)

    def overhang(seed):
        H, W, f, Rt = 24, 40, 28.0, pose(seed)
        spots = [(-1.0, 12.0), (40.0, 11.0), (20.0, -1.0), (19.0, 24.0), (0.0, 0.0), (39.0, 0.0), (0.0, 23.0), (39.0, 23.0)]  # edges, then corners
        tris = []
        for n, (x, y) in enumerate(spots):
            pix = np.array([x, y]) + np.array([[-6.0, -5.0], [7.0, -4.0], [-3.0, 8.0]]) + hash_uniform((3, 2), seed + 10 + n).astype(np.float64)
            tris.append(unproject(pix, _uniform((3,), seed + 30 + n, 2.0, 4.0), H, W, f, *Rt))
        return _case("overhang", H, W, f, Rt, *soup(tris), seed)
    add("overhang", overhang)

    for T in (1, 63, 64, 65, 2000):
        def slivers(seed, T=T):
            H, W, f, Rt = (64, 64, 24.0, pose(seed)) if T == 2000 else (24, 40, 30.0, pose(seed))
            return _case(f"slivers{T}", H, W, f, Rt, *soup(small_triangles(T, H, W, f, *Rt, seed + 5, size=0.9 if T == 2000 else 1.6)), seed,
                         source="texture" if T in (65, 2000) else "colours", patch=3)
        add(f"slivers{T}", slivers)

    def mixed(seed):
        H, W, f, Rt = 37, 53, 45.0, pose(seed)
        tris = np.concatenate([small_triangles(150, H, W, f, *Rt, seed + 5, 1.5), large_triangles(5, H, W, f, *Rt, seed + 9, 0.3), small_triangles(60, H, W, f, *Rt, seed + 13, 4.0)])
        order = np.argsort(hash_uniform((len(tris),), seed + 17), kind="stable")
        return _case("mixed", H, W, f, Rt, *soup(tris[order]), seed, bary=True)
    add("mixed", mixed)

    def interpenetrating(seed):
        H, W, f, Rt = 64, 64, 60.0, pose(seed)
        return _case("interpenetrating", H, W, f, Rt, *soup(large_triangles(40, H, W, f, *Rt, seed + 5, 0.2)), seed, bary=True)
    add("interpenetrating", interpenetrating)

    def behind_and_near(seed):
        H, W, f, Rt = 24, 40, 30.0, pose(seed)
        pix = np.stack([_uniform((6, 3), seed + 5, 0, W), _uniform((6, 3), seed + 6, 0, H)], -1)
        depth = _uniform((6, 3), seed + 7, 2.0, 4.0)
        depth[0] = -depth[0]          # wholly behind the camera
        depth[1, 2] = -1.0            # one corner behind
        depth[2, 1] = 0.5             # one corner nearer than near = 1
        depth[3] = [0.3, 0.6, 0.9]    # wholly nearer
        return _case("behind_and_near", H, W, f, Rt, *soup(unproject(pix, depth, H, W, f, *Rt)), seed, near=1.0)
    add("behind_and_near", behind_and_near)

    def zero_area(seed):
        H, W, f, Rt = 24, 40, 30.0, pose(seed)
        tris = large_triangles(5, H, W, f, *Rt, seed + 5, 0.1)
        vertices, faces = soup(tris)
        faces[1, 1] = faces[1, 0]                                           # two corners on one vertex
        faces[3] = faces[3, 0]                                              # all three
        vertices[3 * 2 + 2] = 0.5 * (vertices[3 * 2] + vertices[3 * 2 + 1])  # three collinear points
        return _case("zero_area", H, W, f, Rt, vertices, faces, seed)
    add("zero_area", zero_area)

    for cull in (False, True):
        def windings(seed, cull=cull):
            seed = 4242  # (the same mesh with culling off and on)
            H, W, f, Rt = 24, 40, 30.0, pose(seed)
            vertices, faces = soup(large_triangles(8, H, W, f, *Rt, seed + 5, 0.0))
            faces[::2] = faces[::2, ::-1]  # every other face runs the other way
            return _case(f"windings-cull{int(cull)}", H, W, f, Rt, vertices, faces, seed, cull=cull, white=cull)
        add(f"windings-cull{int(cull)}", windings)

    for patch in (2, 3, 8):
        def textured(seed, patch=patch):
            H, W, f, Rt = 24, 40, 30.0, pose(seed)
            tris = np.concatenate([large_triangles(5, H, W, f, *Rt, seed + 5, 0.1), small_triangles(30, H, W, f, *Rt, seed + 9, 3.0)])
            return _case(f"textured-P{patch}", H, W, f, Rt, *soup(tris), seed, source="texture", patch=patch, white=patch == 3, bary=True)
        add(f"textured-P{patch}", textured)

    def duplicate(seed):
        H, W, f, Rt = 24, 40, 30.0, pose(seed)
        vertices, faces = soup(large_triangles(4, H, W, f, *Rt, seed + 5, 0.0))
        faces = np.concatenate([faces, faces[1:2], faces[0:1]])  # literal duplicates at higher indices
        return _case("duplicate", H, W, f, Rt, vertices, faces, seed, source="texture", patch=3)
    add("duplicate", duplicate)

    def no_colour(seed):
        H, W, f, Rt = 24, 40, 30.0, pose(seed)
        return _case("no_colour", H, W, f, Rt, *soup(large_triangles(3, H, W, f, *Rt, seed + 5, 0.0)), seed, source=None)
    add("no_colour", no_colour)

    # ---- the exact cases: identity pose, focal 16, depth 4, pixel coordinates in halves; every pixel is compared ----------------------
    for flipped in (False, True):
        def quad(seed, flipped=flipped):
            corners = _exact_points([[2, 2], [10, 2], [10, 10], [2, 10]])  # the diagonal (2, 2) - (10, 10) runs through pixel centres
            faces = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
            return _case(f"exact-quad-{'cw' if flipped else 'ccw'}", 16, 16, 16.0, IDENTITY, corners, faces[:, ::-1] if flipped else faces, seed, exact=True, bary=True)
        add(f"exact-quad-{'cw' if flipped else 'ccw'}", quad)

        def fan(seed, flipped=flipped):
            rim = [[2, 8], [4, 3], [8, 1], [13, 4], [14, 9], [9, 14], [3, 13]]
            pts = _exact_points([[8, 8]] + rim)  # the hub sits exactly on a pixel centre
            faces = np.array([[0, 1 + k, 1 + (k + 1) % len(rim)] for k in range(len(rim))], np.int64)
            return _case(f"exact-fan-{'cw' if flipped else 'ccw'}", 16, 16, 16.0, IDENTITY, pts, faces[:, ::-1] if flipped else faces, seed, exact=True, bary=True)
        add(f"exact-fan-{'cw' if flipped else 'ccw'}", fan)

    def coplanar(seed):
        pts = _exact_points([[1, 1], [12, 2], [3, 12], [4, 3], [14, 8], [6, 14]])
        return _case("exact-coplanar", 16, 16, 16.0, IDENTITY, pts, np.array([[3, 4, 5], [0, 1, 2]], np.int64), seed, exact=True)
    add("exact-coplanar", coplanar)
    return B


BUILDERS = _builders()
CASES = list(BUILDERS)
# cases whose first seed left more than MAX_AMBIGUOUS of the pixels ambiguous draw their inputs from another seed
SEED_BUMP = {}
_MADE = {}


def make_case(name):
    if name not in _MADE:
        _MADE[name] = BUILDERS[name](1000 + 37 * CASES.index(name) + SEED_BUMP.get(name, 0))
    return _MADE[name]


_REFERENCE = {}


def reference(name, wrong=None):
    """the model's result of a case, computed once and shared"""
    if (name, wrong) not in _REFERENCE:
        c = make_case(name)
        _REFERENCE[(name, wrong)] = rasterise(c["vertices"], c["faces"], c["H"], c["W"], c["focal"], c["R"], c["t"], near=c["near"], cull=c["cull"], white=c["white"],
                                              uvs=c["uvs"], texture=c["texture"], colours=c["colours"], wrong=wrong)
    return _REFERENCE[(name, wrong)]
