"""Float64 numpy model of rf.bake_texture_from_views (rf_texture_project_views of include/relu_field.h), restated
independently: the atlas comes from tests/texture_model.py (texels ENUMERATED), the depth buffers from the brute-force rasteriser of
tests/mesh_raster_model.py, and the rule -- project, shadow-map test, angle weight, bilinear fetch, least-squares sums, division -- is
written out here over all texels and views at once.  Next to texture, weight and view count it returns the per-texel bound of
docs/texture_views_errors.md and the mask of AMBIGUOUS texels, those where float32 may take one of the rule's decisions the other
way.  The inputs the GPU test runs (``CASES`` / ``make_case``) live here too, so that the CPU tests can show on exactly those inputs
that few texels are ambiguous and that the comparison can fail."""
import numpy as np

from tests import mesh_raster_model as mrm
from tests import texture_model as tm
from tests.helpers import hash_uniform

UNIT = 2.0 ** -24  # float32 unit round-off
MAX_AMBIGUOUS = 0.01
WRONG = ("no_depth_test", "nearest_fetch", "no_half_shift", "y_not_flipped", "alphas_ignored")


def f32(x):
    return float(np.float32(x))


def _fetch(plane, x, y, nearest=None):
    """bilinear fetch of plane [H, W, C] at (x, y) [M], taps clamped: value [M, C], and (gx, gy) [M]: the largest difference between
    neighbouring taps of the 4 x 4 window around the fetch, per axis (what a shift of the fetch point by one pixel can change)"""
    H, W = plane.shape[:2]
    cl = lambda a, n: np.clip(a, 0, n - 1).astype(np.int64)  # noqa: E731
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    xa, xb, ya, yb = cl(x0, W), cl(x0 + 1, W), cl(y0, H), cl(y0 + 1, H)
    top = (1 - fx) * plane[ya, xa] + fx * plane[ya, xb]
    bot = (1 - fx) * plane[yb, xa] + fx * plane[yb, xb]
    value = (1 - fy) * top + fy * bot
    if nearest is not None:
        value = plane[cl(nearest[0], H), cl(nearest[1], W)]
    gx, gy = np.zeros(len(x)), np.zeros(len(x))
    for oy in range(-1, 3):
        for ox in range(-1, 3):
            here = plane[cl(y0 + oy, H), cl(x0 + ox, W)]
            gx = np.maximum(gx, np.abs(plane[cl(y0 + oy, H), cl(x0 + ox + 1, W)] - here).max(-1))
            gy = np.maximum(gy, np.abs(plane[cl(y0 + oy + 1, H), cl(x0 + ox, W)] - here).max(-1))
    return value, gx, gy


def project(vertices, faces, patch, views, images, depths, alphas=None, near=0.0, depth_bias=0.0, min_cos=0.1, cos_power=2, background=0.0,
            two_sided=False, fallback=None, min_weight=1e-3, cols=None, depth_bounds=None, depth_ambiguous=None, wrong=None):
    """The whole call in float64.  ``views``: a list of dict(H, W, focal, R, t) of one H x W; ``images`` [n, H, W, 3]; ``depths`` [n, H, W],
    the depth of the nearest face per pixel, inf where there is none (``depth_bounds`` its error, ``depth_ambiguous`` the pixels the
    raster model cannot decide); ``alphas`` [n, H, W] or None; ``fallback`` [Ht, Wt, 3] or None.  Returns a dict of [Ht, Wt, ..] arrays:
    ``texture``, ``weight``, ``views``, ``owned``, ``bound`` (of the texture) and ``weight_bound`` per texel, ``ambiguous``, and ``layout``.
    ``wrong``: one of the WRONG models the comparison must reject."""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    T, u = len(faces), UNIT
    near, depth_bias, min_cos, background, min_weight = f32(near), f32(depth_bias), f32(min_cos), f32(background), f32(min_weight)
    table = tm.texel_table(T, patch, cols)
    face = table["face"]
    Ht, Wt = face.shape
    owned = face >= 0
    M = int(owned.sum())
    base = np.zeros((Ht, Wt, 3)) if fallback is None else np.asarray(fallback, np.float64)
    out = dict(texture=base.copy(), weight=np.zeros((Ht, Wt)), views=np.zeros((Ht, Wt), np.int64), owned=owned, bound=np.zeros((Ht, Wt)),
               weight_bound=np.zeros((Ht, Wt)), ambiguous=np.zeros((Ht, Wt), bool), layout=table["layout"])
    if M == 0 or len(views) == 0:
        return out
    p = tm.texel_points(vertices, faces, table)[owned]
    tri = vertices[faces[face[owned]]]
    beta = table["beta"][owned]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cr = np.cross(e1, e2)
    clen = np.linalg.norm(cr, axis=-1)
    flat = clen == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(flat[:, None], 0.0, cr / clen[:, None])
        sin_theta = np.where(flat, 1.0, clen / (np.linalg.norm(e1, axis=-1) * np.linalg.norm(e2, axis=-1)))
    turn = np.where(flat, 0.0, 7.0 / sin_theta + 4.0) * u                     # |delta n| (docs/texture_errors.md)
    eps_p = 8.0 * u * (np.abs(beta) * np.abs(tri).max(-1)).sum(-1)              # |delta p|_inf
    S, Wsum, cnt = np.zeros((M, 3)), np.zeros(M), np.zeros(M, np.int64)
    E_S, E_W, A_S, A_W = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
    amb = np.zeros(M, bool)
    images = np.asarray(images, np.float64)
    for k, view in enumerate(views):
        H, W, f = int(view["H"]), int(view["W"]), f32(view["focal"])
        R, t = np.asarray(view["R"], np.float64).reshape(3, 3), np.asarray(view["t"], np.float64).reshape(3)
        d = p - t
        eps_d = eps_p[:, None] + u * np.abs(d)
        c = d @ R                                                               # c_a = sum_b d_b R_ba
        e_c = (eps_d @ np.abs(R)) + 4.0 * u * (np.abs(d) @ np.abs(R))
        z, e_z = -c[:, 2], e_c[:, 2]
        live = np.isfinite(z) & (z > near)
        amb |= np.abs(z - near) <= e_z
        zs = np.where(live, z, 1.0)
        zl = np.maximum(zs - e_z, 1e-300)
        x = W / 2 + f * c[:, 0] / zs
        y = H / 2 + f * c[:, 1] / zs if wrong == "y_not_flipped" else H / 2 - f * c[:, 1] / zs
        e_x = f / zl * (e_c[:, 0] + np.abs(c[:, 0]) / zl * e_z) + 4.0 * u * (np.abs(f * c[:, 0] / zs) + W / 2)
        e_y = f / zl * (e_c[:, 1] + np.abs(c[:, 1]) / zl * e_z) + 4.0 * u * (np.abs(f * c[:, 1] / zs) + H / 2)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        # the image border and the pixel boundaries are the integers: a coordinate within its error of one, next to the image
        around = (x > -0.5) & (x < W + 0.5) & (y > -0.5) & (y < H + 0.5)
        amb |= live & around & ((np.abs(x - np.round(x)) <= e_x) | (np.abs(y - np.round(y)) <= e_y))
        live &= inside
        dlen = np.maximum(np.linalg.norm(d, axis=-1), 1e-300)
        cs = -(n * d).sum(-1) / dlen
        if two_sided:
            cs = np.abs(cs)
        e_cos = np.where(flat, 0.0, turn + 2.0 * np.sqrt(3.0) * eps_d.max(-1) / dlen + 8.0 * u)
        amb |= live & ~flat & (np.abs(cs - min_cos) <= e_cos)
        live &= cs > min_cos
        j, i = np.clip(np.floor(x), 0, W - 1).astype(np.int64), np.clip(np.floor(y), 0, H - 1).astype(np.int64)
        zb = depths[k][i, j]
        hit = np.isfinite(zb)
        zbs = np.where(hit, zb, 0.0)
        dzb = (0.0 if depth_bounds is None else depth_bounds[k][i, j]) + 2.0 * u * (np.abs(zbs) + depth_bias)
        if depth_ambiguous is not None:
            amb |= live & depth_ambiguous[k][i, j]
        amb |= live & hit & (np.abs(z - (zbs + depth_bias)) <= e_z + dzb)
        live &= hit if wrong == "no_depth_test" else hit & (z <= zbs + depth_bias)
        # ---- the fetch and the terms (the bound: docs/texture_views_errors.md) ------------------------------------------------------
        shift = 0.0 if wrong == "no_half_shift" else 0.5
        nearest = (i, j) if wrong == "nearest_fetch" else None
        e_fx, e_fy = e_x + 2.0 * u * (np.abs(x) + 1.0), e_y + 2.0 * u * (np.abs(y) + 1.0)
        C, gx, gy = _fetch(images[k], x - shift, y - shift, nearest)
        e_C = gx * e_fx + gy * e_fy + 8.0 * u * np.abs(images[k]).max()
        if alphas is None or wrong == "alphas_ignored":
            m, e_m = np.ones(M), np.zeros(M)
        else:
            plane = np.asarray(alphas[k], np.float64)[..., None]
            mv, mgx, mgy = _fetch(plane, x - shift, y - shift, nearest)
            m, e_m = mv[:, 0], mgx * e_fx + mgy * e_fy + 8.0 * u * np.abs(plane).max()
        cs_live = np.where(live, cs, 1.0)
        omega = cs_live ** cos_power
        e_omega = cos_power * cs_live ** max(cos_power - 1, 0) * e_cos + (cos_power + 1) * u * omega if cos_power else np.zeros(M)
        rest, e_rest = (1.0 - m) * background, (e_m + 2.0 * u) * background
        diff = C - rest[:, None]
        term = (omega * m)[:, None] * diff
        dmax = np.abs(diff).max(-1)
        e_term = e_omega * np.abs(m) * dmax + omega * (e_m * dmax + np.abs(m) * (e_C + e_rest)) + 6.0 * u * omega * np.abs(m) * (np.abs(C).max(-1) + np.abs(rest))
        term_w = omega * m * m
        e_tw = e_omega * m * m + 2.0 * omega * np.abs(m) * e_m + 4.0 * u * term_w
        S += np.where(live[:, None], term, 0.0)
        Wsum += np.where(live, term_w, 0.0)
        cnt += live
        E_S += np.where(live, e_term, 0.0)
        E_W += np.where(live, e_tw, 0.0)
        A_S += np.where(live, np.abs(term).max(-1), 0.0)
        A_W += np.where(live, np.abs(term_w), 0.0)
    E_S = E_S + (cnt + 2) * u * A_S    # the running sums: (n + c) u sum |terms|
    E_W = E_W + (cnt + 2) * u * A_W
    seen = Wsum > min_weight
    amb |= (cnt > 0) & (np.abs(Wsum - min_weight) <= E_W)
    amb |= seen & ~(Wsum - E_W > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        tex = np.where(seen[:, None], S / np.where(seen, Wsum, 1.0)[:, None], base[owned])
        tmax = np.abs(tex).max(-1)
        bound = np.where(seen, (E_S + tmax * E_W) / np.maximum(Wsum - E_W, 1e-300) + 2.0 * u * tmax, 0.0)  # the final division
    out["texture"][owned], out["weight"][owned], out["views"][owned] = tex, Wsum, cnt
    out["bound"][owned], out["weight_bound"][owned], out["ambiguous"][owned] = bound, E_W, amb
    return out


def compare(ref, texture, weight, views, exact=False):
    """Assert a result (arrays like the model's) against ``ref`` on the owned texels that are not ambiguous -- on EVERY texel, bit for
    bit in float32, when ``exact``; unowned texels must hold the fallback (or 0), weight 0 and 0 views.  Returns the worst error / bound."""
    texture, weight, views = np.asarray(texture, np.float64), np.asarray(weight, np.float64), np.asarray(views, np.int64)
    owned = ref["owned"]
    assert texture.shape == ref["texture"].shape and weight.shape == owned.shape and views.shape == owned.shape
    assert np.array_equal(texture[~owned], ref["texture"][~owned]) and (weight[~owned] == 0).all() and (views[~owned] == 0).all(), "unowned texels"
    if exact:
        assert np.array_equal(views, ref["views"]), "views"
        assert np.array_equal(texture.astype(np.float32), ref["texture"].astype(np.float32)), "texture"
        assert np.array_equal(weight.astype(np.float32), ref["weight"].astype(np.float32)), "weight"
        return 0.0
    take = owned & ~ref["ambiguous"]
    assert np.array_equal(views[take], ref["views"][take]), f"views: {int((views[take] != ref['views'][take]).sum())} texels differ"
    err_t = np.abs(texture - ref["texture"]).max(-1)
    err_w = np.abs(weight - ref["weight"])
    assert (err_t[take] <= ref["bound"][take]).all(), f"texture: worst error {err_t[take].max():.3e}, over its bound by up to {(err_t[take] - ref['bound'][take]).max():.3e}"
    assert (err_w[take] <= ref["weight_bound"][take]).all(), f"weight: worst error {err_w[take].max():.3e}, over its bound by up to {(err_w[take] - ref['weight_bound'][take]).max():.3e}"
    worst = 0.0
    for err, bound in ((err_t, ref["bound"]), (err_w, ref["weight_bound"])):
        nz = take & (bound > 0)
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
    return worst


def depth_keys(depths):
    """uint64 [n, H, W] as rf_mesh_raster_visibility writes them, from the MODEL's depths: float32 bits of z << 32 (face word 0), all
    ones where nothing was hit -- returned as int64 (the same bits), which torch can hold"""
    z = np.asarray(depths, np.float64)
    bits = np.where(np.isfinite(z), z, 0.0).astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)
    return np.where(np.isfinite(z), bits, np.uint64(0xFFFFFFFFFFFFFFFF)).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test (tests/test_hip_texture_views.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def octahedron(level, seed, jitter=0.04):
    """a subdivided octahedron on the unit sphere, 8 * 4^level faces that share vertices, (v1 - v0) x (v2 - v0) pointing outward; the
    vertices jittered (an unjittered one projects texels exactly onto pixel boundaries)"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(q, np.float64) for q in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                q = v[a] + v[b]
                v.append(q / np.linalg.norm(q))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    v = np.array(v) + jitter * hash_uniform((len(v), 3), seed).astype(np.float64)
    return v.astype(np.float32), np.array(f, np.int64)


def look_at(eye, target, seed=None):
    """R [3, 3] float32 (columns: right, up, backwards -- the camera looks along -R[:, 2]) and t = eye"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(right, fwd), -fwd], axis=1).astype(np.float32), eye.astype(np.float32)


def orbit_views(n, H, W, seed, centre=(0.0, 0.0, 0.0), towards=None, radius=3.0):
    """n cameras on a sphere around ``centre`` looking at it (all on the side of ``towards`` when given), focals so that a unit ball fills
    most of the image"""
    dirs = hash_uniform((n, 3), seed).astype(np.float64)
    if towards is not None:
        dirs = np.asarray(towards, np.float64) / np.linalg.norm(towards) + 0.45 * dirs
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    views = []
    for k in range(n):
        rad = radius * (1.0 + 0.1 * float(hash_uniform((1,), seed + 100 + k)[0]))
        eye = np.asarray(centre) + rad * dirs[k]
        R, t = look_at(eye, np.asarray(centre) + 0.05 * hash_uniform((3,), seed + 200 + k).astype(np.float64))
        focal = f32(1.2 * min(H, W) * (1.0 + 0.1 * float(hash_uniform((1,), seed + 300 + k)[0])))
        views.append(dict(H=H, W=W, focal=focal, R=R, t=t))
    return views


# name: faces (octahedron level, faces kept), patch, H, W, views, alphas, background, cos_power, two_sided, fallback, extras
SPECS = {
    "oct32-P4-40x40-v3":          dict(level=1, T=32, patch=4, H=40, W=40, n=3, power=2),
    "oct128-P4-48x64-v2-alpha":   dict(level=2, T=128, patch=4, H=48, W=64, n=2, alphas=True, background=1.0, power=8, fallback=True),
    "oct128-P8-37x53-v2":         dict(level=2, T=128, patch=8, H=37, W=53, n=2, power=2, fallback=True),
    "oct128-P2-24x40-v1-pow0":    dict(level=2, T=128, patch=2, H=24, W=40, n=1, power=0),
    "oct128-P3-24x40-v16-alpha":  dict(level=2, T=128, patch=3, H=24, W=40, n=16, alphas=True, power=2),
    "oct128-P4-1x1-v2":           dict(level=2, T=128, patch=4, H=1, W=1, n=2, power=2, min_cos=0.0),
    "oct31-P4-40x40-v17":         dict(level=1, T=31, patch=4, H=40, W=40, n=17, alphas=True, power=2, fallback=True, behind=3, nothing=11),
    "tri1-P8-24x40-v2":           dict(level=0, T=1, patch=8, H=24, W=40, n=2, power=2, facing=True),
    "tri2-P8-37x53-v2":           dict(level=0, T=2, patch=8, H=37, W=53, n=2, power=0, facing=True, alphas=True, background=1.0),
    "tri3-P4-24x40-v3":           dict(level=0, T=3, patch=4, H=24, W=40, n=3, power=8, facing=True, fallback=True),
    "oct32-P3-zero-area":         dict(level=1, T=32, patch=3, H=37, W=53, n=2, power=2, zero_area=3, facing=True),
    "oct32-P4-flipped-one-sided": dict(level=1, T=32, patch=4, H=37, W=53, n=2, power=2, flipped=3, facing=True, alphas=True, background=1.0, seed=4242),
    "oct32-P4-flipped-two-sided": dict(level=1, T=32, patch=4, H=37, W=53, n=2, power=2, flipped=3, facing=True, alphas=True, background=1.0, seed=4242, two_sided=True),
    "oct32-P4-near":              dict(level=1, T=32, patch=4, H=40, W=40, n=2, power=2, near=2.7, depth_bias=0.05),
}
CASES = list(SPECS)
# cases whose first seed left more than MAX_AMBIGUOUS of the owned texels ambiguous draw their inputs from another seed
SEED_BUMP = {}
_MADE, _REFERENCE = {}, {}


def make_case(name):
    if name in _MADE:
        return _MADE[name]
    spec = SPECS[name]
    seed = spec.get("seed", 3000 + 41 * CASES.index(name)) + SEED_BUMP.get(name, 0)
    vertices, faces = octahedron(spec["level"], seed)
    faces = faces[:spec["T"]].copy()
    if "zero_area" in spec:
        faces[spec["zero_area"], 1] = faces[spec["zero_area"], 0]  # e1 = 0 exactly
    if "flipped" in spec:
        faces[spec["flipped"]] = faces[spec["flipped"], ::-1]
    H, W, n = spec["H"], spec["W"], spec["n"]
    views = orbit_views(n, H, W, seed + 1, towards=(1.0, 1.0, 1.0) if spec.get("facing") else None)
    if H == 1:
        for view in views:
            view["focal"] = 0.5
    if "behind" in spec:   # the mesh lies behind this camera
        k = spec["behind"]
        views[k]["R"], views[k]["t"] = look_at(views[k]["t"], 2.0 * views[k]["t"].astype(np.float64))
    if "nothing" in spec:  # this camera looks past the mesh
        k = spec["nothing"]
        eye = views[k]["t"].astype(np.float64)
        side = np.cross(eye, [0.3, -0.5, 0.8])
        views[k]["R"], views[k]["t"] = look_at(eye, eye + 3.0 * side / np.linalg.norm(side) - 0.4 * eye)
    images = hash_uniform((n, H, W, 3), seed + 2, 0.0, 1.0)
    alphas = hash_uniform((n, H, W), seed + 3, 0.25, 1.0) if spec.get("alphas") else None
    lay = tm.layout(len(faces), spec["patch"])
    fallback = hash_uniform((lay["height"], lay["width"], 3), seed + 4, 0.0, 1.0) if spec.get("fallback") else None
    corners = vertices.astype(np.float64)[faces]
    default_bias = f32(np.linalg.norm(corners - np.roll(corners, 1, axis=1), axis=-1).mean())  # the Python layer's default: the mean edge length
    made = dict(name=name, vertices=vertices, faces=faces, patch=spec["patch"], views=views, images=images, alphas=alphas, fallback=fallback,
                near=spec.get("near", 0.0), depth_bias=spec.get("depth_bias", default_bias), default_bias="depth_bias" not in spec,
                min_cos=spec.get("min_cos", 0.1), cos_power=spec["power"], background=spec.get("background", 0.0), two_sided=spec.get("two_sided", False),
                min_weight=1e-3)
    _MADE[name] = made
    return made


def depth_buffers(made):
    """(depths [n, H, W] with inf where nothing is hit, their bounds, the raster model's ambiguous pixels) of a case's views"""
    depths, bounds, ambiguous = [], [], []
    for view in made["views"]:
        r = mrm.rasterise(made["vertices"], made["faces"], view["H"], view["W"], view["focal"], view["R"], view["t"], near=made["near"])
        depths.append(np.where(r["mask"], r["depth"], np.inf))
        bounds.append(r["depth_bound"])
        ambiguous.append(r["ambiguous"])
    return np.stack(depths), np.stack(bounds), np.stack(ambiguous)


def project_case(made, depths, bounds=None, ambiguous=None, wrong=None):
    return project(made["vertices"], made["faces"], made["patch"], made["views"], made["images"], depths, made["alphas"], made["near"], made["depth_bias"],
                   made["min_cos"], made["cos_power"], made["background"], made["two_sided"], made["fallback"], made["min_weight"],
                   depth_bounds=bounds, depth_ambiguous=ambiguous, wrong=wrong)


def reference(name, wrong=None):
    """(the model's result of a case, its depth buffers), computed once and shared"""
    if (name, wrong) not in _REFERENCE:
        made = make_case(name)
        if (name, "depth") not in _REFERENCE:
            _REFERENCE[(name, "depth")] = depth_buffers(made)
        depths, bounds, ambiguous = _REFERENCE[(name, "depth")]
        _REFERENCE[(name, wrong)] = (project_case(made, depths, bounds, ambiguous, wrong), depths)
    return _REFERENCE[(name, wrong)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the crafted exact cases: identity pose, focal 16, a 16 x 16 image, dyadic vertices, patch 5, cos_power 0 -- every float32 operation
# of the kernel is exact, every texel is compared bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
EXACT_PATCH, EXACT_SENTINEL = 5, (0.75, 0.5, 0.25)
# corners in pixel coordinates (column, row), wound so that the normal faces the camera
EXACT_FRONT = np.array([[3.0, 3.5], [3.5, 13.0], [13.5, 4.0]])    # at depth 4
EXACT_BACK = np.array([[1.5, 1.5], [2.5, 13.5], [13.5, 2.5]])      # at depth 8, larger
EXACT_CASES = ("exact-one", "exact-two")


def ramp_image():
    """[1, 16, 16, 3] float32, affine in (column j, row i) with dyadic coefficients; ``ramp`` is its closed form"""
    i, j = np.meshgrid(np.arange(16.0), np.arange(16.0), indexing="ij")
    return ramp(j, i).astype(np.float32)[None]


def ramp(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([x / 32.0, y / 32.0, 0.125 + x / 64.0 + y / 64.0], axis=-1)


def make_exact(name):
    two = name == "exact-two"
    pix = [EXACT_FRONT] + ([EXACT_BACK] if two else [])
    depth = [4.0] + ([8.0] if two else [])
    vertices = np.concatenate([mrm._exact_points(q, Z=z) for q, z in zip(pix, depth)])
    faces = np.arange(len(vertices), dtype=np.int64).reshape(-1, 3)
    R, t = mrm.IDENTITY
    lay = tm.layout(len(faces), EXACT_PATCH)
    fallback = np.broadcast_to(np.array(EXACT_SENTINEL, np.float32), (lay["height"], lay["width"], 3)).copy() if two else None
    return dict(name=name, vertices=vertices, faces=faces, patch=EXACT_PATCH, views=[dict(H=16, W=16, focal=16.0, R=R, t=t)], images=ramp_image(), alphas=None,
                fallback=fallback, near=0.0, depth_bias=0.5 if two else 0.0, default_bias=False, min_cos=0.1, cos_power=0, background=0.0, two_sided=False,
                min_weight=1e-3, pixels=pix, depth=depth)


def exact_expectation(made, face_ids, depths):
    """The closed form of an exact case, from the raster model's face ids and depths [16, 16] alone: per texel its class ("seen",
    "occluded", "empty", "outside", "unowned") and its expected texel, weight and view count.  A texel of a face at depth Z whose
    centre has the pixel coordinates q = sum_k beta_k q_k projects to x = q + 1/2; it is seen when pixel floor(x) holds a face no nearer
    than Z - depth_bias, and then holds ramp(q) -- bilinear interpolation reproduces affine functions -- with q clamped to the pixel centres
    [0, 15]: clamping the taps of an affine image is clamping the coordinate."""
    table = tm.texel_table(len(made["faces"]), made["patch"])
    face, beta = table["face"], table["beta"]
    Ht, Wt = face.shape
    base = np.zeros((Ht, Wt, 3)) if made["fallback"] is None else made["fallback"].astype(np.float64)
    texture, weight, views = base.copy(), np.zeros((Ht, Wt)), np.zeros((Ht, Wt), np.int64)
    kind = np.full((Ht, Wt), "unowned", dtype=object)
    for r in range(Ht):
        for c in range(Wt):
            t = face[r, c]
            if t < 0:
                continue
            q = beta[r, c] @ made["pixels"][t]
            x, y = q[0] + 0.5, q[1] + 0.5
            if not (0 <= x < 16 and 0 <= y < 16):
                kind[r, c] = "outside"
                continue
            i, j = int(np.floor(y)), int(np.floor(x))
            if face_ids[i, j] < 0:
                kind[r, c] = "empty"
            elif not made["depth"][t] <= depths[i, j] + made["depth_bias"]:
                kind[r, c] = "occluded"
            else:
                kind[r, c] = "seen"
                texture[r, c], weight[r, c], views[r, c] = ramp(min(max(q[0], 0.0), 15.0), min(max(q[1], 0.0), 15.0)), 1.0, 1
    return dict(kind=kind, texture=texture, weight=weight, views=views, owned=face >= 0)
