"""Float64 model of rf_render_geometry (include/relu_field.h).

Built on tests/node_weights_model.py: ``sample_geometry`` supplies the oracle's float32 z, points, inside masks and deltas -- they
decide WHICH samples and cells there are, and the kernel reproduces them in float32 -- and ``sample_weights`` the float64 compositing
weights w_i = T_i alpha_i.  New here, all float64: the gradient of the trilinear interpolant of the pre-activation density with
respect to the point, the per-sample normal n_i = -g_i / |g_i| (0 where g_i = 0), N64 = sum_i w_i n_i, the accumulated opacity
C_i = 1 - T_{i+1} and the quantile index i* = the first i with C_i >= q (-1: none).

The rounding bound of the composited normal, per ray:

    bound_r = TOL + sum_i |w_i| min(2, 2 |e_i| / |g_i|),      e_{i,a} = KAPPA 2^-24 sum_k |v_k| |c_{a,k}| dims_a norm_scale_a / 2

c_{a,k} = corner k's coefficient in gradient component a (+- the product of the two other axes' weights), v_k the corner's
pre-activation value (0 outside the grid).  A perturbation e of g turns the unit vector by at most 2 |e| / |g| (and two unit vectors
differ by at most 2); TOL = 1e-5 is the project's bar on sum_i w_i, which covers what the weights themselves are off by.  KAPPA = 8 is
COUNTED from render_geometry_kernel, the roundings a term v_k c_{a,k} of the gradient sum passes through: raw * rho (1), the difference
of the two corner values along the axis (2), the product of the two other axes' weights (3), difference * that product (4), the two
levels of the pairwise sum of the four terms (5, 6), the constant dims_a * norm_scale_a (7; the halving is exact) and the scaling by
it (8).  It is not fitted to any result."""
import numpy as np
import torch

from oracle import relu_field_oracle as orc
from tests import node_weights_model as nm

TOL = 1e-5
KAPPA = 8
UNIT = 2.0 ** -24
BOUND_CAP = 1e-3  # rays whose bound exceeds this say nothing about the kernel: they may be left out (at most 2 % of the rays with acc > 0.01)
QUANTILE_BAND = 1e-5  # |C - q| below this at i* or i* - 1: float32 may cross one sample earlier or later (at most 1 % of the rays)


def cell_geometry(points, aabb, dims):
    """per-axis geometry of float32 points [M,3]: (i0 [3][M] int64, lo [3][M], hi [3][M] float64).  WHICH cell a sample lies in is the
    oracle's float32 decision, like which samples there are (floor of the float32 continuous index, the arithmetic of
    relu_field_oracle.trilinear_recipe): the gradient of a piecewise trilinear field jumps across a cell face, and a sample within a
    rounding of one belongs to the cell float32 puts it in.  The weights are float64, of the float64 index relative to that cell (a
    sample a rounding beyond the face has a weight a rounding outside [0, 1]: the cell's own polynomial, continued)."""
    q32 = orc.normalise_points(points.to(torch.float32), aabb)
    q = orc.normalise_points(points.double(), aabb).numpy()
    i0, lo, hi = [], [], []
    for a in range(3):
        idx32 = ((q32[:, a] + 1.0) * dims[a] - 1.0) / 2.0
        assert idx32.dtype == torch.float32
        cell = np.floor(idx32.numpy()).astype(np.int64)
        idx = ((q[:, a] + 1.0) * dims[a] - 1.0) / 2.0
        i0.append(cell)
        hi.append(idx - cell)
        lo.append(1.0 - (idx - cell))
    return i0, lo, hi


def gradient_terms(densities, aabb, rho, mode, points):
    """float64: (g [M,3] world-space gradient of the interpolated pre-activation density at float32 points [M,3],
    spread [M,3] = sum_k |v_k| |c_{a,k}| dims_a norm_scale_a / 2, the magnitude the rounding bound scales with)"""
    dims = tuple(densities.shape[:3])
    X, Y, Z = dims
    i0, lo, hi = cell_geometry(points, aabb, dims)
    pre = densities.double().numpy().reshape(-1) * float(np.float32(rho))
    if mode == "abs":
        pre = np.abs(pre)
    consts = orc.normalisation_constants(aabb)
    scale = [dims[a] * float(consts[a][0]) / 2.0 for a in range(3)]
    g = np.zeros((points.shape[0], 3))
    spread = np.zeros((points.shape[0], 3))
    for k in range(8):
        d = (k & 1, (k >> 1) & 1, k >> 2)
        c = [i0[a] + d[a] for a in range(3)]
        ok = (c[0] >= 0) & (c[0] < X) & (c[1] >= 0) & (c[1] < Y) & (c[2] >= 0) & (c[2] < Z)
        lin = (np.clip(c[0], 0, X - 1) * Y + np.clip(c[1], 0, Y - 1)) * Z + np.clip(c[2], 0, Z - 1)
        v = np.where(ok, pre[lin], 0.0)
        wt = [hi[a] if d[a] else lo[a] for a in range(3)]
        for a in range(3):
            b, c2 = [x for x in range(3) if x != a]
            coeff = (1.0 if d[a] else -1.0) * wt[b] * wt[c2] * scale[a]
            g[:, a] += v * coeff
            spread[:, a] += np.abs(v) * np.abs(coeff)
    return g, spread


def unit_normals(g, sign=-1.0):
    """n = sign * g / |g| per row, 0 where g = 0"""
    norm = np.linalg.norm(g, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(norm > 0, sign * g / norm, 0.0)


def model(densities, aabb, rho, mode, origins, directions, near, far, num_samples, quantile=0.5, optimized_sampling=False, t_rand=None,
          wrong=None):
    """The whole pass for one ray batch, float64.  Returns a dict: ``acc`` [N], ``normal`` [N,3] = N64, ``bound`` [N] = bound_r,
    ``z`` [N,S] (float32 ray parameters), ``C`` [N,S], ``istar`` [N] (-1: no crossing), ``depth`` [N] = z[i*] or 0, ``ambiguous`` [N]
    bool (|C - q| <= QUANTILE_BAND at i* or i* - 1), ``w`` [N,S].
    ``wrong``: one of the WRONG models the bound must reject -- "unnormalised" (N = -sum w_i g_i), "plus_gradient" (n_i = +g/|g|),
    "drop_transmittance" (w_i = alpha_i)."""
    z, pts, inside, deltas = nm.sample_geometry(origins, directions, aabb, near, far, num_samples, optimized_sampling, t_rand)
    n, S = inside.shape
    w, _, _, _ = nm.sample_weights(densities, aabb, rho, mode, pts, inside, deltas, drop_transmittance=(wrong == "drop_transmittance"))
    g, spread = gradient_terms(densities, aabb, rho, mode, pts.reshape(-1, 3))
    if wrong == "unnormalised":
        ni = -g
    else:
        ni = unit_normals(g, +1.0 if wrong == "plus_gradient" else -1.0)
    ni = ni.reshape(n, S, 3)
    live = w != 0  # a sample without weight contributes nothing, whatever its gradient
    normal = np.where(live[..., None], w[..., None] * ni, 0.0).sum(1)
    gn = np.linalg.norm(g, axis=-1).reshape(n, S)
    en = np.linalg.norm(KAPPA * UNIT * spread, axis=-1).reshape(n, S)
    with np.errstate(invalid="ignore", divide="ignore"):
        turn = np.where(en > 0, np.minimum(2.0, 2.0 * en / gn), 0.0)
    bound = TOL + (np.abs(w) * turn).sum(-1)
    # accumulated opacity through sample i from the TRUE weights' alphas (samples outside the box: alpha = 0)
    w_true = w if wrong != "drop_transmittance" else nm.sample_weights(densities, aabb, rho, mode, pts, inside, deltas)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        C = np.cumsum(w_true, axis=-1)  # sum_{j<=i} T_j alpha_j = 1 - T_{i+1} (telescoping)
    hit = C >= quantile
    any_hit = hit.any(-1)
    istar = np.where(any_hit, hit.argmax(-1), -1)
    rows = np.arange(n)
    z64 = z.numpy().astype(np.float64)
    depth = np.where(any_hit, z64[rows, np.maximum(istar, 0)], 0.0)
    c_at = np.where(any_hit, C[rows, np.maximum(istar, 0)], np.inf)
    c_before = np.where(istar > 0, C[rows, np.maximum(istar - 1, 0)], np.where(istar == 0, 0.0, np.inf))
    ambiguous = (np.abs(c_at - quantile) <= QUANTILE_BAND) | (np.abs(c_before - quantile) <= QUANTILE_BAND)
    return {"acc": w_true.sum(-1), "normal": normal, "bound": bound, "z": z.numpy(), "C": C, "istar": istar, "depth": depth,
            "ambiguous": ambiguous, "w": w, "inside": inside.numpy()}


# --------------------------------------------------------------------------------------------
# float32 restatement of the kernel's arithmetic (numpy; sequential sums where the kernel's are wave-parallel)
# --------------------------------------------------------------------------------------------
def emulate_float32(densities, aabb, rho, mode, origins, directions, near, far, num_samples, optimized_sampling=False, t_rand=None, samples=False):
    """(N32 [N,3], acc32 [N]) with the kernel's formulas and operation order in float32: locate's index arithmetic and per-axis
    weights, raw * rho, the pairwise sum of the four difference terms per axis, the scaling, the normalisation by the largest
    component first; alpha, T and w as in tests/distortion_model.emulate_float32."""
    f = np.float32
    _, pts, inside, deltas = nm.sample_geometry(origins, directions, aabb, near, far, num_samples, optimized_sampling, t_rand)
    n, S = inside.shape
    dims = tuple(densities.shape[:3])
    X, Y, Z = dims
    consts = orc.normalisation_constants(aabb)
    p = pts.numpy().reshape(-1, 3).astype(f)
    i0, w0, w1 = [], [], []
    for a in range(3):
        q = (p[:, a] * consts[a][0]).astype(f) + consts[a][1]
        idx = ((((q + f(1)).astype(f) * f(dims[a])).astype(f) - f(1)).astype(f) / f(2)).astype(f)
        fl = np.floor(idx).astype(f)
        i0.append(fl.astype(np.int64))
        w1.append((idx - fl).astype(f))
        w0.append(((fl + f(1)).astype(f) - idx).astype(f))
    raw = densities.numpy().reshape(-1).astype(f)
    v, oks = [], []
    for k in range(8):
        d = (k & 1, (k >> 1) & 1, k >> 2)
        c = [i0[a] + d[a] for a in range(3)]
        ok = (c[0] >= 0) & (c[0] < X) & (c[1] >= 0) & (c[1] < Y) & (c[2] >= 0) & (c[2] < Z)
        lin = (np.clip(c[0], 0, X - 1) * Y + np.clip(c[1], 0, Y - 1)) * Z + np.clip(c[2], 0, Z - 1)
        vk = (raw[lin] * f(rho)).astype(f)
        if mode == "abs":
            vk = np.abs(vk)
        v.append(np.where(ok, vk, f(0)).astype(f))
        oks.append(ok)
    # the density sum in ATen's corner order with corners_of's weights (masked per axis, (x * y) * z)
    acc = np.zeros(p.shape[0], dtype=f)
    for k in range(8):
        d = (k & 1, (k >> 1) & 1, k >> 2)
        wt = [(w1[a] if d[a] else w0[a]) for a in range(3)]
        b = ((wt[0] * wt[1]).astype(f) * wt[2]).astype(f)
        acc = (acc + (v[k] * np.where(oks[k], b, f(0))).astype(f)).astype(f)
    ins = inside.numpy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if mode == "relu":
            sigma = np.maximum(acc, f(0))
        elif mode == "softplus":
            sigma = np.where(acc > 20, acc, np.log1p(np.exp(np.minimum(acc, f(20))))).astype(f)
        else:
            sigma = acc
        sigma = np.where(ins.reshape(-1), sigma, f(0)).astype(f).reshape(n, S)
        delta = deltas.numpy().astype(f)
        E = np.exp(-(sigma * delta).astype(f)).astype(f)
        T = np.cumprod(np.concatenate([np.ones((n, 1), dtype=f), E], axis=-1), axis=-1, dtype=f)[:, :-1]
        w = np.where(ins, ((f(1) - E) * T).astype(f), f(0)).astype(f)
        gw = []
        for a, (b, c2) in enumerate(((1, 2), (0, 2), (0, 1))):
            step = 1 << a
            lows = [k for k in range(8) if not k & step]  # ascending: (second axis, third axis) = (0,0), (1,0), (0,1), (1,1)
            terms = []
            for k in lows:
                db, dc = (k >> b) & 1, (k >> c2) & 1
                wb, wc = (w1[b] if db else w0[b]), (w1[c2] if dc else w0[c2])
                terms.append(((v[k + step] - v[k]).astype(f) * (wb * wc).astype(f)).astype(f))
            s = ((terms[0] + terms[1]).astype(f) + (terms[2] + terms[3]).astype(f)).astype(f)
            gw.append((s * ((f(dims[a]) * consts[a][0]).astype(f) * f(0.5)).astype(f)).astype(f))
        big = np.maximum(np.maximum(np.abs(gw[0]), np.abs(gw[1])), np.abs(gw[2]))
        safe = np.where(big > 0, big, f(1))
        u = [(gw[a] / safe).astype(f) for a in range(3)]
        length = np.sqrt((((u[0] * u[0]).astype(f) + (u[1] * u[1]).astype(f)).astype(f) + (u[2] * u[2]).astype(f)).astype(f)).astype(f)
        length = np.where(big > 0, length, f(1))
        N = np.zeros((n, 3), dtype=f)
        wf = w.reshape(-1)
        for a in range(3):
            na = -(u[a] / length).astype(f)
            part = np.where((wf != 0) & (big > 0), (wf * na).astype(f), f(0)).astype(f).reshape(n, S)
            for i in range(S):
                N[:, a] = (N[:, a] + part[:, i]).astype(f)
        acc32 = np.zeros(n, dtype=f)
        for i in range(S):
            acc32 = (acc32 + w[:, i]).astype(f)
    if samples:  # (for diagnosis: the per-sample weights and world gradients)
        return N, acc32, w, np.stack(gw, -1).reshape(n, S, 3)
    return N, acc32


# --------------------------------------------------------------------------------------------
# the cases of the kernel comparison (tests/test_hip_geometry.py runs them, tests/test_geometry_model.py checks their conditions)
# --------------------------------------------------------------------------------------------
STORAGES = ["reference", "split", "bricked"]
MODES = ["relu", "softplus", "abs", "identity"]
DIMS = [(5, 6, 7), (9, 10, 17)]  # the second crosses an 8-node brick on every axis
SAMPLES = [1, 63, 64, 65, 130]
FEATURES = [3, 27]
OPTIONS = ["plain", "aabb", "occupancy", "t_rand", "keyed", "camera"]
RAYS = 96
CAMERA_HW = (8, 12)
CAMERA_FOCAL = {(5, 6, 7): 12.0, (9, 10, 17): 16.0}  # about a quarter of the frame misses the box
CAMERA_RADIUS = 4.0
JITTER_KEY = 0xC0FFEE1234
JITTER_FIRST = 5
QUANTILE = 0.5


def voxel_of(dims):
    return (3.0 / max(dims),) * 3


def rho_of(mode):
    return 100.0 / 3.0


def kernel_cases():
    """(dims, storage, S, F, mode, option): dims x storage x S in full, the other factors dealt out so that every value of every
    factor occurs (asserted by tests/test_hip_geometry.py and, without a GPU, by tests/test_geometry_model.py).  Two substitutions at
    S = 1, where the deal would give a case with nothing to compare: "aabb" becomes "plain" (the one sample would sit ON the box) and
    "identity" becomes "softplus" (the one sample carries the 1e10 interval: a negative density there is alpha = -inf in the reference
    itself).  Under the identity mode the blob also has a radius of its own (blob_radius)."""
    cases = []
    for j, (dims, storage) in enumerate((d, st) for d in DIMS for st in STORAGES):
        for s, S in enumerate(SAMPLES):
            option = OPTIONS[(j + s) % 6]
            if S == 1 and option == "aabb":  # (the one sample would sit ON the box: t = t_enter -- nothing to compare)
                option = "plain"
            mode = MODES[(j + 2 * s + j // 4) % 4]
            if S == 1 and mode == "identity":  # (the one sample carries the 1e10 interval: a negative density there is alpha = -inf)
                mode = "softplus"
            cases.append((dims, storage, S, FEATURES[(j + s // 2) % 2], mode, option))
    return cases


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


_CACHE = {}


def blob_radius(dims, mode):
    """r of the blob.  0.9 of the smallest half extent: the zero level lies inside the box, surfaces exist under ReLU / |.|.  Under the
    identity a negative density is an amplifying medium (alpha < 0), and one at a ray's last sample, whose interval is 1e10 long, is
    alpha = -inf in the reference itself: there r is the box's half diagonal / 0.55 -- the field is positive but for pockets of
    slightly negative density in the box's corners."""
    half = [n * v / 2.0 for n, v in zip(dims, voxel_of(dims))]
    return float(np.linalg.norm(half)) / 0.55 if mode == "identity" else 0.9 * min(half)


def blob_grid(dims, F, mode, seed=33):
    """densities [X,Y,Z,1] = 0.6 - |p| / r + 0.1 U(-1,1) at the node positions p (r: blob_radius), features U(-1,1) [X,Y,Z,F]"""
    from tests.helpers import hash_uniform

    key = ("grid", dims, F, mode == "identity", seed)
    if key not in _CACHE:
        vox = voxel_of(dims)
        ax = [(np.arange(n, dtype=np.float64) + 0.5 - n / 2.0) * v for n, v in zip(dims, vox)]
        dist = np.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
        dens = (0.6 - dist / blob_radius(dims, mode) + 0.1 * hash_uniform(dims, seed)).astype(np.float32)[..., None]
        _CACHE[key] = (torch.from_numpy(dens), torch.from_numpy(hash_uniform(dims + (F,), seed + 1)))
    return _CACHE[key]


def camera_pose():
    import thr3ed_atom_amd as rf

    return rf.pose_spherical(40.0, -35.0, CAMERA_RADIUS)


def case_rays(dims, S, option):
    """(origins [96,3], directions [96,3], near, far).  "camera": the 8 x 12 pixel rays of a wide posed camera (the frame is wider than
    the box).  Otherwise a ray list: 64 rays from a sphere of radius 4 aimed into the box, 24 that miss it (half point away from it,
    half pass beside it), 8 that START inside it (short directions, so that the sampled span leaves the box again).  Directions are
    not normalised: z = 4 is the aim point.  A single-sample ray samples z = near, so near is the aim point there."""
    from tests.helpers import hash_uniform

    key = ("rays", dims, S == 1, option == "camera")
    if key not in _CACHE:
        near, far = (4.0 if S == 1 else 2.0), 6.0
        if option == "camera":
            pose = camera_pose()
            o, d = orc.cast_rays(CAMERA_HW[0], CAMERA_HW[1], CAMERA_FOCAL[dims], torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))
            o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
        else:
            half = np.array([n * v / 2.0 for n, v in zip(dims, voxel_of(dims))])
            unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)  # noqa: E731
            o = 4.0 * unit(hash_uniform((RAYS, 3), 401).astype(np.float64))
            aim = 0.6 * half * hash_uniform((RAYS, 3), 402)
            beside = 3.2 * unit(np.cross(o, hash_uniform((RAYS, 3), 403)))  # perpendicular to the line to the centre, far outside the box
            d = (aim - o) / 4.0
            d[64:76] = o[64:76] / 4.0 + 0.05 * hash_uniform((12, 3), 404)  # away from the box
            d[76:88] = (beside[76:88] - o[76:88]) / 4.0
            o[88:] = 0.3 * half * hash_uniform((8, 3), 405)
            d[88:] = 0.6 * unit(hash_uniform((8, 3), 406).astype(np.float64))
            o, d = torch.from_numpy(o.astype(np.float32)).contiguous(), torch.from_numpy(d.astype(np.float32)).contiguous()
        _CACHE[key] = (o, d, float(np.float32(near)), float(np.float32(far)))
    return _CACHE[key]


def case_jitter(S, option):
    from tests.helpers import hash_uniform

    if option == "t_rand":
        return torch.from_numpy(hash_uniform((RAYS, S), 77, 0.0, 1.0))
    if option == "keyed":
        return torch.from_numpy(orc.keyed_jitter(JITTER_KEY, JITTER_FIRST, RAYS, S).astype(np.float32))
    return None


def case_reference(dims, F, mode, S, option, quantile=QUANTILE):
    """the model dict of a case -- computed once per (case, quantile), never modified; the storage does not enter"""
    key = ("ref", dims, F, mode, S, option, quantile)
    if key not in _CACHE:
        dens, _ = blob_grid(dims, F, mode)
        o, d, near, far = case_rays(dims, S, option)
        _CACHE[key] = model(dens, orc.make_aabb(dims, voxel_of(dims)), rho_of(mode), mode, o, d, near, far, S, quantile=quantile,
                            optimized_sampling=(option == "aabb"), t_rand=case_jitter(S, option))
    return _CACHE[key]
