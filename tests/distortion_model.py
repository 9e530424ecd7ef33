"""Float64 model of rf_distortion (include/relu_field.h).

Sample positions, inside masks and interval lengths come from the oracle's float32 restatement of the sampler through
tests/node_weights_model.py, as in the parity tests: they decide WHICH samples and cells there are, and the kernel reproduces them in
float32.  Everything downstream is float64 torch: trilinear weights, density sum, activation, alpha, transmittance, w_i = T_i alpha_i,
the normalised intervals, and

    l = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i

as the O(S^2) DOUBLE SUM (not the scan form the kernel uses); the density gradient is autograd through all of it."""
import numpy as np
import torch

from tests import node_weights_model as nm

RELU_BAND = 1e-5  # |pre| < RELU_BAND * rho: float32 and float64 may decide the ReLU differently


def intervals(z, near, far):
    """float64 (m [N,S], d [N,S]) of float32 sample parameters z [N,S]: s = (z - near) / (far - near) with the float32 bounds;
    sample i stands for [s_i, s_{i+1}], the last one for the point s_{S-1}"""
    near, far = float(np.float32(near)), float(np.float32(far))
    s = (z.double() - near) / (far - near)
    m = torch.cat([0.5 * (s[:, :-1] + s[:, 1:]), s[:, -1:]], dim=-1)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], dim=-1)
    return m, d


def double_sum(w, m, d, drop_width=False):
    """l [N] by the O(S^2) double sum, rays in blocks (the [n, S, S] table stays small)"""
    n, S = w.shape
    out = []
    block = max(1, (1 << 22) // (S * S))
    for lo in range(0, n, block):
        ww, mm = w[lo : lo + block], m[lo : lo + block]
        pair = (ww[:, :, None] * ww[:, None, :] * (mm[:, :, None] - mm[:, None, :]).abs()).sum((-1, -2))
        out.append(pair if drop_width else pair + (ww * ww * d[lo : lo + block]).sum(-1) / 3.0)
    return torch.cat(out)


def scan_form(w, m, d):
    """The O(S) form in float64 numpy: (l [N], e = dl/dw [N,S]) from the exclusive prefixes A, B and the totals W, WM (sorted m)."""
    w, m, d = (np.asarray(v, dtype=np.float64) for v in (w, m, d))
    wm = w * m
    A = np.cumsum(w, -1) - w
    B = np.cumsum(wm, -1) - wm
    W, WM = w.sum(-1, keepdims=True), wm.sum(-1, keepdims=True)
    ell = (2.0 * w * (m * A - B) + w * w * d / 3.0).sum(-1)
    e = 2.0 * (m * (A - (W - A - w)) - (B - (WM - B - wm))) + (2.0 / 3.0) * w * d
    return ell, e


def weights(D, aabb, rho, mode, pts, inside, deltas):
    """float64 torch, differentiable in D (flat node values, plain order): (w [N,S], interpolated pre-activation [N,S])"""
    n, S = inside.shape
    dims = D.shape
    lin, b, ok = nm.corner_weights(pts.reshape(-1, 3), aabb, dims)
    pre = D.reshape(-1) * float(np.float32(rho))
    if mode == "abs":
        pre = pre.abs()
    b = torch.from_numpy(np.where(ok, b, 0.0))
    interp = (pre[torch.from_numpy(lin)] * b).sum(-1).reshape(n, S)
    if mode == "relu":
        sigma = torch.relu(interp)
    elif mode == "softplus":
        sigma = torch.nn.functional.softplus(interp)
    else:
        sigma = interp
    sigma = torch.where(inside, sigma, torch.zeros_like(sigma))
    alpha = -torch.expm1(-(sigma * deltas.double()))
    trans = torch.cumprod(torch.cat([torch.ones((n, 1), dtype=torch.float64), 1.0 - alpha], dim=-1), dim=-1)[:, :-1]
    w = torch.where(inside, alpha * trans, torch.zeros_like(alpha))
    return w, interp


def model(densities, aabb, rho, mode, origins, directions, near, far, num_samples, optimized_sampling=False, t_rand=None, grad_loss=None,
          drop_width=False, point_mid=False, want_grad=True):
    """The whole term for one ray batch.  Returns a dict: ``loss`` [N] float64, ``grad`` [X,Y,Z] float64 = d sum_r grad_loss_r l_r / d D
    (None without ``want_grad``), ``spread`` [N] = max_ij |m_i - m_j|, ``band`` = number of inside samples with |pre| < 1e-5 rho,
    ``w`` [N,S].  ``drop_width`` / ``point_mid``: the two WRONG models (no (1/3) sum w^2 d term; m_i = s_i) the bars must reject."""
    z, pts, inside, deltas = nm.sample_geometry(origins, directions, aabb, near, far, num_samples, optimized_sampling, t_rand)
    dims = tuple(densities.shape[:3])
    D = densities.detach().double().reshape(dims).clone().requires_grad_(want_grad)
    w, interp = weights(D, aabb, rho, mode, pts, inside, deltas)
    m, d = intervals(z, near, far)
    if point_mid:
        nr, fr = float(np.float32(near)), float(np.float32(far))
        m = (z.double() - nr) / (fr - nr)
    ell = double_sum(w, m, d, drop_width)
    grad = None
    if want_grad:
        gl = torch.ones_like(ell) if grad_loss is None else torch.as_tensor(grad_loss).double()
        (grad,) = torch.autograd.grad((ell * gl).sum(), D)
        grad = grad.numpy()
    band = int((inside & (interp.detach().abs() < RELU_BAND * float(np.float32(rho)))).sum())
    return {"loss": ell.detach().numpy(), "grad": grad, "spread": (m.max(-1).values - m.min(-1).values).numpy(), "band": band,
            "w": w.detach().numpy(), "m": m.numpy(), "d": d.numpy()}


def loss_bar(spread):
    """|l - l64| <= 2e-5 max(1, max_ij |m_i - m_j|): l is quadratic in w with coefficients up to that maximum, and the project's bar
    on sum w is 1e-5"""
    return 2e-5 * np.maximum(1.0, spread)


GRAD_RTOL, GRAD_ATOL = 5e-4, 5e-6  # x max |g64|: the bar of tests/test_hip_parity.py for grid gradients


def grad_within_bar(g, g64):
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    return bool((np.abs(g - g64) <= GRAD_ATOL * np.abs(g64).max() + GRAD_RTOL * np.abs(g64)).all())


# --------------------------------------------------------------------------------------------
# the cases of the kernel comparison (tests/test_hip_distortion.py runs them, tests/test_distortion_model.py checks their conditions)
# --------------------------------------------------------------------------------------------
STORAGES = ["reference", "split", "bricked"]
MODES = ["relu", "softplus", "abs", "identity"]
DIMS = [(2, 2, 2), (3, 4, 5), (9, 8, 17)]
SAMPLES = [1, 2, 7, 64, 65, 130]  # one sample, a pair, a partial chunk, a full chunk, the lane-63 -> lane-0 hand-over, a third chunk
STASH_SAMPLES = 1100  # above the 16 chunks (1024 samples) whose carry the kernel keeps in LDS: chunks 16 and 17 walk forward again
OPTIONS = ["plain", "aabb", "occupancy", "t_rand", "keyed"]
RAY_COUNTS = [1, 5, 67]  # 67: not a multiple of the 4 rays of a workgroup
JITTER_KEY = 0xC0FFEE1234
GRID_SEED = 33
RAY_SIDE = 12  # the rays are picked from the 144 pixel rays of a wide camera: part of them miss the box


def voxel_of(dims):
    return (3.0 / max(dims),) * 3


def rho_of(mode, S):
    if S == STASH_SAMPLES:
        return 0.5  # thin: the weights beyond sample 1024 must matter
    # identity: sigma < 0 in pockets makes the transmittance grow; a small scale keeps the weights O(1)
    return 0.5 if mode == "identity" else 100.0 / 3.0


def kernel_cases():
    """(dims, storage, S, F, mode, option, rays): dims x storage x S in full, the other factors dealt out so that every storage, every
    S and every dims meets each of their values; then one case per storage above the stash capacity."""
    cases = []
    for j, (dims, storage) in enumerate((d, st) for d in DIMS for st in STORAGES):
        for s, S in enumerate(SAMPLES):
            option = OPTIONS[(2 * j + s) % 5]
            if S == 1 and option == "aabb":  # (the one sample would sit ON the box: t = t_enter -- nothing to compare)
                option = "plain"
            cases.append((dims, storage, S, (3, 27)[(j + s // 2 + j // 4) % 2], MODES[(j + s) % 4], option, RAY_COUNTS[(j + s) % 3]))
    for i, storage in enumerate(STORAGES):  # every sample inside the box (AABB sampling), a thin medium
        cases.append(((9, 8, 17), storage, STASH_SAMPLES, (27, 3)[i % 2], MODES[i], "aabb", 5))
    return cases


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


_CACHE = {}


def case_rays(count, S):
    """(origins, directions, near, far): ``count`` of the pixel rays of a wide camera, evenly spread over the frame (up to five: central
    ones and corners); a single-sample ray samples z = near, so near is put inside the volume there"""
    import thr3ed_atom_amd as rf
    from oracle import relu_field_oracle as orc
    from tests.helpers import hotdog_like_camera

    cam = hotdog_like_camera()
    pose = rf.pose_spherical(40.0, -35.0, cam["radius"])
    o, d = orc.cast_rays(RAY_SIDE, RAY_SIDE, RAY_SIDE * 0.9, torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))
    total = RAY_SIDE * RAY_SIDE
    centre = total // 2 + RAY_SIDE // 2
    if count <= 5:  # the central ray, neighbours of it, two corners of the frame (which miss the box)
        pick = [centre, centre + 1, 0, centre - RAY_SIDE, total - 1][:count]
    else:
        pick = [int(round(i * (total - 1) / (count - 1))) for i in range(count)]
    pick = torch.tensor(pick)
    near = 3.9 if S == 1 else cam["near"]
    return o.reshape(-1, 3)[pick].contiguous(), d.reshape(-1, 3)[pick].contiguous(), float(np.float32(near)), cam["far"]


def case_grid(dims, F, mode):
    from tests.helpers import procedural_grid, signed_density_grid

    key = ("grid", dims, F, mode)
    if key not in _CACHE:
        _CACHE[key] = signed_density_grid(dims, F, GRID_SEED) if mode == "identity" else procedural_grid(dims, F, GRID_SEED)
    return _CACHE[key]


def case_grad_loss(count):
    """the upstream gradient per ray of the comparison: a known pattern in [0.5, 1.5)"""
    from tests.helpers import hash_uniform

    return hash_uniform((count,), 91, 0.5, 1.5)


def case_reference(dims, F, mode, S, option, count):
    """(model dict with the gradient weighted by case_grad_loss, jitter table or None) -- computed once per case, never modified"""
    from oracle import relu_field_oracle as orc
    from tests.helpers import hash_uniform

    key = ("ref", dims, F, mode, S, option, count)
    if key not in _CACHE:
        dens, _ = case_grid(dims, F, mode)
        o, d, near, far = case_rays(count, S)
        t_rand = None
        if option == "t_rand":
            t_rand = torch.from_numpy(hash_uniform((count, S), 77, 0.0, 1.0))
        elif option == "keyed":
            t_rand = torch.from_numpy(orc.keyed_jitter(JITTER_KEY, 5, count, S).astype(np.float32))
        ref = model(dens, orc.make_aabb(dims, voxel_of(dims)), rho_of(mode, S), mode, o, d, near, far, S, optimized_sampling=(option == "aabb"),
                    t_rand=t_rand, grad_loss=case_grad_loss(count))
        _CACHE[key] = (ref, t_rand)
    return _CACHE[key]


# --------------------------------------------------------------------------------------------
# float32 restatement of the kernel's two passes (numpy; sequential scans where the kernel's are wave-parallel)
# --------------------------------------------------------------------------------------------
def emulate_float32(densities, aabb, rho, mode, origins, directions, near, far, num_samples, optimized_sampling=False, t_rand=None, grad_loss=None):
    """(l [N] float32, gradient [X,Y,Z] float64 sum of float32 contributions): pass 1 near to far with running prefixes A, B and the
    running transmittance, pass 2 far to near with a running suffix sum -- every product and sum rounded to float32 as in the
    kernel; the trilinear weights are the float64 ones rounded once."""
    f = np.float32
    z, pts, inside, deltas = nm.sample_geometry(origins, directions, aabb, near, far, num_samples, optimized_sampling, t_rand)
    n, S = inside.shape
    dims = tuple(densities.shape[:3])
    lin, b, ok = nm.corner_weights(pts.reshape(-1, 3), aabb, dims)
    b32 = np.where(ok, b, 0.0).astype(f).reshape(n, S, 8)
    lin = lin.reshape(n, S, 8)
    raw = densities.numpy().reshape(-1).astype(f)
    pre_nodes = raw * f(rho)
    if mode == "abs":
        pre_nodes = np.abs(pre_nodes)
    acc = np.zeros((n, S), dtype=f)
    for k in range(8):
        acc = (acc + pre_nodes[lin[..., k]] * b32[..., k]).astype(f)
    ins = inside.numpy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if mode == "relu":
            sigma = np.maximum(acc, f(0))
        elif mode == "softplus":
            sigma = np.where(acc > 20, acc, np.log1p(np.exp(np.minimum(acc, f(20))))).astype(f)
        else:
            sigma = acc
        sigma = np.where(ins, sigma, f(0)).astype(f)
        delta = deltas.numpy().astype(f)
        E = np.exp(-(sigma * delta).astype(f)).astype(f)
        alpha = (f(1) - E).astype(f)
        zz = z.numpy().astype(f)
        inv = f(1) / (f(far) - f(near))
        s = ((zz - f(near)) * inv).astype(f)
        m = np.concatenate([(f(0.5) * (s[:, :-1] + s[:, 1:])).astype(f), s[:, -1:]], -1)
        d = np.concatenate([(s[:, 1:] - s[:, :-1]).astype(f), np.zeros((n, 1), dtype=f)], -1)
        T = np.ones(n, dtype=f)
        A, B, ell = np.zeros(n, dtype=f), np.zeros(n, dtype=f), np.zeros(n, dtype=f)
        w, Tn, As, Bs = (np.zeros((n, S), dtype=f) for _ in range(4))
        for i in range(S):  # pass 1
            w[:, i] = np.where(ins[:, i], alpha[:, i] * T, f(0))
            Tn[:, i] = T * E[:, i]
            As[:, i], Bs[:, i] = A, B
            ell = (ell + (f(2) * w[:, i] * (m[:, i] * A - B) + f(1.0 / 3.0) * (w[:, i] * w[:, i]) * d[:, i])).astype(f)
            A, B, T = (A + w[:, i]).astype(f), (B + w[:, i] * m[:, i]).astype(f), Tn[:, i]
        W, WM = A, B
        gl = np.ones(n, dtype=f) if grad_loss is None else np.asarray(grad_loss, dtype=f)
        suffix = np.zeros(n, dtype=f)
        grad = np.zeros(int(np.prod(dims)))
        for i in range(S - 1, -1, -1):  # pass 2
            wm = w[:, i] * m[:, i]
            e = (f(2) * (m[:, i] * (As[:, i] - ((W - As[:, i]) - w[:, i])) - (Bs[:, i] - ((WM - Bs[:, i]) - wm))) + f(2.0 / 3.0) * (w[:, i] * d[:, i])).astype(f)
            g_sigma = (delta[:, i] * (Tn[:, i] * e - suffix)).astype(f)
            suffix = (suffix + w[:, i] * e).astype(f)
            if mode == "relu":
                g_pre = np.where(sigma[:, i] > 0, g_sigma, f(0))
            elif mode == "softplus":
                g_pre = (g_sigma * -np.expm1(-sigma[:, i].astype(np.float64))).astype(f)
            else:
                g_pre = g_sigma
            g_pre = np.where(ins[:, i], g_pre * gl, f(0)).astype(f)
            for k in range(8):
                gv = ((b32[:, i, k] * g_pre) * f(rho)).astype(f)
                if mode == "abs":
                    gv = gv * np.sign(raw[lin[:, i, k]])
                np.add.at(grad, lin[:, i, k], np.where(np.isfinite(gv), gv, 0.0).astype(np.float64))
    return ell, grad.reshape(dims)
