"""The float64 model of SSIM (include/relu_field.h: rf_ssim_forward / rf_ssim_backward), its rounding bound, two float32 restatements
and the test images.  Everything here runs on the CPU.

Contract: Wang et al. 2004 per colour channel, data range 1, Gaussian 11 x 11 window of sigma 1.5 normalised to sum 1, C1 = 0.01^2,
C2 = 0.03^2, variances NOT clamped, S = (A1 A2) / (B1 B2); "valid" counts the windows inside the image (map [H - 10, W - 10, C]),
"same" zero-pads the image by 5 (map [H, W, C]); the result is the mean of the map.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import hash_uniform

WINDOW, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
U = 2.0 ** -24  # unit roundoff of float32

# kappa of the bound: the number of roundings on the longest path of one filtered moment in the kernel.  A second moment is
# sum_r g_r (sum_c g_c fl(x y)): 1 rounding of the product, 11 of the row chain acc = fmaf(g_k, v_k, acc), 11 of the column chain,
# and the two float32 weights of a tap carry one rounding each: 1 + 11 + 11 + 2 = 25.  One more covers the roundings the propagated
# formulas do not list (mu_x^2, the subtraction G*x^2 - mu_x^2, the sums of A and B): 26.  
KAPPA = 26

# (padding, H, W) of the issue; the kernel's tile is 16 map rows x 32 map columns, so edge - 1, edge, edge + 1 on each axis follow
TILE_H, TILE_W = 16, 32
VALID_SHAPES = [(11, 11), (11, 40), (12, 27), (26, 26), (27, 43), (37, 50)] + [(TILE_H + 10 + d, 13) for d in (-1, 0, 1)] + [(13, TILE_W + 10 + d) for d in (-1, 0, 1)]
SAME_SHAPES = [(1, 1), (5, 7), (16, 16), (17, 33), (37, 50)] + [(TILE_H + d, 3) for d in (-1, 0, 1)] + [(3, TILE_W + d) for d in (-1, 0, 1)]
CASES = [("valid", h, w) for h, w in VALID_SHAPES] + [("same", h, w) for h, w in SAME_SHAPES]
KINDS = ("noise", "smooth", "equal", "flat")


def case_id(case) -> str:
    return f"{case[0]}-{case[1]}x{case[2]}"


def gaussian_window(sigma: float = SIGMA) -> torch.Tensor:
    k = torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2
    g = torch.exp(-(k * k) / (2.0 * sigma * sigma))
    return g / g.sum()


def images(kind: str, H: int, W: int, C: int, seed: int = 7):
    """(image, target): float32 [H, W, C] tensors in [0, 1]"""
    shape = (H, W, C)
    noise = hash_uniform(shape, seed, 0.0, 1.0)
    if kind == "noise":
        x, y = noise, hash_uniform(shape, seed + 1, 0.0, 1.0)
    elif kind == "smooth":
        r, c, ch = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        x = (0.5 + 0.45 * np.sin(0.37 * r + 0.9 * ch) * np.cos(0.23 * c)).astype(np.float32)
        y = np.clip(x + np.float32(0.05) * hash_uniform(shape, seed + 2, -1.0, 1.0), 0.0, 1.0).astype(np.float32)
    elif kind == "equal":
        x, y = noise, noise.copy()
    elif kind == "flat":
        x = np.full(shape, 0.7, dtype=np.float32)
        y = x.copy()
        y[H // 2, W // 2, :] = np.float32(0.69)
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y))


def _filter(v: torch.Tensor, g: torch.Tensor, padding: str) -> torch.Tensor:
    """G*v of a [H, W, C] tensor with the 11 x 11 window g (x) g, as ONE 121-term convolution in v's dtype"""
    w = (g[:, None] * g[None, :]).to(v.dtype)[None, None]
    out = F.conv2d(v.permute(2, 0, 1)[:, None], w, padding=WINDOW // 2 if padding == "same" else 0)
    return out[:, 0].permute(1, 2, 0)


def _map_from_moments(mx, my, xx, yy, xy, k1=K1, k2=K2):
    c1, c2 = k1 * k1, k2 * k2
    sxx, syy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    a1, a2 = 2.0 * mx * my + c1, 2.0 * sxy + c2
    b1, b2 = mx * mx + my * my + c1, sxx + syy + c2
    return (a1 * a2) / (b1 * b2)


def check_shape(H: int, W: int, padding: str) -> None:
    if padding not in ("valid", "same"):
        raise ValueError(padding)
    if padding == "valid" and (H < WINDOW or W < WINDOW):
        raise ValueError("valid needs at least 11 x 11")


def ssim_map(x: torch.Tensor, y: torch.Tensor, padding: str = "valid", sigma: float = SIGMA, k2: float = K2, dtype=torch.float64) -> torch.Tensor:
    """the map [Hm, Wm, C]: float64 is the model; dtype=float32 is the F.conv2d restatement a user would write today"""
    check_shape(x.shape[0], x.shape[1], padding)
    x, y = x.to(dtype), y.to(dtype)
    g = gaussian_window(sigma)
    f = lambda v: _filter(v, g, padding)  # noqa: E731
    return _map_from_moments(f(x), f(y), f(x * x), f(y * y), f(x * y), K1, k2)


def ssim_mean(x, y, padding="valid", dtype=torch.float64) -> torch.Tensor:
    return ssim_map(x, y, padding, dtype=dtype).mean()


def dssim_grad(x: torch.Tensor, y: torch.Tensor, padding: str, dtype=torch.float64) -> torch.Tensor:
    """gradient of 3 * (1 - ssim(x, y)) with respect to x by autograd in `dtype`"""
    leaf = x.detach().to(dtype).clone().requires_grad_(True)
    (3.0 * (1.0 - ssim_mean(leaf, y.detach(), padding, dtype=dtype))).backward()
    return leaf.grad


def rounding_bound(x: torch.Tensor, y: torch.Tensor, padding: str = "valid", kappa: float = KAPPA) -> torch.Tensor:
    """per-pixel bound on |S32 - S64| of a float32 evaluation whose filtered moments carry kappa roundings: e(Q) = kappa u G*|v|,
    propagated through S to first order; finite everywhere because C2 > 0"""
    x, y = x.double(), y.double()
    g = gaussian_window()
    f = lambda v: _filter(v, g, padding)  # noqa: E731
    mx, my, xx, yy, xy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    ax, ay, axy = f(x.abs()), f(y.abs()), f((x * y).abs())
    c1, c2 = K1 * K1, K2 * K2
    a1, a2 = 2.0 * mx * my + c1, 2.0 * (xy - mx * my) + c2
    b1, b2 = mx * mx + my * my + c1, (xx - mx * mx) + (yy - my * my) + c2
    s = (a1 * a2) / (b1 * b2)
    ku = kappa * U
    e_a1 = 4.0 * ku * ax * ay + U * a1.abs()
    e_b1 = 2.0 * ku * (ax * ax + ay * ay)
    e_a2 = 2.0 * ku * (axy + 2.0 * ax * ay)
    e_b2 = ku * (xx + yy + 2.0 * ax * ax + 2.0 * ay * ay)
    return (a2.abs() * e_a1 + a1.abs() * e_a2) / (b1 * b2) + s.abs() * (e_b1 / b1 + e_b2 / b2) + 4.0 * U


# ---- the kernel's own arithmetic in numpy float32 ------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)  # (double rounding: below 2^-29 relative)


def _chain(v: np.ndarray, g32: np.ndarray, axis: int) -> np.ndarray:
    """acc = fmaf(g_k, v[.. + k ..], acc), k = 0 .. 10 along `axis` (valid extent)"""
    n = v.shape[axis] - WINDOW + 1
    acc = np.zeros_like(np.take(v, range(n), axis=axis))
    for k in range(WINDOW):
        acc = _fma32(np.float32(g32[k]) * np.ones_like(acc), np.take(v, range(k, k + n), axis=axis), acc)
    return acc


def emulate_float32(x: torch.Tensor, y: torch.Tensor, padding: str = "valid"):
    """(map, gradient of the mean with respect to x) as the kernels compute them: separable fmaf chains, rows first, the
    derivative maps in float32, the gather adjoint.  Bit-faithful up to the double rounding of the emulated fma."""
    check_shape(x.shape[0], x.shape[1], padding)
    g32 = gaussian_window().numpy().astype(np.float32)
    pad = WINDOW // 2 if padding == "same" else 0
    xn, yn = x.numpy().astype(np.float32), y.numpy().astype(np.float32)
    xp, yp = (np.pad(v, ((pad, pad), (pad, pad), (0, 0))) for v in (xn, yn))
    f = lambda v: _chain(_chain(v, g32, 1), g32, 0)  # noqa: E731
    mx, my, xx, yy, xy = f(xp), f(yp), f(xp * xp), f(yp * yp), f(xp * yp)
    one = np.float32
    mxmy, mx2, my2 = mx * my, mx * mx, my * my
    sxx, syy, sxy = xx - mx2, yy - my2, xy - mxmy
    a1, a2 = one(2) * mxmy + one(1e-4), one(2) * sxy + one(9e-4)
    b1, b2 = mx2 + my2 + one(1e-4), sxx + syy + one(9e-4)
    s = (a1 * a2) / (b1 * b2)
    inv = one(1) / (b1 * b2)
    d_sxx, d_sxy = -s / b2, one(2) * (a1 * inv)
    d_mu = (one(2) * inv) * (my * (a2 - a1) + (mx * s) * (b1 - b2))
    back = WINDOW - 1 - pad
    g = lambda d: _chain(_chain(np.pad(d, ((back, back), (back, back), (0, 0))), g32, 1), g32, 0)  # noqa: E731
    scale = one(1.0 / s.size)
    grad = scale * (g(d_mu) + one(2) * xn * g(d_sxx) + yn * g(d_sxy))
    return torch.from_numpy(s), torch.from_numpy(grad.astype(np.float32))
