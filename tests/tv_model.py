"""Float64 restatement of the total-variation contract of rf_tv_grad (include/relu_field.h), for the tests.

    d_a(n, c) = theta[n + e_a, c] - theta[n, c]   (0 where n + e_a is outside the grid)
    r(n, c)   = sqrt(eps + sum_a d_a(n, c)^2)
    TV_density = (1 / N) sum_n r(n, density),   TV_features = (1 / (N F)) sum_{n, c} r(n, c)

The loss is written with slices and its gradient comes from torch.autograd, both in float64, from the SAME float32 parameters the
kernel reads (in the reference layout: ``voxels.unpack_storage`` of the stored tensors).  Nothing here shares code with the kernel."""
import numpy as np
import torch

ULP = 2.0**-24  # unit round-off of float32
GRAD_BOUND_ULPS = 64.0  # |g - g64| <= 64 * 2^-24 * w per element (six terms of magnitude <= 1, each ~6 roundings, five adds)


def _r(theta: torch.Tensor, eps: float, axes=(0, 1, 2)) -> torch.Tensor:
    """r(n, c) of a [X, Y, Z, C] float64 tensor; ``axes``: the axes whose differences take part (all three in the contract)."""
    sq = torch.zeros_like(theta)
    for a in axes:
        hi = theta.narrow(a, 1, theta.shape[a] - 1) if theta.shape[a] > 1 else theta.narrow(a, 0, 0)
        lo = theta.narrow(a, 0, theta.shape[a] - 1)
        d = hi - lo
        pad = [0, 0] * 4
        pad[2 * (3 - a) + 1] = 1  # F.pad counts dimensions from the last one: one zero plane at the upper face of axis a
        sq = sq + torch.nn.functional.pad(d, pad) ** 2
    return torch.sqrt(eps + sq)


def tv_sums(dens, feat, eps: float = 1e-8, axes=(0, 1, 2)):
    """(sum_n r(n, density), sum_{n, c} r(n, c)) as float64 0-d tensors (differentiable when the inputs are)."""
    return _r(dens, eps, axes).sum(), _r(feat, eps, axes).sum()


def tv_values(dens, feat, eps: float = 1e-8):
    """(TV_density, TV_features) as Python floats, from float32 or float64 reference-layout tensors."""
    d, f = dens.detach().double(), feat.detach().double()
    sd, sf = tv_sums(d, f, eps)
    n = d.shape[0] * d.shape[1] * d.shape[2]
    return float(sd) / n, float(sf) / (n * f.shape[-1])


def tv_loss_and_grad(dens, feat, weight_density: float, weight_features: float, eps: float = 1e-8, axes=(0, 1, 2)):
    """loss = lambda_D TV_density + lambda_F TV_features and its gradient (float64, reference layout) by autograd."""
    d = dens.detach().double().clone().requires_grad_(True)
    f = feat.detach().double().clone().requires_grad_(True)
    n = d.shape[0] * d.shape[1] * d.shape[2]
    sd, sf = tv_sums(d, f, eps, axes)
    loss = weight_density * sd / n + weight_features * sf / (n * f.shape[-1])
    gd, gf = torch.autograd.grad(loss, (d, f))
    return float(loss.detach()), gd, gf


def element_weights(dims, num_features: int, weight_density: float, weight_features: float):
    """(w of a density element, w of a feature element) = (lambda_D / N, lambda_F / (N F))"""
    n = float(np.prod(dims))
    return weight_density / n, weight_features / (n * num_features)


def grad_bound(w: float) -> float:
    return GRAD_BOUND_ULPS * ULP * w


def grad_error(g, g64) -> float:
    """largest |g - g64| over the elements"""
    return float((g.detach().double().cpu() - g64.cpu()).abs().max()) if g64.numel() else 0.0


def grad_within_bound(g, g64, w: float) -> bool:
    """the comparison the GPU tests apply to every gradient tensor"""
    return bool(torch.isfinite(g).all()) and grad_error(g, g64) <= grad_bound(w)


def adam_trajectory(dens, feat, weight_density: float, weight_features: float, eps: float, lr: float, steps: int):
    """``steps`` iterations of torch.optim.Adam(betas=(0.9, 0.999)) in float64 on the model's TV gradient alone.  Returns the final
    (densities, features) and, per tensor, the mask of the elements to COMPARE: those whose |gradient| stayed at or above 100 x the
    kernel's gradient bound at every step (Adam's first steps are sign-like: below that a rounding error of the gradient is not small
    against the gradient itself)."""
    d = dens.detach().double().clone().requires_grad_(True)
    f = feat.detach().double().clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [d, f], "lr": lr}], betas=(0.9, 0.999))
    wd, wf = element_weights(d.shape[:3], f.shape[-1], weight_density, weight_features)
    keep_d, keep_f = torch.ones_like(d, dtype=torch.bool), torch.ones_like(f, dtype=torch.bool)
    for _ in range(steps):
        _, gd, gf = tv_loss_and_grad(d, f, weight_density, weight_features, eps)
        keep_d &= gd.abs() >= 100.0 * grad_bound(wd)
        keep_f &= gf.abs() >= 100.0 * grad_bound(wf)
        d.grad, f.grad = gd, gf
        opt.step()
    return d.detach(), f.detach(), keep_d, keep_f


# the isolated-TV trainer test: dims, seed and weights (tests/test_tv_model.py checks the left-out share of this choice on the CPU)
TRAINER_CASE = {"dims": (16, 16, 24), "num_features": 27, "seed": 4100, "weight_density": 1e-2, "weight_features": 1e-3, "eps": 1e-8, "lr": 0.03, "steps": 3}
