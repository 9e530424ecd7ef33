"""The float64 SSIM model (tests/ssim_model.py) against independent restatements, on the CPU: a literal 121-term window loop, the
closed formula of a single window, the algebraic properties of the contract, the float32 restatements under the rounding bound --
and proof that the comparison can fail: a wrong sigma, a wrong K2, a map shifted by a pixel and the wrong padding each exceed it."""
import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import ssim_model as sm


def literal_map(x: torch.Tensor, y: torch.Tensor, padding: str) -> torch.Tensor:
    """S per window by two nested loops over the 121 taps (float64, plain Python)"""
    pad = 5 if padding == "same" else 0
    x, y = x.double().numpy(), y.double().numpy()
    H, W, C = x.shape
    g = [float(v) for v in sm.gaussian_window()]
    hm, wm = (H, W) if padding == "same" else (H - 10, W - 10)
    out = np.zeros((hm, wm, C))
    for r in range(hm):
        for c in range(wm):
            for ch in range(C):
                mx = my = xx = yy = xy = 0.0
                for i in range(11):
                    for j in range(11):
                        rr, cc = r - pad + i, c - pad + j
                        if 0 <= rr < H and 0 <= cc < W:
                            w, a, b = g[i] * g[j], x[rr, cc, ch], y[rr, cc, ch]
                            mx, my, xx, yy, xy = mx + w * a, my + w * b, xx + w * a * a, yy + w * b * b, xy + w * a * b
                a1, a2 = 2 * mx * my + 1e-4, 2 * (xy - mx * my) + 9e-4
                b1, b2 = mx * mx + my * my + 1e-4, (xx - mx * mx) + (yy - my * my) + 9e-4
                out[r, c, ch] = (a1 * a2) / (b1 * b2)
    return torch.from_numpy(out)


@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("shape", [(11, 11), (13, 12)])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_model_equals_the_literal_window_loop(shape, padding, kind):
    x, y = sm.images(kind, *shape, 2)
    ours, ref = sm.ssim_map(x, y, padding), literal_map(x, y, padding)
    assert ours.shape == ref.shape == ((shape[0], shape[1], 2) if padding == "same" else (shape[0] - 10, shape[1] - 10, 2))
    assert (ours - ref).abs().max().item() <= 1e-12


def test_single_window_against_the_closed_formula():
    x, y = sm.images("noise", 11, 11, 1)
    g = sm.gaussian_window()
    assert abs(g.sum().item() - 1.0) < 1e-15 and torch.equal(g, g.flip(0)) and abs((g[5] / g[4]).item() - np.exp(1.0 / 4.5)) < 1e-12
    w = (g[:, None] * g[None, :]).reshape(-1)
    a, b = x.double().reshape(-1), y.double().reshape(-1)
    mx, my = (w * a).sum(), (w * b).sum()
    vx, vy, cov = (w * a * a).sum() - mx * mx, (w * b * b).sum() - my * my, (w * a * b).sum() - mx * my
    closed = (2 * mx * my + 0.01**2) * (2 * cov + 0.03**2) / ((mx * mx + my * my + 0.01**2) * (vx + vy + 0.03**2))
    m = sm.ssim_map(x, y, "valid")
    assert m.shape == (1, 1, 1) and abs(m.item() - closed.item()) <= 1e-13
    assert abs(sm.ssim_mean(x, y).item() - closed.item()) <= 1e-13


@pytest.mark.parametrize("case", sm.CASES, ids=sm.case_id)
def test_identity_and_symmetry(case):
    padding, H, W = case
    x, y = sm.images("noise", H, W, 3)
    for dtype in (torch.float64, torch.float32):
        assert bool((sm.ssim_map(x, x, padding, dtype=dtype) == 1.0).all())  # the contract's association: numerator == denominator
        assert torch.equal(sm.ssim_map(x, y, padding, dtype=dtype), sm.ssim_map(y, x, padding, dtype=dtype))
    assert bool((sm.emulate_float32(x, x, padding)[0] == 1.0).all())


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (16, 16), (17, 33)])
def test_same_is_valid_on_the_zero_padded_image(shape):
    x, y = sm.images("smooth", *shape, 3)
    pad = lambda v: torch.nn.functional.pad(v, (0, 0, 5, 5, 5, 5))  # noqa: E731
    same, valid = sm.ssim_map(x, y, "same"), sm.ssim_map(pad(x), pad(y), "valid")
    assert same.shape == valid.shape == (*shape, 3)
    assert (same - valid).abs().max().item() <= 1e-14


def test_shapes_the_contract_refuses():
    x, y = sm.images("noise", 10, 30, 3)
    with pytest.raises(ValueError):
        sm.ssim_map(x, y, "valid")
    assert sm.ssim_map(x, y, "same").shape == (10, 30, 3)
    with pytest.raises(ValueError):
        sm.ssim_map(x, y, "reflect")


def _ratio(candidate, x, y, padding):
    return ((candidate.double() - sm.ssim_map(x, y, padding)).abs() / sm.rounding_bound(x, y, padding)).max().item()


@pytest.mark.parametrize("case", sm.CASES, ids=sm.case_id)
def test_float32_restatements_stay_under_the_bound(case):
    """the F.conv2d restatement (121 terms) and the kernel's separable fmaf chains (numpy float32), every pixel of every kind"""
    padding, H, W = case
    for C in (1, 3):
        for kind in sm.KINDS:
            x, y = sm.images(kind, H, W, C)
            bound = sm.rounding_bound(x, y, padding)
            assert bool(torch.isfinite(bound).all()) and bound.min().item() >= 4 * sm.U
            assert _ratio(sm.ssim_map(x, y, padding, dtype=torch.float32), x, y, padding) < 0.5
            assert _ratio(sm.emulate_float32(x, y, padding)[0], x, y, padding) < 0.5


@pytest.mark.parametrize("case", [c for c in sm.CASES if c[1] * c[2] >= 35], ids=sm.case_id)
def test_the_comparison_can_fail(case):
    """what a wrong implementation would get, in float64: each exceeds the bound on the noise images"""
    padding, H, W = case
    x, y = sm.images("noise", H, W, 3)
    assert _ratio(sm.ssim_map(x, y, padding, sigma=1.4), x, y, padding) > 1.0
    assert _ratio(sm.ssim_map(x, y, padding, k2=0.02), x, y, padding) > 1.0
    good = sm.ssim_map(x, y, padding)
    if good.shape[1] > 1:
        assert _ratio(torch.roll(good, 1, dims=1), x, y, padding) > 1.0  # a map shifted by one pixel
    if padding == "same" and H >= 11 and W >= 11:  # "valid" where "same" was asked for: the interior stretched over the frame
        valid = sm.ssim_map(x, y, "valid")
        stretched = torch.nn.functional.pad(valid.permute(2, 0, 1)[None], (5, 5, 5, 5), mode="replicate")[0].permute(1, 2, 0)
        assert _ratio(stretched, x, y, "same") > 1.0


@pytest.mark.parametrize("case", [("valid", 12, 27), ("same", 5, 7), ("same", 17, 33)], ids=sm.case_id)
def test_emulated_adjoint_against_float64_autograd(case):
    """the gather adjoint from the three derivative maps, in the kernel's float32 arithmetic, under the tolerance of the GPU test"""
    padding, H, W = case
    for kind in ("noise", "smooth"):
        x, y = sm.images(kind, H, W, 3)
        g64 = sm.dssim_grad(x, y, padding)
        scale = g64.abs().max().item()
        yardstick = (sm.dssim_grad(x, y, padding, dtype=torch.float32).double() - g64).abs().max().item() / scale
        ours = (-3.0 * sm.emulate_float32(x, y, padding)[1].double() - g64).abs().max().item() / scale
        assert ours <= 4.0 * yardstick + 1e-6, (ours, yardstick)


def test_ssim_has_no_cpu_fallback():
    x, y = sm.images("noise", 12, 12, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rf.ssim(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rf.ssim(x, y, padding="same", return_map=True)
