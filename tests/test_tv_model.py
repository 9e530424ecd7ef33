"""CPU checks of the total-variation tests' own yardstick (tests/tv_model.py) and of rf_tv_grad's argument validation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from thr3ed_atom_amd import _lib
from tests import tv_model
from tests.helpers import hash_uniform, procedural_grid


def test_model_gradient_equals_central_finite_differences():
    dims, F, wd, wf, eps = (3, 4, 5), 3, 0.7, 0.3, 1e-8
    dens, feat = procedural_grid(dims, F, 77)
    _, gd, gf = tv_model.tv_loss_and_grad(dens, feat, wd, wf, eps)
    n = float(np.prod(dims))

    def loss(d, f):
        sd, sf = tv_model.tv_sums(d, f, eps)
        return float(wd * sd / n + wf * sf / (n * F))

    h = 1e-6
    for base, grad, which in ((dens.double(), gd, 0), (feat.double(), gf, 1)):
        flat = base.reshape(-1)
        for i in range(flat.numel()):
            lo, hi = flat.clone(), flat.clone()
            lo[i] -= h
            hi[i] += h
            args = [dens.double(), feat.double()]
            args[which] = hi.reshape(base.shape)
            up = loss(*args)
            args[which] = lo.reshape(base.shape)
            fd = (up - loss(*args)) / (2 * h)
            # central differences of a smooth function (|d| ~ 1 >> sqrt(eps)): O(h^2) truncation + 1e-16 / h rounding
            assert abs(fd - float(grad.reshape(-1)[i])) <= 1e-8, (which, i, fd, float(grad.reshape(-1)[i]))


def test_model_values_of_a_hand_computed_grid():
    # two nodes along z, one channel each: d_z(0) = 3, everything else 0 -> r = (sqrt(eps + 9), sqrt(eps))
    dens = torch.tensor([1.0, 4.0]).reshape(1, 1, 2, 1)
    feat = torch.zeros(1, 1, 2, 3)
    tvd, tvf = tv_model.tv_values(dens, feat, 1e-8)
    assert tvd == pytest.approx((np.sqrt(9 + 1e-8) + 1e-4) / 2, rel=1e-12) and tvf == pytest.approx(1e-4, rel=1e-12)
    _, gd, _ = tv_model.tv_loss_and_grad(dens, feat, 2.0, 0.0, 1e-8)
    np.testing.assert_allclose(gd.reshape(-1).numpy(), [-1.0, 1.0], rtol=1e-8)  # w = 2 / 2 nodes, d / r = 1


def test_comparison_rejects_a_gradient_with_one_axis_dropped():
    """The bound the GPU tests apply can fail: the gradient of a TV that ignores the z differences is far outside it, the float32
    rounding of the right gradient is inside."""
    dims, F, lam = (5, 4, 6), 12, (1e-2, 1e-3)
    dens, feat = procedural_grid(dims, F, 5)
    wd, wf = tv_model.element_weights(dims, F, *lam)
    _, gd, gf = tv_model.tv_loss_and_grad(dens, feat, *lam)
    _, bad_d, bad_f = tv_model.tv_loss_and_grad(dens, feat, *lam, axes=(0, 1))
    assert tv_model.grad_within_bound(gd.float(), gd, wd) and tv_model.grad_within_bound(gf.float(), gf, wf)
    assert not tv_model.grad_within_bound(bad_d.float(), gd, wd)
    assert not tv_model.grad_within_bound(bad_f.float(), gf, wf)
    assert not tv_model.grad_within_bound(torch.full_like(gd, float("nan")).float(), gd, wd)
    assert tv_model.grad_error(bad_d, gd) > 1000 * tv_model.grad_bound(wd)


def test_trainer_case_leaves_out_at_most_one_percent():
    """The isolated-TV trainer test compares the elements whose float64 gradient stays >= 100 x the kernel's gradient bound over its
    three Adam steps: for the dims and seed it uses, the model alone must leave out at most 1 % of either tensor."""
    c = tv_model.TRAINER_CASE
    dens, feat = procedural_grid(c["dims"], c["num_features"], c["seed"])
    _, _, keep_d, keep_f = tv_model.adam_trajectory(dens, feat, c["weight_density"], c["weight_features"], c["eps"], c["lr"], c["steps"])
    for keep in (keep_d, keep_f):
        left_out = 1.0 - float(keep.double().mean())
        print("left out:", left_out)
        assert left_out <= 0.01


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _grid(layout="reference", F=27):
    g = _lib.RFGrid()
    g.densities_dev, g.features_dev = 4096, 8192
    g.dims[0], g.dims[1], g.dims[2] = 4, 5, 6
    g.num_features, g.layout = F, _lib.LAYOUTS[layout]
    g.density_stride, g.feature_stride = (1, F) if layout == "reference" else (4, F - 3)
    if layout != "reference" and F == 3:
        g.features_dev = None
    return g


def test_rf_tv_grad_argument_validation_needs_no_gpu(lib):
    """Every error is a return code before any device access (the pointers below are not device memory)."""
    assert "rf_tv_grad" in _lib.EXPORTED_SYMBOLS
    tv = lib.rf_tv_grad
    gd, gf, inf, nan = 1 << 20, 1 << 21, float("inf"), float("nan")
    assert tv(None, 1.0, 1.0, 1e-8, gd, gf, None, None) == -1  # null grid
    g = _lib.RFGrid()
    assert tv(C.byref(g), 1.0, 1.0, 1e-8, gd, gf, None, None) == -1  # null grid tensors
    g = _grid()
    g.dims[1] = 0
    assert tv(C.byref(g), 1.0, 1.0, 1e-8, gd, gf, None, None) == -2  # bad dims
    g = _grid()
    g.num_features = 5
    assert tv(C.byref(g), 1.0, 1.0, 1e-8, gd, gf, None, None) == -3  # no SH degree
    g = _grid()
    for eps in (0.0, -1e-8, inf, nan):
        assert tv(C.byref(g), 1.0, 1.0, eps, gd, gf, None, None) == -2
    for w in (-1.0, inf, nan):
        assert tv(C.byref(g), w, 1.0, 1e-8, gd, gf, None, None) == -2
        assert tv(C.byref(g), 1.0, w, 1e-8, gd, gf, None, None) == -2
    # a gradient tensor a non-zero weight needs
    assert tv(C.byref(g), 1.0, 0.0, 1e-8, None, gf, None, None) == -1
    assert tv(C.byref(g), 0.0, 1.0, 1e-8, gd, None, None, None) == -1
    for layout in ("split", "bricked"):
        s = _grid(layout)
        assert tv(C.byref(s), 0.0, 1.0, 1e-8, None, gf, None, None) == -1  # the degree-0 coefficients live in the base tensor
        assert tv(C.byref(s), 0.0, 1.0, 1e-8, gd, None, None, None) == -1
    # the gradient must not be written into the parameters
    assert tv(C.byref(g), 1.0, 1.0, 1e-8, g.densities_dev, gf, None, None) == -2
    assert tv(C.byref(g), 1.0, 1.0, 1e-8, gd, g.features_dev, None, None) == -2
    # both weights zero: a no-op, whatever the pointers
    assert tv(C.byref(g), 0.0, 0.0, 1e-8, None, None, None, None) == 0
    assert tv(C.byref(g), 0.0, 0.0, 1e-8, gd, gf, 1 << 22, None) == 0
    # the error of a bad argument wins over the no-op
    assert tv(C.byref(g), 0.0, 0.0, nan, None, None, None, None) == -2
