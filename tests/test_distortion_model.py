"""CPU checks of the distortion-loss model (tests/distortion_model.py), of the conditions the GPU comparison relies on, and of
rf_distortion's argument validation through the library (no GPU: every error is returned before any device access)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import relu_field_oracle as orc
from tests import distortion_model as dm
from tests.helpers import hash_uniform, procedural_grid
from thr3ed_atom_amd import _lib


def small_case(mode="relu", S=9, n=6, dims=(3, 4, 5), seed=5):
    dens, _ = procedural_grid(dims, 3, seed)
    o, d, near, far = dm.case_rays(67, S)
    pick = torch.tensor([14, 19, 20, 24, 25, 0])[:n]  # five rays through the box, one beside it
    return dens, orc.make_aabb(dims, dm.voxel_of(dims)), o[pick], d[pick], near, far


@pytest.mark.parametrize("mode", dm.MODES)
def test_model_gradient_equals_central_differences(mode):
    dens, aabb, o, d, near, far = small_case(mode)
    rho = 0.5 if mode == "identity" else 4.0
    gl = dm.case_grad_loss(o.shape[0])
    ref = dm.model(dens, aabb, rho, mode, o, d, near, far, 9, grad_loss=gl)
    assert np.abs(ref["grad"]).max() > 1e-3
    total = lambda D: float((dm.model(D, aabb, rho, mode, o, d, near, far, 9, want_grad=False)["loss"] * gl).sum())  # noqa: E731
    flat = dens.double().reshape(-1)
    h = 1e-6
    for node in np.argsort(-np.abs(ref["grad"]).reshape(-1))[:12]:
        hi, lo = flat.clone(), flat.clone()
        hi[node] += h
        lo[node] -= h
        fd = (total(hi.reshape(dens.shape)) - total(lo.reshape(dens.shape))) / (2 * h)
        assert abs(fd - ref["grad"].reshape(-1)[node]) <= 1e-6 * max(1.0, abs(fd)), (node, fd, ref["grad"].reshape(-1)[node])


def test_scan_form_equals_the_double_sum():
    w = hash_uniform((7, 40), 3, 0.0, 0.2).astype(np.float64)
    s = np.sort(hash_uniform((7, 41), 4, 0.0, 1.0).astype(np.float64), -1)
    m, d = 0.5 * (s[:, :-1] + s[:, 1:]), s[:, 1:] - s[:, :-1]
    wt = torch.from_numpy(w).requires_grad_(True)
    ell = dm.double_sum(wt, torch.from_numpy(m), torch.from_numpy(d))
    (e64,) = torch.autograd.grad(ell.sum(), wt)
    ell_scan, e_scan = dm.scan_form(w, m, d)
    np.testing.assert_allclose(ell_scan, ell.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(e_scan, e64.numpy(), rtol=1e-11, atol=1e-14)


def test_two_separated_slabs_cost_more_than_one_of_the_same_weight():
    S = 32
    s = np.linspace(0.0, 1.0, S + 1)
    m, d = (0.5 * (s[:-1] + s[1:]))[None], (s[1:] - s[:-1])[None]
    one, two = np.zeros((1, S)), np.zeros((1, S))
    one[0, 10:14] = 0.2
    two[0, 4:6] = 0.2
    two[0, 24:26] = 0.2
    assert one.sum() == two.sum()
    f = lambda w: float(dm.double_sum(torch.from_numpy(w), torch.from_numpy(m), torch.from_numpy(d))[0])  # noqa: E731
    assert f(two) > 4 * f(one) > 0


def test_case_table_meets_every_value_of_every_factor():
    cases = [c for c in dm.kernel_cases() if c[2] != dm.STASH_SAMPLES]
    assert len(cases) == len(dm.DIMS) * len(dm.STORAGES) * len(dm.SAMPLES)
    for col, values in ((3, (3, 27)), (4, dm.MODES), (5, dm.OPTIONS), (6, dm.RAY_COUNTS)):
        for storage in dm.STORAGES:
            assert {c[col] for c in cases if c[1] == storage} == set(values), (col, storage)
        for S in dm.SAMPLES:
            assert {c[col] for c in cases if c[2] == S} | ({"aabb"} if S == 1 else set()) >= set(values), (col, S)
        for dims in dm.DIMS:
            assert {c[col] for c in cases if c[0] == dims} == set(values), (col, dims)
    assert {c[1] for c in dm.kernel_cases() if c[2] == dm.STASH_SAMPLES} == set(dm.STORAGES)


def test_every_gpu_case_is_finite_nontrivial_and_has_no_sample_in_the_relu_band():
    """A condition on the chosen seeds and grids, not a measurement: no element is left out of any comparison."""
    seen, live_pairs = set(), 0
    for dims, storage, S, F, mode, option, count in dm.kernel_cases():
        key = (dims, F, mode, S, option, count)
        if key in seen:
            continue
        seen.add(key)
        ref, _ = dm.case_reference(*key)
        assert np.isfinite(ref["loss"]).all() and np.isfinite(ref["grad"]).all(), key
        assert ref["band"] == 0, (key, ref["band"])
        assert np.abs(ref["w"]).max() < 64.0
        if S == 1:
            assert (ref["loss"] == 0).all() and (ref["grad"] == 0).all()
        elif S == 2:  # (without jitter the two samples are z = near and z = far, both outside the box: exact zeros to reproduce)
            live_pairs += bool(np.abs(ref["loss"]).max() > 1e-3 and np.abs(ref["grad"]).max() > 1e-3)
        else:
            assert np.abs(ref["loss"]).max() > 1e-6 and np.abs(ref["grad"]).max() > 1e-6, (key, ref["loss"].max())
            if count >= 5:
                assert (np.abs(ref["w"]).sum(-1) == 0).any() and (np.abs(ref["w"]).sum(-1) > 0).any(), "the batch needs rays that miss and rays that hit"
        if S == dm.STASH_SAMPLES:  # the samples whose chunks lie beyond the stash carry weight: 250 x the bar on l
            assert np.abs(ref["w"][:, 1024:]).sum(-1).max() > 5e-3, key
    assert live_pairs >= 3


@pytest.mark.parametrize("wrong", ["drop_width", "point_mid"])
def test_the_bars_reject_the_two_wrong_models(wrong):
    """A model without the (1/3) sum w^2 d term, and one with m_i = s_i, miss the GPU bars on cases of the table: the comparison
    tells them from the contract."""
    rejected_loss = rejected_grad = 0
    # (on evenly spaced samples m_i = s_i only shifts every mid-point but the last by the same half interval: it takes jitter to tell)
    table = [c for c in dm.kernel_cases() if c[5] in ("t_rand", "keyed") and c[2] in (7, 64, 65) and c[0] != (2, 2, 2)][:3]
    assert len(table) == 3
    for dims, _, S, F, mode, option, count in table:
        dens, _ = dm.case_grid(dims, F, mode)
        o, d, near, far = dm.case_rays(count, S)
        aabb = orc.make_aabb(dims, dm.voxel_of(dims))
        gl = dm.case_grad_loss(count)
        right, t_rand = dm.case_reference(dims, F, mode, S, option, count)
        bad = dm.model(dens, aabb, dm.rho_of(mode, S), mode, o, d, near, far, S, t_rand=t_rand, grad_loss=gl, **{wrong: True})
        rejected_loss += bool((np.abs(bad["loss"] - right["loss"]) > dm.loss_bar(right["spread"])).any())
        rejected_grad += not dm.grad_within_bar(bad["grad"], right["grad"])
    assert rejected_loss == 3 and rejected_grad == 3


# --------------------------------------------------------------------------------------------
# the library, without a GPU
# --------------------------------------------------------------------------------------------
def test_the_symbol_is_exported():
    assert "rf_distortion" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.rf_distortion.restype is C.c_int and lib.rf_abi_version() == 4


def _grid(dims=(3, 4, 5), F=3, layout="reference"):
    g = _lib.RFGrid()
    g.densities_dev, g.features_dev = 0x1000, 0x2000  # never dereferenced: every call below returns before any device access
    g.dims = (C.c_int32 * 3)(*dims)
    g.num_features, g.density_stride, g.feature_stride = F, (1 if layout == "reference" else 4), F
    g.aabb_min, g.aabb_max = _lib.float3((-1, -1, -1)), _lib.float3((1, 1, 1))
    g.norm_scale, g.norm_bias = _lib.float3((1, 1, 1)), _lib.float3((0, 0, 0))
    g.density_scale, g.density_mode, g.layout = 1.0, 0, _lib.LAYOUTS[layout]
    return g


def _rays(n=4, S=8, near=1.0, far=5.0):
    r = _lib.RFRayBatch()
    r.origins_dev, r.directions_dev, r.t_vals_dev = 0x3000, 0x4000, 0x5000
    r.num_rays, r.num_samples, r.near, r.far = n, S, near, far
    return r


def test_argument_validation_without_a_gpu():
    lib = _lib.load()
    NULL, BAD = -1, -2
    call = lambda g, r, flags=0, scale=1.0, gl=None, loss=0x6000, grad=0x7000: lib.rf_distortion(  # noqa: E731
        None if g is None else C.byref(g), None if r is None else C.byref(r), flags, scale, gl, loss, grad, None)
    assert lib.rf_error_string(NULL) == b"null pointer" and lib.rf_error_string(BAD).startswith(b"bad shape")
    assert call(None, _rays()) == NULL and call(_grid(), None) == NULL
    g = _grid()
    g.densities_dev = None
    assert call(g, _rays()) == NULL
    r = _rays()
    r.t_vals_dev = None
    assert call(_grid(), r) == NULL
    r = _rays()
    r.directions_dev = None
    assert call(_grid(), r) == NULL
    assert call(_grid(dims=(0, 4, 5)), _rays()) == BAD and call(_grid(dims=(3, 4, 2047)), _rays()) == BAD
    assert call(_grid(), _rays(S=0)) == BAD and call(_grid(), _rays(n=-1)) == BAD
    assert call(_grid(), _rays(near=2.0, far=2.0)) == BAD
    for bad in (float("nan"), float("inf")):
        assert call(_grid(), _rays(near=bad)) == BAD and call(_grid(), _rays(far=bad)) == BAD and call(_grid(), _rays(), scale=bad) == BAD
    assert call(_grid(), _rays(), grad=0x1000) == BAD  # the gradient pointer IS the density tensor
    assert call(_grid(), _rays(), flags=_lib.FLAG_OCCUPANCY_SKIP) == NULL  # no mask
    # nothing to do: RF_OK without a launch (the pointers are not device memory -- a launch would fault)
    assert call(_grid(), _rays(), loss=None, grad=None) == 0
    assert call(_grid(), _rays(), scale=0.0, loss=None) == 0
    assert call(_grid(), _rays(n=0)) == 0
    for layout in ("split", "bricked"):
        assert call(_grid(layout=layout), _rays(n=0)) == 0


def test_float32_restatement_of_the_two_passes_meets_the_gpu_bars():
    """The kernel's arithmetic -- prefixes near to far, e_i from prefixes and totals, a running suffix far to near, the density lane --
    restated in float32 numpy meets the bars of the GPU comparison on every case of the table (no GPU needed)."""
    seen = set()
    for dims, storage, S, F, mode, option, count in dm.kernel_cases():
        key = (dims, F, mode, S, option, count)
        if key in seen:
            continue
        seen.add(key)
        ref, t_rand = dm.case_reference(*key)
        dens, _ = dm.case_grid(dims, F, mode)
        o, d, near, far = dm.case_rays(count, S)
        ell, grad = dm.emulate_float32(dens, orc.make_aabb(dims, dm.voxel_of(dims)), dm.rho_of(mode, S), mode, o, d, near, far, S,
                                       optimized_sampling=option == "aabb", t_rand=t_rand, grad_loss=dm.case_grad_loss(count))
        assert (np.abs(ell.astype(np.float64) - ref["loss"]) <= dm.loss_bar(ref["spread"])).all(), key
        assert dm.grad_within_bar(grad, ref["grad"]), key
