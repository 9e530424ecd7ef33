"""rf_resample_grid and rf_node_bounds on the GPU against the float64 model (tests/resample_model.py): exact crops, dyadic
refinement under the float32 evaluation bound, one non-dyadic scale under that bound plus the priced rounding of s, layout
independence bit for bit, the bounds exactly, and every error code."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import resample_model as rm
from tests.helpers import hash_uniform, procedural_grid
from thr3ed_atom_amd import _lib, ops
from thr3ed_atom_amd.voxels import brick_nodes

pytestmark = pytest.mark.gpu

STORAGES = ["reference", "split", "bricked"]
PAIRS = list(itertools.product(STORAGES, STORAGES))
MODES = ["relu", "softplus", "abs", "identity"]
ACTIVATIONS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
               "abs": (torch.abs, torch.nn.Identity()), "identity": (torch.nn.Identity(), torch.nn.Identity())}
SRC_DIMS = [(5, 6, 7), (9, 8, 17)]  # the second crosses an 8-node brick edge on two axes: bricked storage has padding
FEATURES = [3, 12, 27, 48]
CASES = [(d, F) for d in SRC_DIMS for F in FEATURES]
IDS = [f"{'x'.join(map(str, d))}-F{F}" for d, F in CASES]
# |hip - model64| <= 16 * 2^-24 * max|source value|: the weights are exact dyadics that sum to 1; what remains is the <= 2 roundings
# of (wx * wy) * wz and the 8 roundings of the accumulation, each <= 2^-24 of a partial sum bounded by max|v|
EVAL_BOUND = 16 * 2.0**-24


@functools.lru_cache(maxsize=None)
def source(dims, F):
    return procedural_grid(dims, F, 7 + F)


def make_grid(dev, dens, feat, storage, mode="relu", rho=2.0):
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(0.25, 0.25, 0.25), density_preactivation=ACTIVATIONS[mode][0],
                        density_postactivation=ACTIVATIONS[mode][1], expected_density_scale=rho, tunable=False, storage=storage)


def destination(dev, dims, F, storage):
    """a grid of NaN for the launch to overwrite"""
    return make_grid(dev, torch.full((*dims, 1), float("nan")), torch.full((*dims, F), float("nan")), storage)


def run(dev, src_grid, dst_dims, F, storage, scale, offset, fill=0.0):
    dst = destination(dev, dst_dims, F, storage)
    ops.resample_grid_raw(src_grid, dst, scale, offset, fill)
    return dst.densities.detach().cpu(), dst.features.detach().cpu()


def padding_mask(grid, like):
    X, Y, Z = grid.grid_dims
    real = brick_nodes(torch.ones((X, Y, Z, 1), device=like.device))
    return (real == 0).expand_as(like)


@pytest.mark.parametrize("dims,F", CASES, ids=IDS)
def test_crop_is_a_bit_exact_copy(hip_device, dims, F):
    """scale 1, integer offsets: inside torch.equal to the slice, outside exactly (fill, 0) -- every storage pair"""
    dens, feat = source(dims, F)
    inner_off, inner_dims = (1, 2, 3), (3, 4, 4)
    sl = tuple(slice(o, o + n) for o, n in zip(inner_off, inner_dims))
    push = (-2.0, 0.0, 3.0)  # part of the destination outside the source
    out = torch.from_numpy(rm.outside_mask(dims, dims, (1.0,) * 3, push))
    assert bool(out.any()) and not bool(out.all())
    for s_src, s_dst in PAIRS:
        grid = make_grid(hip_device, dens, feat, s_src)
        d, f = run(hip_device, grid, inner_dims, F, s_dst, (1.0,) * 3, inner_off)
        assert torch.equal(d, dens[sl]) and torch.equal(f, feat[sl]), (s_src, s_dst)
        d, f = run(hip_device, grid, dims, F, s_dst, (1.0,) * 3, push, fill=-7.0)
        assert bool((d[out] == -7.0).all()) and bool((f[out] == 0.0).all()), (s_src, s_dst)
        assert torch.equal(d[2:, :, : dims[2] - 3], dens[: dims[0] - 2, :, 3:]) and torch.equal(f[2:, :, : dims[2] - 3], feat[: dims[0] - 2, :, 3:])


DYADIC = [((0.5, 0.5, 0.5), (-0.25, -0.25, -0.25), 2), ((0.25, 0.25, 0.25), (0.25, -0.5, 0.75), 4), ((0.5, 0.25, 0.5), (1.0, 0.5, -0.75), 2)]


@pytest.mark.parametrize("dims,F", CASES, ids=IDS)
def test_dyadic_refinement_within_the_float32_evaluation_bound(hip_device, dims, F):
    """scales 0.5 / 0.25 and offsets on the 0.25 lattice: s and lambda are exact in float32, so the model's float64 sum differs
    from the kernel's by the float32 evaluation alone.  Measured maximum: see DESIGN.md section 15."""
    dens, feat = source(dims, F)
    vmax = max(float(dens.abs().max()), float(feat.abs().max()))
    worst = 0.0
    for scale, offset, factor in DYADIC:
        dst_dims = tuple(min(n * factor, 24) for n in dims)
        d64, f64 = rm.resample(dens.numpy(), feat.numpy(), dst_dims, scale, offset, fill=0.5)
        for s_src, s_dst in PAIRS:
            d, f = run(hip_device, make_grid(hip_device, dens, feat, s_src), dst_dims, F, s_dst, scale, offset, fill=0.5)
            err = max(np.abs(d.numpy() - d64).max(), np.abs(f.numpy() - f64).max())
            worst = max(worst, err)
            assert err <= EVAL_BOUND * vmax, (scale, offset, s_src, s_dst, err)
    print(f"dyadic refinement {dims} F={F}: max |hip - model64| = {worst:.3e} = {worst / (2.0**-24 * vmax):.2f} x 2^-24 max|v| (bound 16)")


def test_a_corrupted_source_node_fails_the_dyadic_comparison(hip_device):
    dims, F = (9, 8, 17), 12
    dens, feat = source(dims, F)
    scale, offset = DYADIC[0][:2]
    dst_dims = tuple(2 * n for n in dims)
    d64, f64 = rm.resample(dens.numpy(), feat.numpy(), dst_dims, scale, offset)
    bad = feat.clone()
    bad[4, 3, 9, 5] += 1e-5  # 10 x the bound on one channel of one node
    _, f = run(hip_device, make_grid(hip_device, dens, bad, "bricked"), dst_dims, F, "split", scale, offset)
    err = np.abs(f.numpy() - f64)
    assert err.max() > EVAL_BOUND * 1.0
    assert (err > EVAL_BOUND * 1.0).sum() <= 64 and (err[..., [c for c in range(F) if c != 5]] <= EVAL_BOUND).all()  # only that node's 4^3 destination neighbourhood, only that channel


def test_a_non_dyadic_scale_within_the_bound_plus_the_priced_rounding_of_s(hip_device):
    """scale 7/5: the kernel's s = fmaf(scale, i, offset) carries one float32 rounding (<= 2^-24 |s| <= 2^-24 n), which moves the value
    by at most |d value / d s| times that; the slope term sum_a |d value / d s_a| comes from the model, and the issue's allowance is
    2^-23 n per unit of slope.  The weights are no longer exact: 1 - lambda adds one rounding per axis weight, still within the 16."""
    dims, F = (9, 8, 17), 12
    dens, feat = source(dims, F)
    scale = (float(np.float32(7 / 5)),) * 3
    offset = (0.0, float(np.float32(-0.2)), float(np.float32(0.3)))
    dst_dims = (8, 6, 12)
    # no destination node within 1e-3 of the source box's faces, where float32 and float64 could disagree about inside / outside
    for a in range(3):
        s = scale[a] * np.arange(dst_dims[a]) + offset[a]
        assert np.abs(s + 0.5).min() > 1e-3 and np.abs(s - (dims[a] - 0.5)).min() > 1e-3
    d64, f64, (sd, sf) = rm.resample(dens.numpy(), feat.numpy(), dst_dims, scale, offset, return_slope=True)
    assert rm.outside_mask(dst_dims, dims, scale, offset).any()  # (x: s = 9.8 > 8.5 at the last node)
    vmax = max(float(dens.abs().max()), float(feat.abs().max()))
    for s_src, s_dst in PAIRS:
        d, f = run(hip_device, make_grid(hip_device, dens, feat, s_src), dst_dims, F, s_dst, scale, offset)
        for got, want, slope in ((d, d64, sd), (f, f64, sf)):
            excess = np.abs(got.numpy() - want) - (EVAL_BOUND * vmax + slope * 2.0**-23 * max(dims))
            assert excess.max() <= 0.0, (s_src, s_dst, excess.max())
    print(f"non-dyadic 7/5: max |hip - model64| = {max(np.abs(d.numpy() - d64).max(), np.abs(f.numpy() - f64).max()):.3e}, largest slope term {max(sd.max(), sf.max()) * 2.0**-23 * max(dims):.3e}")


@pytest.mark.parametrize("dims,F", CASES, ids=IDS)
def test_results_are_bit_identical_across_the_storage_pairs(hip_device, dims, F):
    """destination (1, 1, 1) and a destination larger than the source, a general map; bricked padding stays untouched"""
    dens, feat = source(dims, F)
    for dst_dims, scale, offset in (((1, 1, 1), (1.0, 1.0, 1.0), (2.25, 3.5, 4.125)), (tuple(n + 5 for n in dims), (0.8125, 0.75, 0.9375), (-1.0, -0.3125, 0.4375))):
        first = None
        for s_src, s_dst in PAIRS:
            src = make_grid(hip_device, dens, feat, s_src)
            dst = destination(hip_device, dst_dims, F, s_dst)
            if s_dst == "bricked":
                for t in dst.kernel_tensors():
                    if t is not None:
                        t.data[padding_mask(dst, t)] = 123.0
            ops.resample_grid_raw(src, dst, scale, offset, -1.5)
            got = (dst.densities.detach().cpu(), dst.features.detach().cpu())
            assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())  # every real node was written
            if s_dst == "bricked":
                for t in dst.kernel_tensors():
                    if t is not None:
                        assert bool((t[padding_mask(dst, t)] == 123.0).all())
            if first is None:
                first = got
                d64, f64 = rm.resample(dens.numpy(), feat.numpy(), dst_dims, scale, offset, fill=-1.5)
                assert np.abs(got[0].numpy() - d64).max() <= 1e-6 and np.abs(got[1].numpy() - f64).max() <= 1e-6
            else:
                assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), (s_src, s_dst)


# --------------------------------------------------------------------------------------------
# rf_node_bounds
# --------------------------------------------------------------------------------------------
def bounds_densities(dims, mode, seed):
    """sparse content away from the x = 0 face; no node within 1e-3 of either threshold"""
    dens = torch.from_numpy(hash_uniform((*dims, 1), seed))
    u = torch.from_numpy(hash_uniform((*dims, 1), seed + 1, 0.0, 1.0))
    low = torch.zeros_like(dens) if mode == "abs" else -dens.abs() - 0.1
    dens = torch.where(u > 0.9, torch.where(dens > 0, torch.full_like(dens, 0.4), torch.full_like(dens, 0.1)), low)  # sigma = 0.8 / 0.2 under rho = 2
    dens[0] = low[0]
    return dens * 10.0 if mode == "softplus" else dens


def launch_bounds(dev, grid, threshold, init=None, count0=0):
    bounds = torch.tensor(list(init) if init is not None else [*grid.grid_dims, -1, -1, -1], dtype=torch.int32, device=dev)
    count = torch.tensor([count0], dtype=torch.int64, device=dev)
    ops.node_bounds_raw(grid, threshold, bounds, count)
    return bounds.tolist(), int(count.item())


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [(5, 6, 7), (9, 8, 17), (16, 16, 24)], ids=lambda d: "x".join(map(str, d)))
def test_node_bounds_equal_the_model(hip_device, dims, mode, storage):
    F, rho = 3, 2.0
    dens = bounds_densities(dims, mode, 31)
    feat = source(dims, F)[1] if dims in SRC_DIMS else procedural_grid(dims, F, 3)[1]
    grid = make_grid(hip_device, dens, feat, storage, mode, rho)
    if storage == "bricked":  # NaN in the padding nodes beforehand: the result must not change
        for t in grid.kernel_tensors():
            if t is not None:
                t.data[padding_mask(grid, t)] = float("nan")
    sigma = rm.activated(dens.numpy(), rho, mode)
    for thr in (0.0, 0.5):
        if mode == "softplus" and thr == 0.0:
            # every node passes: the whole grid (the Python entry refuses this meaningless call; the kernel just answers)
            assert launch_bounds(hip_device, grid, 0.0) == ([0, 0, 0, dims[0] - 1, dims[1] - 1, dims[2] - 1], int(np.prod(dims)))
            continue
        assert np.abs(sigma - thr)[sigma != thr].min() > 1e-3  # (float32 and float64 activations agree about every node)
        want = rm.node_bounds(dens.numpy(), rho, mode, thr)
        assert want is not None and want[0][0] > 0 and want[2] < np.prod(dims)
        got, count = launch_bounds(hip_device, grid, thr, count0=1000)
        assert got == [*want[0], *want[1]] and count == 1000 + want[2], (thr, got, want)
        assert rf.content_bounds(grid, thr) == want


@pytest.mark.parametrize("storage", STORAGES)
def test_node_bounds_empty_corner_and_merge(hip_device, storage):
    dims, F = (9, 8, 17), 12
    feat = source(dims, F)[1]
    dens = torch.full((*dims, 1), -1.0)
    grid = make_grid(hip_device, dens, feat, storage)
    # empty: the initial values, whatever they are, are untouched and the count stays
    assert launch_bounds(hip_device, grid, 0.0) == ([9, 8, 17, -1, -1, -1], 0)
    assert launch_bounds(hip_device, grid, 0.0, init=[4, 5, 6, 1, 2, 3], count0=7) == ([4, 5, 6, 1, 2, 3], 7)
    assert rf.content_bounds(grid, 0.0) is None
    # one passing node in a corner (the last node: the last lane of a partial wave)
    for corner in ((8, 7, 16), (0, 0, 0), (8, 0, 16)):
        d = dens.clone()
        d[corner] = 0.25
        g = make_grid(hip_device, d, feat, storage)
        assert launch_bounds(hip_device, g, 0.0) == ([*corner, *corner], 1)
        assert launch_bounds(hip_device, g, 0.5) == ([9, 8, 17, -1, -1, -1], 0)  # sigma = 0.5 is not > 0.5
    # merging across two calls = the model's merge
    a, b = dens.clone(), dens.clone()
    a[2:4, 5, 9:12] = 1.0
    b[6, 1:3, 3] = 1.0
    ga, gb = make_grid(hip_device, a, feat, storage), make_grid(hip_device, b, feat, storage)
    first, n1 = launch_bounds(hip_device, ga, 0.0)
    second, n2 = launch_bounds(hip_device, gb, 0.0, init=first, count0=n1)
    fa, fb = rm.node_bounds(a.numpy(), 2.0, "relu", 0.0), rm.node_bounds(b.numpy(), 2.0, "relu", 0.0)
    assert first == rm.merge_bounds([9, 8, 17, -1, -1, -1], fa) and second == rm.merge_bounds(first, fb) == [2, 1, 3, 6, 5, 11]
    assert n2 == fa[2] + fb[2] == 8


# --------------------------------------------------------------------------------------------
# error codes
# --------------------------------------------------------------------------------------------
def test_every_error_code_is_returned_before_anything_is_written(hip_device):
    lib = _lib.load()
    dims, F = (5, 6, 7), 12
    dens, feat = source(dims, F)
    src, other = make_grid(hip_device, dens, feat, "split"), make_grid(hip_device, *source(dims, 27), "split")
    dst = destination(hip_device, (4, 4, 4), F, "reference")
    stream = torch.cuda.current_stream(hip_device).cuda_stream
    NULL, SHAPE = -1, -2

    def copy(g, **fields):
        c = _lib.RFGrid.from_buffer_copy(g)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def with_dims(g, d):
        c = _lib.RFGrid.from_buffer_copy(g)
        for a in range(3):
            c.dims[a] = d[a]
        return c

    gs, gd = src.to_rf_grid(), dst.to_rf_grid()
    bounds = torch.tensor([5, 6, 7, -1, -1, -1], dtype=torch.int32, device=hip_device)
    count = torch.zeros(1, dtype=torch.int64, device=hip_device)

    def nb(g, thr, b=bounds):
        return lib.rf_node_bounds(None if g is None else C.byref(g), thr, None if b is None else b.data_ptr(), count.data_ptr(), stream)

    assert nb(None, 0.0) == NULL
    assert nb(copy(gs, densities_dev=None), 0.0) == NULL
    assert nb(copy(gs, features_dev=None), 0.0) == NULL
    assert nb(gs, 0.0, None) == NULL
    assert nb(with_dims(gs, (0, 6, 7)), 0.0) == SHAPE
    assert nb(gs, float("nan")) == SHAPE and nb(gs, -0.5) == SHAPE
    torch.cuda.synchronize()
    assert bounds.tolist() == [5, 6, 7, -1, -1, -1] and int(count.item()) == 0

    one, zero = _lib.float3((1.0, 1.0, 1.0)), _lib.float3((0.0, 0.0, 0.0))

    def rs(s, d, scale=one, offset=zero, fill=0.0):
        return lib.rf_resample_grid(None if s is None else C.byref(s), None if d is None else C.byref(d), scale, offset, fill, stream)

    assert rs(None, gd) == NULL and rs(gs, None) == NULL
    assert rs(copy(gs, densities_dev=None), gd) == NULL and rs(gs, copy(gd, features_dev=None)) == NULL
    assert rs(gs, gd, scale=None) == NULL and rs(gs, gd, offset=None) == NULL
    assert rs(with_dims(gs, (5, 0, 7)), gd) == SHAPE and rs(gs, with_dims(gd, (4, 4, -1))) == SHAPE
    assert rs(other.to_rf_grid(), gd) == SHAPE  # F mismatch
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert rs(gs, gd, scale=_lib.float3((1.0, bad, 1.0))) == SHAPE, bad
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert rs(gs, gd, offset=_lib.float3((0.0, 0.0, bad))) == SHAPE, bad
    assert rs(gs, gd, fill=float("nan")) == SHAPE
    # a destination tensor that is a source tensor, in either slot
    assert rs(gs, copy(gd, densities_dev=gs.densities_dev)) == SHAPE and rs(gs, copy(gd, features_dev=gs.features_dev)) == SHAPE
    assert rs(gs, copy(gd, features_dev=gs.densities_dev)) == SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst.densities).all()) and bool(torch.isnan(dst.features).all())  # nothing was launched
    assert rs(gs, gd) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.densities.detach().cpu(), dens[:4, :4, :4])
