"""CPU: the numpy model of tests/brick_lists.py is the adjoint of the oracle's interpolation; the crafted lists of every grid the GPU
module uses reach every corner they claim to reach (conditions computed from the lists alone, so that an edit of the generator cannot
thin the GPU tests out unnoticed); and the comparison the GPU tests call rejects the kernel faults it is there to catch."""
import numpy as np
import pytest
import torch

from oracle import relu_field_oracle as orc
from tests import brick_lists as bl

GRID_EDGES = [(dims, bl.edges_of(b)) for dims in bl.GRIDS + (bl.RANGE_GRID,) for b in bl.BRICK_SIZES]
IDS = [f"{'x'.join(map(str, d))}-{'x'.join(map(str, e))}" for d, e in GRID_EDGES]


# ---- the model is the oracle's adjoint --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [True, False], ids=["full-width", "base-channel"])
@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_scatter_is_the_adjoint_of_the_oracle_interpolation(K, wide):
    """d/d(grid tensors) of sum_i [g_d interp(densities)(p_i) + sum_c g_c sum_k Y_k(v_i) interp(features[c, k])(p_i)] in float64 autograd,
    built from the oracle's trilinear_recipe and sh_basis, equals scatter() to 1e-12 relative."""
    dims = (5, 6, 7)
    degree = int(round(np.sqrt(K))) - 1
    rng = np.random.default_rng(7 + K)
    n = 400
    pos = rng.uniform(0.0, 1.0, size=(n, 3)) * np.array(dims)
    pos[:40] = np.floor(pos[:40])  # fractional part 0
    pos[40:60, 0] = dims[0] - 1 + rng.uniform(0, 1, 20)  # the upper node is outside the grid
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if wide and K > 1:
        rec = np.zeros((n, 12), np.float32)
        rec[:, 3:7] = rng.uniform(-1, 1, size=(n, 4))
        rec[:, 7:10] = v
    else:
        rec = np.zeros((n, 8), np.float32)
        rec[:, 4:8] = rng.uniform(-1, 1, size=(n, 4))
    rec[:, :3] = pos
    r64 = torch.from_numpy(rec.astype(np.float64))
    # the oracle maps normalised coordinates q to the continuous index i = ((q + 1) * size - 1) / 2: q of a given index
    q = torch.stack([(2.0 * r64[:, a] + 1.0) / dims[a] - 1.0 for a in range(3)], dim=1)
    dens = torch.zeros(dims + (1,), dtype=torch.float64, requires_grad=True)
    feat = torch.zeros(dims + (3 * K,), dtype=torch.float64, requires_grad=True)
    d_i = orc.trilinear_recipe(dens, q)[:, 0]
    f_i = orc.trilinear_recipe(feat, q).reshape(n, 3, K)
    if wide and K > 1:
        Y = orc.sh_basis(degree, r64[:, 7:10])
        total = (r64[:, 3] * d_i).sum() + (r64[:, 4:7] * (f_i * Y[:, None, :]).sum(-1)).sum()
    else:  # base-channel records carry the gradient of the degree-0 coefficient itself
        total = (r64[:, 4] * d_i).sum() + (r64[:, 5:8] * f_i[:, :, 0]).sum()
    total.backward()
    want = bl.from_reference(dens.grad.numpy(), feat.grad.numpy(), K)
    got, bound, count = bl.scatter(rec, wide, dims, K)
    assert np.abs(want).max() > 1.0
    # (the float32 record holds the index; the index -> q -> index round trip of the oracle costs a few float64 roundings of the weights)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    assert count.max() <= n and (bound[count == 0] == 0).all() and (got[count == 0] == 0).all()
    assert (bound[count > 0] > 0).all()


def test_abs_basis_dominates_the_basis():
    v = np.random.default_rng(0).normal(size=(500, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for K in (1, 4, 9, 16):
        Y, Yhat = bl.sh_basis(v, K), bl.sh_basis_abs(v, K)
        assert Y.shape == Yhat.shape == (500, K)
        assert (Yhat >= np.abs(Y) - 1e-15).all()
        assert (Yhat <= 8.0).all()


def test_brick_key_matches_the_header_formula():
    """key = ((((bx * 2 + f_x) * NBY + by) * NBZ + bz) << 2) | f_y | f_z << 1, spelled out per record"""
    for dims, edges in GRID_EDGES[:6]:
        nb = bl.brick_counts(dims, edges)
        lat = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
        keys = bl.brick_key(lat, dims, edges)
        for (x, y, z), key in list(zip(lat.tolist(), keys.tolist()))[::7]:
            b = (x // edges[0], y // edges[1], z // edges[2])
            f = [int(c + 1 < d and (c + 1) // e != c // e) for c, d, e in zip((x, y, z), dims, edges)]
            assert key == ((((b[0] * 2 + f[0]) * nb[1] + b[1]) * nb[2] + b[2]) << 2) | f[1] | (f[2] << 1)
        assert bl.possible_keys(dims, edges)[keys].all() and keys.max() < bl.num_keys(dims, edges)
        brick, flags = bl.key_parts(keys, dims, edges)
        assert np.array_equal(brick, (lat[:, 0] // edges[0] * nb[1] + lat[:, 1] // edges[1]) * nb[2] + lat[:, 2] // edges[2])


# ---- what the crafted lists cover ---------------------------------------------------------------------------------------------------
def _reached(counts, dims, edges):
    """[nbricks] bool from per-class record counts: some record touches a node of the brick"""
    nbricks = bl.num_keys(dims, edges) // 8
    t = bl.touched_bricks(np.flatnonzero(counts > 0), dims, edges)
    out = np.zeros(nbricks, bool)
    out[t[t >= 0]] = True
    return out


@pytest.mark.parametrize("dims,edges", GRID_EDGES, ids=IDS)
def test_crafted_lists_cover_what_they_claim(dims, edges):
    wide, narrow = bl.crafted_records(dims, edges, seed=21)
    nkeys = bl.num_keys(dims, edges)
    nbricks = nkeys // 8
    possible = bl.possible_keys(dims, edges)
    reached = {}
    for kind, rec in (("wide", wide), ("narrow", narrow)):
        lists = bl.sorted_lists(rec, dims, edges, num_lists=8, base=5, seed=3)
        per_list = bl.class_counts(lists)
        assert (per_list[4] == 0).all() and len(set(lists[4][1].tolist())) == 1  # the empty list: all offsets equal
        assert len(set(c.sum() for c in per_list)) == 8  # uneven shares
        for rec_l, off in lists:
            assert off[0] == 5 and np.isnan(rec_l[:5]).all() and np.isnan(rec_l[off[-1]:]).all() and off[-1] < len(rec_l)
            assert np.isfinite(rec_l[off[0]: off[-1]]).all() and (np.diff(off) >= 0).all()
            keys = bl.record_keys(rec_l[off[0]: off[-1]], dims, edges)
            assert (np.diff(keys) >= 0).all() and np.array_equal(np.searchsorted(keys, np.arange(nkeys + 1)) + 5, off)
        counts = per_list.sum(axis=0)
        assert counts.sum() == len(rec) and (counts[~possible] == 0).all()
        reached[kind] = _reached(counts, dims, edges)
        # every (brick, flags) class that can hold a record holds one -- seen from the receiving brick: every brick receives records
        # from every one of its (up to 15) neighbour key ranges -- unless the class touches a brick this kind must not reach at all
        t = bl.touched_bricks(np.arange(nkeys), dims, edges)
        touches_hole = np.any((t >= 0) & ~reached[kind][np.maximum(t, 0)], axis=1)
        assert (counts[possible & ~touches_hole] > 0).all()
        assert (~reached[kind]).sum() <= 2  # ... and those bricks are the two of holes_of(), no more
        brick, _ = bl.key_parts(np.arange(nkeys), dims, edges)
        per_brick = np.bincount(brick, weights=counts, minlength=nbricks)
        assert per_brick.max() > 512  # two or more full batches (256, or 128 in the 4 x 8 x 8 kernels) plus a tail
        cells = np.unique(np.floor(rec[:, :3]).astype(np.int64), axis=0, return_counts=True)[1]
        assert (cells >= 300).sum() >= 2 and cells.max() > 512
        frac0 = (rec[:, :3] == np.floor(rec[:, :3])).sum(axis=1)
        assert all((frac0 == n).sum() >= 3 for n in (1, 2, 3))
        lower = np.floor(rec[:, :3]).astype(np.int64)
        for a in range(3):
            assert (lower[:, a] == dims[a] - 1).any()  # the upper node on this axis is outside the grid
            if dims[a] > 1:
                assert (lower[:, a] == dims[a] - 2).any()  # the last cell of the axis
        assert (lower == np.array(dims) - 1).all(axis=1).any()
        if len(rec[0]) == 12:
            assert np.allclose(np.linalg.norm(rec[:, 7:10], axis=1), 1.0, atol=1e-6)
    holes = bl.holes_of(dims, edges)
    if holes is not None:
        empty, wide_only, narrow_only = holes
        assert not reached["wide"][empty] and not reached["narrow"][empty]
        assert reached["wide"][wide_only] and not reached["narrow"][wide_only]
        assert reached["narrow"][narrow_only] and not reached["wide"][narrow_only]
    else:
        assert reached["wide"].all() and reached["narrow"].all()
    # no element is reached by more than MAX_COUNT records, so (count + 16) * 2^-24 <= 1e-4 everywhere: the bound of an element is at
    # most 1e-4 of its own A, while one missing record of n changes it by about A / n >= 6e-4 A
    for K in (1, 9):
        _, _, count = bl.expected(("wide", "narrow"), bl.base_records(wide) if K == 1 else wide, narrow, dims, K)
        assert count.max() <= bl.MAX_COUNT
    assert (bl.MAX_COUNT + bl.ROUNDINGS) * bl.U32 <= 1e-4


def test_some_grid_of_every_brick_shape_has_holes_and_interior_bricks():
    for b in bl.BRICK_SIZES:
        edges = bl.edges_of(b)
        assert any(bl.holes_of(dims, edges) is not None for dims in bl.GRIDS)
        assert any(min(bl.brick_counts(dims, edges)) >= 2 for dims in bl.GRIDS)  # a brick with all seven lower neighbours
        assert any(max(bl.brick_counts(dims, edges)) == 1 for dims in bl.GRIDS) or edges[0] == 4


def test_long_grid_records():
    rec = bl.long_grid_records(seed=3)
    windows = bl.long_grid_windows(3)
    X, Y, Z = bl.LONG_GRID
    assert ((X + 7) // 8 * 8) * ((Y + 7) // 8 * 8) * ((Z + 7) // 8 * 8) > 2 ** 24
    assert windows[0][0] == 0 and windows[-1][1] == Z and all(a[1] < b[0] for a, b in zip(windows, windows[1:]))
    lower = np.floor(rec[:, 2]).astype(np.int64)
    inside = np.zeros(len(rec), bool)
    for z0, z1 in windows:
        inside |= (lower >= z0) & ((lower + 1 < z1) | (z1 == Z))
    assert inside.all()  # every node a record reaches lies in a window
    assert (lower == 0).any() and (lower == Z - 1).any()
    for w in windows:
        _, _, count = bl.scatter(rec, False, bl.LONG_GRID, 1, window=w)
        assert 512 < count.max() <= bl.MAX_COUNT


# ---- the comparison can fail --------------------------------------------------------------------------------------------------------
DIMS, EDGES, K = (10, 13, 17), (4, 8, 8), 9


@pytest.fixture(scope="module")
def crafted():
    wide, narrow = bl.crafted_records(DIMS, EDGES, seed=21)
    total, bound, count = bl.expected(("wide", "narrow"), wide, narrow, DIMS, K)
    return wide, narrow, total, bound


def _brick_slices(brick):
    b3 = bl.brick_of_id(brick, DIMS, EDGES)
    return tuple(slice(b * e, (b + 1) * e) for b, e in zip(b3, EDGES))


def test_comparison_accepts_a_float32_sum_in_another_order(crafted):
    wide, narrow, total, bound = crafted
    forward = bl.scatter_float32(wide, True, DIMS, K) + bl.scatter_float32(narrow, False, DIMS, K)
    backward = bl.scatter_float32(wide[::-1], True, DIMS, K) + bl.scatter_float32(narrow[::-1], False, DIMS, K)
    assert not np.array_equal(forward, backward)  # the order matters in float32 ...
    assert bl.mismatch(forward, total, bound) <= 1.0 and bl.mismatch(backward, total, bound) <= 1.0  # ... and stays inside the bound
    assert bl.mismatch(total.astype(np.float32), total, bound) <= 1.0


def test_comparison_rejects_a_missing_neighbour_class(crafted):
    wide, narrow, total, bound = crafted
    nb = bl.brick_counts(DIMS, EDGES)
    brick = (1 * nb[1] + 1) * nb[2] + 1  # has all seven lower neighbours
    keys = bl.record_keys(narrow, DIMS, EDGES)
    for source, flags in (((0, 0, 0), (1, 1, 1)), ((1, 0, 1), (0, 1, 0)), ((0, 1, 1), (1, 0, 0))):
        key = ((((source[0] * 2 + flags[0]) * nb[1] + source[1]) * nb[2] + source[2]) << 2) | flags[1] | (flags[2] << 1)
        assert (keys == key).any()
        faulty = total.copy()
        at = _brick_slices(brick)
        faulty[at] = (bl.scatter(wide, True, DIMS, K)[0] + bl.scatter(narrow[keys != key], False, DIMS, K)[0])[at]
        assert not np.array_equal(faulty, total) and np.array_equal(faulty[..., 4:], total[..., 4:])
        assert bl.mismatch(faulty.astype(np.float32), total, bound) > 1.0


def test_comparison_rejects_a_missing_tail_batch(crafted):
    wide, narrow, total, bound = crafted
    (_, _), (cell, n) = bl.hot_cells(DIMS, EDGES)
    for batch in (256, 128):
        in_cell = np.flatnonzero((np.floor(wide[:, :3]).astype(np.int64) == cell).all(axis=1))
        assert len(in_cell) >= n
        keep = np.ones(len(wide), bool)
        keep[in_cell[len(in_cell) - len(in_cell) % batch:]] = False  # the records behind the last full batch
        assert 0 < (~keep).sum() < batch
        faulty = bl.scatter(wide[keep], True, DIMS, K)[0] + bl.scatter(narrow, False, DIMS, K)[0]
        assert bl.mismatch(faulty.astype(np.float32), total, bound) > 1.0
    # a single record of the crowded cell
    keep = np.ones(len(wide), bool)
    keep[in_cell[17]] = False
    faulty = bl.scatter(wide[keep], True, DIMS, K)[0] + bl.scatter(narrow, False, DIMS, K)[0]
    assert bl.mismatch(faulty.astype(np.float32), total, bound) > 1.0


def test_comparison_rejects_a_missing_list(crafted):
    wide, narrow, total, bound = crafted
    owner = bl.deal(len(wide), 8, seed=3)
    assert (owner == 0).sum() > 0  # the smallest share
    faulty = bl.scatter(wide[owner != 0], True, DIMS, K)[0] + bl.scatter(narrow, False, DIMS, K)[0]
    assert bl.mismatch(faulty.astype(np.float32), total, bound) > 1.0


def test_comparison_rejects_swapped_channels_and_a_shift(crafted):
    wide, narrow, total, bound = crafted
    swapped = total.copy()
    swapped[..., [2, 3]] = total[..., [3, 2]]  # degree 0 of g and b
    assert bl.mismatch(swapped.astype(np.float32), total, bound) > 1.0
    swapped = total.copy()
    swapped[..., 4 + 8: 4 + 16], swapped[..., 4 + 16: 4 + 24] = total[..., 4 + 16: 4 + 24], total[..., 4 + 8: 4 + 16]
    assert bl.mismatch(swapped.astype(np.float32), total, bound) > 1.0
    assert bl.mismatch(np.roll(total, 1, axis=2).astype(np.float32), total, bound) > 1.0
    nan = total.astype(np.float32)
    nan[3, 4, 5, 6] = np.nan
    assert bl.mismatch(nan, total, bound) == float("inf")
    stray = total.astype(np.float32)
    empty = bl.holes_of(DIMS, EDGES)[0]
    stray[_brick_slices(empty)] = 1e-30  # an element nothing reaches has bound 0: it must be exactly 0
    assert (bound[_brick_slices(empty)] == 0).all() and bl.mismatch(stray, total, bound) == float("inf")
