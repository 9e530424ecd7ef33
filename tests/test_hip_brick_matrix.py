"""GPU: every variant of the brick pass (brick_gather_kernel behind rf_brick_accumulate*) on the crafted lists of tests/brick_lists.py,
against the float64 scatter-add ``sum64`` under the derived bound (count + 16) * 2^-24 * A, and against a float64 Adam step on ``sum64``
with the tolerances of test_hip_brick_narrow.py.  Outputs start from garbage, every pass runs twice (bit-identical, except the split
pass), lists come 1, 2, 3 and 8 per kind with one empty, behind a NaN prefix and in front of a NaN tail; a NaN in an output means a
record outside a key class was read.  What was measured is in docs/brick_pass_errors.md (a record, never a tolerance source); every
comparison prints its figures (``BRICK_ERR ...``) before it asserts.

Instantiation of brick_accumulate_impl's dispatch <K, ADAM, ONE_ROUND, SPLIT, BX, MIRROR>  ->  case that reaches it
  <1|4|9|16, false, true>            test_gradient_tensors[K-8-*]             <1|4|9|16, false, false>      test_gradient_tensors[K-4-*]
  <1|9, false, true, false, 4>       test_gradient_tensors[K-488-*]           (K = 4, 16, 488, full-width lists: refused, asserted)
  <1|9, true, true>                  test_adam[K-8-*], test_adam_ranges[K-8]  <1|9, true, false>            test_adam[K-4-*], test_adam_ranges[K-4],
  <1|9, true, true, false, 4>        test_adam[K-488-*] (no mirror: bricked,                                test_adam_long_grid[K] (brick size 8)
                                     or dims no multiple), test_adam_ranges[K-488]
  <1|9, true, true, false, 4, true>  test_adam[K-488-split] on 16 x 16 x 24   <1|9, true, true, true>       test_adam_split[K-parts]"""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import brick_lists as bl
from thr3ed_atom_amd import ops
from thr3ed_atom_amd.voxels import pack_storage, unpack_split

pytestmark = pytest.mark.gpu

SEED = 21
UNSUPPORTED = "(code -3)"  # RF_ERR_UNSUPPORTED in the message of _lib.check
# rf_brick_accumulate refuses exactly these (K, brick_size) when a full-width list is among the lists (base-channel lists alone run on the
# four base channels whatever the grid's degree); include/relu_field.h lists them
REFUSED_GRADIENT = {(4, ops.BRICK_4X8X8), (16, ops.BRICK_4X8X8)}
LISTS = (1, 2, 3, 8)
LR, B1, B2, EPS, STEP = 0.03, 0.9, 0.999, 1e-8, 3
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "relu_field.h")


@functools.lru_cache(maxsize=None)
def records(dims, brick, K):
    wide, narrow = bl.crafted_records(dims, bl.edges_of(brick), SEED)
    return (bl.base_records(wide) if K == 1 else wide), narrow


@functools.lru_cache(maxsize=None)
def reference(dims, brick, K, kinds):
    wide, narrow = records(dims, brick, K)
    return bl.expected(kinds, wide, narrow, dims, K)


def device_lists(dims, brick, K, kinds, per_kind, base, device, poison=None):
    """the lists of a call, full-width ones first; a degree-0 grid and a call with base-channel lists only have ONE kind (8 lists at most)"""
    wide, narrow = records(dims, brick, K)
    edges = bl.edges_of(brick)
    if K == 1 or kinds == ("narrow",):
        per_kind = min(per_kind, 8 // len(kinds))
    out = []
    if "wide" in kinds:
        out += bl.to_device(bl.sorted_lists(wide, dims, edges, per_kind, base, poison, seed=3), False, device)
    if "narrow" in kinds:
        out += bl.to_device(bl.sorted_lists(narrow, dims, edges, per_kind, base + 2 if base else 0, poison, seed=4), True, device)
    return out


def make_grid(dims, K, storage, device, seed=3):
    rng = np.random.default_rng(seed)
    dens = torch.from_numpy(rng.uniform(-1, 1, size=tuple(dims) + (1,)).astype(np.float32))
    feat = torch.from_numpy(rng.uniform(-1, 1, size=tuple(dims) + (3 * K,)).astype(np.float32))
    return rf.VoxelGrid(dens.to(device), feat.to(device), rf.VoxelSize(0.1, 0.1, 0.1), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=3.0, tunable=True, storage=storage)


def to_storage(values, K, storage, device):
    """float [X, Y, Z, 3K + 1] in channel order -> the two tensors of the storage (padding nodes of bricked storage: zero)"""
    dens, feat = (torch.from_numpy(np.ascontiguousarray(t.astype(np.float32))) for t in bl.to_reference(values, K))
    first, second = (dens, feat) if storage == "reference" else pack_storage(dens, feat, storage)
    return first.to(device), None if second is None else second.to(device)


def channels(grid, first, second, K):
    """the two tensors of the grid's storage -> float32 numpy [X, Y, Z, 3K + 1] in channel order"""
    dens, feat = grid.unpack(first, second)
    return bl.from_reference(dens.detach().cpu().numpy(), feat.detach().cpu().numpy(), K)


def clone(pair):
    return [None if t is None else t.detach().clone() for t in pair]


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def check(variant, got, total, bound):
    """print the figures of a comparison, then assert it: |got - sum64| <= bound on every element, no NaN"""
    worst = bl.mismatch(got, total, bound)
    scale = float(np.abs(total).max())
    rel = float(np.abs(got.astype(np.float64) - total).max()) / scale if np.isfinite(got).all() else float("inf")
    print(f"BRICK_ERR variant={variant} ratio={worst:.4f} rel={rel:.3e} scale={scale:.3f}")
    assert scale > 1.0
    assert worst <= 1.0, f"{variant}: |hip - sum64| is {worst:.3g} x the bound"


def kinds_name(kinds):
    return "+".join(kinds)


# ---- gradient tensors ---------------------------------------------------------------------------------------------------------------
GRADIENT_CASES = list(itertools.product((1, 4, 9, 16), bl.BRICK_SIZES, ("reference", "split", "bricked"),
                                        (("wide",), ("narrow",), ("wide", "narrow"))))


@pytest.mark.parametrize("index", range(len(GRADIENT_CASES)), ids=[f"{K}-{b}-{s}-{kinds_name(k)}" for K, b, s, k in GRADIENT_CASES])
def test_gradient_tensors(hip_device, index):
    """rf_brick_accumulate, every (K, brick, storage, lists) combination; the grids, list counts and NaN prefixes rotate through the
    combinations so that every grid meets every list count.  Base-channel lists on an SH grid write density + degree 0 only."""
    K, brick, storage, kinds = GRADIENT_CASES[index]
    dims = bl.GRIDS[index % 4]
    per_kind = LISTS[(index // 4 + index // 16) % 4]
    base = (0, 5)[(index // 2) % 2]
    variant = f"grad-K{K}-b{brick}-{storage}-{kinds_name(kinds)}"
    C = 3 * K + 1
    live = C if "wide" in kinds else 4  # channels the pass writes
    grid = make_grid(dims, K, storage, hip_device)
    lists = device_lists(dims, brick, K, kinds, per_kind, base, hip_device)
    rng = np.random.default_rng(100 + index)
    garbage = to_storage(rng.uniform(-3, 3, size=tuple(dims) + (C,)), K, storage, hip_device)
    garbage = [None if t is None else torch.where(t == 0, torch.full_like(t, 7.0), t) for t in garbage]  # (padding nodes too)

    def run(out, accumulate):
        ops.brick_accumulate_raw(grid, brick, lists, out[0], out[1], accumulate=accumulate)
        torch.cuda.synchronize()
        return out

    if (K, brick) in REFUSED_GRADIENT and "wide" in kinds:
        out = clone(garbage)
        with pytest.raises(RuntimeError) as err:
            run(out, False)
        assert UNSUPPORTED in str(err.value)
        assert same_bits(out, garbage)  # refused before anything was launched
        text = open(HEADER).read()
        assert "RF_ERR_UNSUPPORTED combinations of the brick pass" in text and "RF_BRICK_4X8X8 with full-width lists on a grid of SH degree 1 or 3" in text
        return
    total, bound, count = reference(dims, brick, K, kinds)
    first = run(clone(garbage), False)
    got = channels(grid, *first, K)
    before = channels(grid, *garbage, K)
    check(variant, got[..., :live], total[..., :live], bound[..., :live])
    # what the lists do not carry stays bitwise as it was (base-channel lists on an SH grid: every higher-degree element)
    assert np.array_equal(got[..., live:].view(np.uint32), before[..., live:].view(np.uint32))
    assert (count[..., :live] == 0).any() == (bl.holes_of(dims, bl.edges_of(brick)) is not None)  # (elements nothing reaches are written as 0)
    assert same_bits(run(clone(garbage), False), first)  # deterministic
    # accumulate = 1 after an overwrite pass: the flush adds the FINISHED brick sum to the content (brick_flush: o + v), so this is 2 x bit for bit
    twice = channels(grid, *run(clone(first), True), K)
    assert np.array_equal((twice[..., :live]).view(np.uint32), (got[..., :live] + got[..., :live]).view(np.uint32))
    assert np.array_equal(twice[..., live:].view(np.uint32), before[..., live:].view(np.uint32))
    # accumulate = 1 onto random content c, |c| <= A where records arrive (any value elsewhere: c + 0 is exact): the one more rounding,
    # of c + sum, is at most 2^-24 (|c| + A) <= 2 * 2^-24 * A, which the 16 of the bound still covers (brick_lists: twelve at most + one)
    A = bound / ((count + bl.ROUNDINGS) * bl.U32)
    content = rng.uniform(-1, 1, size=A.shape) * np.where(count > 0, A, 1.0)
    content = content.astype(np.float32)
    start = to_storage(content, K, storage, hip_device)
    added = channels(grid, *run(clone(start), True), K)
    check(variant + "-onto-content", added[..., :live], content[..., :live].astype(np.float64) + total[..., :live], bound[..., :live])
    assert np.array_equal(added[..., live:].view(np.uint32), content[..., live:].view(np.uint32))


@pytest.mark.parametrize("per_kind,base", [(1, 0), (2, 5), (3, 0), (8, 5)])
@pytest.mark.parametrize("dims", bl.GRIDS, ids=["x".join(map(str, d)) for d in bl.GRIDS])
@pytest.mark.parametrize("K,brick", [(9, 8), (16, 4), (9, ops.BRICK_4X8X8), (1, 4)])
def test_gradient_tensors_every_grid_and_list_count(hip_device, K, brick, dims, per_kind, base):
    """every grid x every list count (8 + 8 with one empty list of each kind, NaN prefix and tail) for four of the kernels, split storage"""
    kinds = ("wide", "narrow")
    grid = make_grid(dims, K, "split", hip_device)
    lists = device_lists(dims, brick, K, kinds, per_kind, base, hip_device)
    assert len(lists) == (2 * per_kind if K > 1 else 2 * min(per_kind, 4))
    total, bound, _ = reference(dims, brick, K, kinds)
    outs = []
    for _ in range(2):
        out = [None if t is None else torch.full_like(t, -7.0) for t in grid.kernel_tensors()]
        ops.brick_accumulate_raw(grid, brick, lists, out[0], out[1], accumulate=False)
        torch.cuda.synchronize()
        outs.append(out)
    assert same_bits(*outs)
    check(f"grad-K{K}-b{brick}-split-lists", channels(grid, *outs[0], K), total, bound)


# ---- Adam in the flush --------------------------------------------------------------------------------------------------------------
class AdamState:
    """a grid with optimizer state in its storage (m ~ U(-1, 1), v ~ U(0.5, 1.5): the distributions of test_hip_brick_narrow.py)"""

    def __init__(self, dims, K, storage, device, seed=5):
        self.dims, self.K, self.storage = dims, K, storage
        self.grid = make_grid(dims, K, storage, device)
        rng = np.random.default_rng(seed)
        C = 3 * K + 1
        self.p0 = clone(self.grid.kernel_tensors())
        self.m0 = to_storage(rng.uniform(-1, 1, size=tuple(dims) + (C,)), K, storage, device)
        self.v0 = to_storage(rng.uniform(0.5, 1.5, size=tuple(dims) + (C,)), K, storage, device)

    def run(self, brick, lists, probe=False, **kwargs):
        """one pass from the initial state -> (p, m, v) as pairs of tensors.  ``probe``: beta1 = 0 and m = 0, so that the first moment
        the pass leaves IS its gradient sum, m + (g - m) * 1 = g exactly: the sums of the optimizer kernels under the derived bound."""
        with torch.no_grad():
            for dst, src in zip(self.grid.kernel_tensors(), self.p0):
                if dst is not None:
                    dst.copy_(src)
            m = [None if t is None else torch.zeros_like(t) for t in self.m0] if probe else clone(self.m0)
            v = clone(self.v0)
            ops.brick_accumulate_adam_raw(self.grid, brick, lists, m, v, LR, 0.0 if probe else B1, B2, EPS, STEP, **kwargs)
        torch.cuda.synchronize()
        return clone(self.grid.kernel_tensors()), m, v

    def chan(self, pair):
        return channels(self.grid, *pair, self.K)

    def check_step(self, state, total, where=None):
        """(p, m, v) against the float64 Adam step on the gradient ``total`` (on the nodes ``where``), per tensor of the split channel
        arrangement, with the tolerances of test_brick_adam_with_base_channel_records"""
        p1, m1, v1 = (self.chan(t) for t in state)
        p, m, v = bl.adam_reference(self.chan(self.p0), self.chan(self.m0), self.chan(self.v0), total, LR, B1, B2, EPS, STEP)
        sel = (slice(None),) if where is None else (where,)
        for ch in ((slice(0, 4), slice(4, None)) if self.K > 1 else (slice(0, 4),)):
            bl.assert_adam_close(p1[sel][..., ch], m1[sel][..., ch], v1[sel][..., ch], p[sel][..., ch], m[sel][..., ch], v[sel][..., ch], LR)


ADAM_CASES = list(itertools.product((1, 9), bl.BRICK_SIZES, ("split", "bricked")))


@pytest.mark.parametrize("index", range(len(ADAM_CASES)), ids=[f"{K}-{b}-{s}" for K, b, s in ADAM_CASES])
def test_adam(hip_device, index):
    K, brick, storage = ADAM_CASES[index]
    mirror = brick == ops.BRICK_4X8X8 and storage == "split"
    dims = bl.GRIDS[1] if mirror else bl.GRIDS[(0, 3, 2, 1)[index % 4]]
    kinds = ("wide", "narrow")
    st = AdamState(dims, K, storage, hip_device)
    lists = device_lists(dims, brick, K, kinds, LISTS[index % 4], 7, hip_device)
    total, bound, _ = reference(dims, brick, K, kinds)
    mir = None
    if mirror:
        mir = (torch.full(tuple(dims) + (1,), 9.0, device=hip_device), torch.full(tuple(dims) + (3 * K,), 9.0, device=hip_device))
        assert ops.mirror_flush_applies(st.grid, brick, *mir)
    first = st.run(brick, lists, mirror=mir)
    st.check_step(first, total)
    if mirror:  # the mirror tensors are the updated parameters, bit for bit
        dens, feat = st.grid.unpack(*first[0])
        assert torch.equal(mir[0], dens) and torch.equal(mir[1], feat)
    second = st.run(brick, lists, mirror=mir)
    assert all(same_bits(a, b) for a, b in zip(first, second))  # deterministic
    probe = st.run(brick, lists, probe=True, mirror=mir)
    check(f"adam-K{K}-b{brick}-{storage}{'-mirror' if mirror else ''}", st.chan(probe[1]), total, bound)
    if storage == "bricked":  # the padding nodes of the storage are nobody's parameters
        nodes = to_storage(np.ones(tuple(dims) + (3 * K + 1,)), K, storage, hip_device)
        for after, before in zip(first, (st.p0, st.m0, st.v0)):
            for a, b, n in zip(after, before, nodes):
                assert a is None or torch.equal(a[n == 0], b[n == 0])


def _wide_from_base(rec, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((len(rec), 12), np.float32)
    out[:, :3], out[:, 3:7] = rec[:, :3], rec[:, 4:8]
    v = rng.normal(size=(len(rec), 3))
    out[:, 7:10] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return out


@pytest.mark.parametrize("K", [1, 9])
def test_adam_long_grid(hip_device, K):
    """8 x 1026 x 2046 (the ABI takes at most 2046 nodes per axis): more than 2^24 padded nodes, so brick size 8 takes the flush that is
    not one-round.  Records at both z ends and in four windows at random; the host reference covers those windows of z slabs (48 each)
    -- everywhere else the gradient is zero, and the zero-gradient step is checked on the device in float64 over the whole grid."""
    dims, brick = bl.LONG_GRID, 8
    C = 3 * K + 1
    base = bl.long_grid_records(seed=3)
    rec = base if K == 1 else _wide_from_base(base, 8)
    windows = bl.long_grid_windows(3)
    edges = bl.edges_of(brick)
    lists = bl.to_device(bl.sorted_lists(rec, dims, edges, 2, 3, seed=3), False, hip_device)
    gen = torch.Generator(device=hip_device).manual_seed(17)
    shapes = [tuple(dims) + (4,)] + ([tuple(dims) + (C - 4,)] if K > 1 else [])

    def rand(lo, hi):
        out = [torch.rand(s, generator=gen, device=hip_device) * (hi - lo) + lo for s in shapes]
        return out + [None] * (2 - len(out))

    p0, m0, v0 = rand(-1, 1), rand(-1, 1), rand(0.5, 1.5)
    dens, feat = unpack_split(p0[0], p0[1])
    grid = rf.VoxelGrid(dens, feat, rf.VoxelSize(0.1, 0.1, 0.1), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(),
                        expected_density_scale=3.0, tunable=True, storage="split")
    del dens, feat
    assert all(a is None or torch.equal(a, b) for a, b in zip(p0, grid.kernel_tensors()))

    def run(probe):
        with torch.no_grad():
            for dst, src in zip(grid.kernel_tensors(), p0):
                if dst is not None:
                    dst.copy_(src)
            m = [None if t is None else torch.zeros_like(t) for t in m0] if probe else clone(m0)
            v = clone(v0)
            ops.brick_accumulate_adam_raw(grid, brick, lists, m, v, LR, 0.0 if probe else B1, B2, EPS, STEP)
        torch.cuda.synchronize()
        return clone(grid.kernel_tensors()), m, v

    def window(pair, z0, z1):  # channel order [X, Y, z1 - z0, C]
        return np.concatenate([t[:, :, z0:z1].cpu().numpy() for t in pair if t is not None], axis=-1)

    first = run(False)
    probe = run(True)
    worst = 0.0
    for z0, z1 in windows:
        total, bound, _ = bl.scatter(rec, K > 1, dims, K, window=(z0, z1))
        got = window(probe[1], z0, z1)
        worst = max(worst, bl.mismatch(got, total, bound))
        p, m, v = bl.adam_reference(window(p0, z0, z1), window(m0, z0, z1), window(v0, z0, z1), total, LR, B1, B2, EPS, STEP)
        for ch in ((slice(0, 4), slice(4, None)) if K > 1 else (slice(0, 4),)):
            bl.assert_adam_close(window(first[0], z0, z1)[..., ch], window(first[1], z0, z1)[..., ch], window(first[2], z0, z1)[..., ch],
                                 p[..., ch], m[..., ch], v[..., ch], LR)
    print(f"BRICK_ERR variant=adam-K{K}-b8-long ratio={worst:.4f} rel=nan scale=nan")
    assert worst <= 1.0
    # outside the windows: no record, the zero-gradient step (same tolerances), and the probe's first moment is exactly zero
    outside = torch.ones(dims[2], dtype=torch.bool, device=hip_device)
    for z0, z1 in windows:
        outside[z0:z1] = False
    bc1, bc2 = 1.0 - B1 ** STEP, 1.0 - B2 ** STEP
    for i in range(2):
        if p0[i] is None:
            continue
        assert float(probe[1][i][:, :, outside].abs().max()) == 0.0
        m = m0[i][:, :, outside].double() * B1
        v = v0[i][:, :, outside].double() * B2
        p = p0[i][:, :, outside].double() - (LR / bc1) * m / (v.sqrt() / np.sqrt(bc2) + EPS)
        assert float((first[1][i][:, :, outside].double() - m).abs().max()) <= 1e-5 * float(m.abs().max())
        assert float((first[2][i][:, :, outside].double() - v).abs().max()) <= 1e-6 * float(v.abs().max())
        assert float((first[0][i][:, :, outside].double() - p).abs().max()) <= 1e-5 * LR + 2e-7
        del m, v, p
    assert all(same_bits(a, b) for a, b in zip(first, run(False)))


# ---- ranges -------------------------------------------------------------------------------------------------------------------------
def node_bricks(dims, edges):
    """[X, Y, Z] brick id of every node"""
    nb = bl.brick_counts(dims, edges)
    x, y, z = np.meshgrid(*[np.arange(d) // e for d, e in zip(dims, edges)], indexing="ij")
    return (x * nb[1] + y) * nb[2] + z


@pytest.mark.parametrize("brick", bl.BRICK_SIZES)
@pytest.mark.parametrize("K", [1, 9])
def test_adam_ranges(hip_device, K, brick):
    """rf_brick_accumulate_adam_range over a partition of the bricks into x-slab ranges, one slab cut into its first brick and the rest:
    together bit for bit the whole-grid pass; after each pass everything outside the range is bitwise unchanged; every key class that
    cannot touch the range is NaN (the owner of a range never receives those classes)."""
    dims, kinds = bl.RANGE_GRID, ("wide", "narrow")
    edges = bl.edges_of(brick)
    nb = bl.brick_counts(dims, edges)
    slab, nbricks = nb[1] * nb[2], nb[0] * nb[1] * nb[2]
    assert nb[0] >= 3 and slab > 1
    ranges = [(0, slab), (slab, 1), (slab + 1, slab - 1)] + [(s * slab, slab) for s in range(2, nb[0])]
    assert sum(n for _, n in ranges) == nbricks and ranges[-1][0] + ranges[-1][1] == nbricks
    st = AdamState(dims, K, "split", hip_device)
    whole = st.run(brick, device_lists(dims, brick, K, kinds, 2, 4, hip_device))
    total, bound, _ = reference(dims, brick, K, kinds)
    st.check_step(whole, total)
    owner = node_bricks(dims, edges)
    with torch.no_grad():
        for dst, src in zip(st.grid.kernel_tensors(), st.p0):
            if dst is not None:
                dst.copy_(src)
        m, v = clone(st.m0), clone(st.v0)
        for first, num in ranges:
            poison = ~bl.keys_touching(first, num, dims, edges)
            assert poison.any()
            lists = device_lists(dims, brick, K, kinds, 2, 4, hip_device, poison=poison)
            before = [st.chan(t) for t in (st.grid.kernel_tensors(), m, v)]
            ops.brick_accumulate_adam_raw(st.grid, brick, lists, m, v, LR, B1, B2, EPS, STEP, brick_range=(first, num))
            torch.cuda.synchronize()
            after = [st.chan(t) for t in (st.grid.kernel_tensors(), m, v)]
            out = (owner < first) | (owner >= first + num)
            for a, b in zip(after, before):
                assert np.isfinite(a).all()
                assert np.array_equal(a[out].view(np.uint32), b[out].view(np.uint32))
                assert not np.array_equal(a[~out], b[~out])
    assert all(same_bits(a, b) for a, b in zip(whole, (st.grid.kernel_tensors(), m, v)))


# ---- several workgroups per brick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [2, 3, 8])
@pytest.mark.parametrize("K", [1, 9])
def test_adam_split(hip_device, K, parts):
    """rf_brick_accumulate_adam_split over the x-slabs 1.. of bricks with 8 + 8 lists (a degree-0 grid: 4 + 4, one kind), one of each
    kind empty, the classes that cannot touch the range NaN.  The partial sums merge in the order the workgroups arrive, so results are
    held to sum64 / the float64 Adam step, not to the range pass bit for bit; the scratch counters are zero after every launch."""
    dims, brick, kinds = bl.RANGE_GRID, 8, ("wide", "narrow")
    edges = bl.edges_of(brick)
    nb = bl.brick_counts(dims, edges)
    slab, nbricks = nb[1] * nb[2], nb[0] * nb[1] * nb[2]
    rng_ = (slab, nbricks - slab)
    st = AdamState(dims, K, "split", hip_device)
    lists = device_lists(dims, brick, K, kinds, 8, 6, hip_device, poison=~bl.keys_touching(*rng_, dims, edges))
    assert len(lists) == (16 if K > 1 else 8)
    total, bound, _ = reference(dims, brick, K, kinds)
    owner = node_bricks(dims, edges)
    inside = owner >= slab
    scratch = ops.brick_split_scratch(st.grid, rng_[1], parts)
    counters = (rng_[1] * (1 + parts) * 4 + 255) // 256 * 256 // 4
    for launch in range(2):  # (the second launch finds the scratch the first one left)
        state = st.run(brick, lists, brick_range=rng_, split=(parts, scratch))
        assert int(scratch.view(torch.int32)[:counters].abs().max()) == 0
        st.check_step(state, total, where=inside)
        for t, t0 in zip(state, (st.p0, st.m0, st.v0)):
            a, b = st.chan(t), st.chan(t0)
            assert np.isfinite(a).all() and np.array_equal(a[~inside].view(np.uint32), b[~inside].view(np.uint32))
        probe = st.run(brick, lists, probe=True, brick_range=rng_, split=(parts, scratch))
        assert int(scratch.view(torch.int32)[:counters].abs().max()) == 0
        check(f"adam-K{K}-b8-split-parts{parts}", st.chan(probe[1])[inside], total[inside], bound[inside])
