"""GPU: the record batches of the brick pass on crafted sorted lists, against the float64 scatter-add of tests/brick_lists.py under its
derived float32 bound.

The 4 x 8 x 8 pass of an SH-2 grid sums the base-channel (render_diffuse) records in batches of up to 256, one thread per record, and
the full-width records in batches of 128, two threads per record (the first reads the index, d density and d raw quads, the second
d raw and the viewing direction).  One TARGET brick receives exactly n base-channel and m full-width record instances, n and m around the batch
sizes; the records sit on every face, edge and corner of the brick -- lower node c = -1 (they arrive from a lower neighbour's key
classes) and c = edge - 1 on every axis, 1, 2 and 4 yz-blocks --, in eight and more key classes, none of which holds a whole batch.
Further bricks see one kind of record only, or nothing (written as zeros).  Two launches of every case are bit-identical."""
import functools
import itertools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import brick_lists as bl
from thr3ed_atom_amd import ops

pytestmark = pytest.mark.gpu

K = 9
C = 3 * K + 1
EDGES = (4, 8, 8)
BRICK = ops.BRICK_4X8X8
BASE_BATCH, WIDE_BATCH = 256, 128  # records per batch of the 4 x 8 x 8 pass (base-channel, full-width)
BOUNDARY_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513)
# grid -> target brick.  (8, 16, 24): whole bricks (the mirror flush needs them); no record of the target reaches the bricks bz = 0
TARGETS = {(10, 13, 17): (1, 1, 1), (8, 16, 24): (1, 1, 2)}
LR, B1, B2, EPS, STEP = 0.03, 0.9, 0.999, 1e-8, 3


def brick_id(b3, dims):
    nb = bl.brick_counts(dims, EDGES)
    return (b3[0] * nb[1] + b3[1]) * nb[2] + b3[2]


def target_lowers(dims, target):
    """lower nodes of cells that reach the target brick, relative coordinate c per axis out of: -1 (from the lower neighbour), 0, the
    nodes on both sides of the yz-block boundary (3, 4), edge - 1 (the upper node belongs to the next brick, or to nobody) -- every
    combination that exists in the grid: corners, edges and faces of the brick and of its four yz-blocks"""
    rel = [(-1, -1, 0, 1, 3), (-1, -1, 0, 3, 4, 7), (-1, -1, 0, 3, 4, 7)]  # (c = -1 twice: no key class gets a whole batch)
    org = np.array(target) * np.array(EDGES)
    lower = np.array(list(itertools.product(*rel))) + org
    lower = lower[np.all((lower >= 0) & (lower < np.array(dims)), axis=1)]
    assert bl.reaches_brick(lower, brick_id(target, dims), dims, EDGES).all()
    for ax in range(3):  # c = -1 and c = edge - 1 are there on every axis
        assert (lower[:, ax] == org[ax] - 1).any() and (lower[:, ax] == min(org[ax] + EDGES[ax], dims[ax]) - 1).any()
    return lower


def positions(lower, rng):
    pos = (lower + rng.uniform(0.0, 1.0, size=lower.shape)).astype(np.float32)
    pos[::7, 0] = lower[::7, 0]  # fractional part exactly 0: the upper node is reached with weight zero
    pos[3::11, 1:] = lower[3::11, 1:]
    return np.minimum(pos, np.nextafter((lower + 1).astype(np.float32), np.float32(0.0)))


def make_records(lower, wide, rng, scale=(1.0, 1.0, 1.0, 1.0)):
    rec = np.zeros((len(lower), 12 if wide else 8), np.float32)
    rec[:, :3] = positions(lower, rng)
    vals = rng.uniform(0.25, 1.0, size=(len(rec), 4)) * rng.choice([-1.0, 1.0], size=(len(rec), 4)) * np.array(scale)
    if wide:
        rec[:, 3:7] = vals
        v = rng.uniform(0.2, 1.0, size=(len(rec), 3)) * rng.choice([-1.0, 1.0], size=(len(rec), 3))  # no axis-aligned direction
        rec[:, 7:10] = v / np.linalg.norm(v, axis=1, keepdims=True)
    else:
        rec[:, 4:8] = vals
    assert np.array_equal(np.floor(rec[:, :3]).astype(np.int64), lower)
    return rec


def target_records(dims, count, wide, seed):
    """``count`` records that all reach the target brick, dealt over ``target_lowers`` in a shuffled order (so that a short list already
    comes from several key classes)"""
    rng = np.random.default_rng(seed)
    cells = target_lowers(dims, TARGETS[dims])
    cells = cells[rng.permutation(len(cells))]
    return make_records(cells[np.arange(count) % len(cells)], wide, rng)


def background_records(dims, wide, seed):
    """records that do not reach the target brick: on (8, 16, 24) full-width ones inside brick (0, 0, 0) and base-channel ones inside
    brick (0, 1, 0) -- a brick of each kind alone; nothing reaches bricks (1, 0, 0) and (1, 1, 0) --, on the other grid both kinds in brick 0"""
    rng = np.random.default_rng(seed)
    y0 = 8 if (dims == (8, 16, 24) and not wide) else 0
    lower = np.stack([rng.integers(0, 3, 200), y0 + rng.integers(0, 7, 200), rng.integers(0, 7, 200)], axis=1)
    assert not bl.reaches_brick(lower, brick_id(TARGETS[dims], dims), dims, EDGES).any()
    return make_records(lower, wide, rng)


@functools.lru_cache(maxsize=None)
def case(dims, m, n):
    """(full-width records, base-channel records, float64 sum, bound) of a pass whose target brick receives m + n record instances"""
    wide = np.concatenate([target_records(dims, m, True, 100 + m), background_records(dims, True, 7)])
    narrow = np.concatenate([target_records(dims, n, False, 200 + n), background_records(dims, False, 8)])
    target = brick_id(TARGETS[dims], dims)
    for rec, count, batch in ((wide, m, WIDE_BATCH), (narrow, n, BASE_BATCH)):
        lower = np.floor(rec[:, :3]).astype(np.int64)
        reach = bl.reaches_brick(lower, target, dims, EDGES)
        assert int(reach.sum()) == count  # exactly that many instances
        if count > batch:  # the records behind the first batch come from another key range than the first record
            classes = np.unique(bl.record_keys(rec[reach], dims, EDGES), return_counts=True)[1]
            assert len(classes) >= 8 and classes.max() < batch
    total, bound, cnt = bl.expected(("wide", "narrow"), wide, narrow, dims, K)
    assert cnt.max() <= bl.MAX_COUNT
    return wide, narrow, total, bound


def make_grid(dims, device, seed=3):
    rng = np.random.default_rng(seed)
    dens = torch.from_numpy(rng.uniform(-1, 1, size=tuple(dims) + (1,)).astype(np.float32))
    feat = torch.from_numpy(rng.uniform(-1, 1, size=tuple(dims) + (3 * K,)).astype(np.float32))
    return rf.VoxelGrid(dens.to(device), feat.to(device), rf.VoxelSize(0.1, 0.1, 0.1), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=3.0, tunable=True, storage="split")


def device_lists(wide, narrow, dims, edges, device, per_kind=1):
    return (bl.to_device(bl.sorted_lists(wide, dims, edges, per_kind, 0, seed=3), False, device)
            + bl.to_device(bl.sorted_lists(narrow, dims, edges, per_kind, 0, seed=4), True, device))


def channels(grid, first, second):
    dens, feat = grid.unpack(first, second)
    return bl.from_reference(dens.detach().cpu().numpy(), feat.detach().cpu().numpy(), K)


def gradient_sums(grid, brick, lists):
    """rf_brick_accumulate twice onto garbage: bit-identical; -> [X, Y, Z, C]"""
    outs = []
    for _ in range(2):
        out = [torch.full_like(t, 7.0) for t in grid.kernel_tensors()]
        ops.brick_accumulate_raw(grid, brick, lists, out[0], out[1], accumulate=False)
        torch.cuda.synchronize()
        outs.append(out)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs))
    return channels(grid, *outs[0])


def check(what, got, total, bound):
    worst = bl.mismatch(got, total, bound)
    print(f"BRICK_ERR variant={what} ratio={worst:.4f}")
    bl.assert_within_bound(got, total, bound, what)


def check_empty_bricks(dims, got):
    if dims == (8, 16, 24):  # bricks (1, 0, 0) and (1, 1, 0): nothing reaches them
        assert float(np.abs(got[4:, :, :8]).max()) == 0.0


@pytest.mark.parametrize("n", BOUNDARY_COUNTS)
@pytest.mark.parametrize("dims", list(TARGETS), ids=["x".join(map(str, d)) for d in TARGETS])
def test_base_channel_batch_boundaries(hip_device, dims, n):
    """the target brick receives n base-channel records and no full-width one (other bricks of the pass do)"""
    wide, narrow, total, bound = case(dims, 0, n)
    grid = make_grid(dims, hip_device)
    got = gradient_sums(grid, BRICK, device_lists(wide, narrow, dims, EDGES, hip_device))
    check(f"batches-{'x'.join(map(str, dims))}-m0-n{n}", got, total, bound)
    check_empty_bricks(dims, got)


@pytest.mark.parametrize("m,n", [(m, n) for m in (0, 1, 128, 129, 257) for n in (0, 1, 129, 256, 257) if m + n > 0 and (m, n) != (0, 1)]
                         + [(128, 513), (257, 300)])
def test_both_kinds_in_one_brick(hip_device, m, n):
    """m full-width and n base-channel records in the target brick: the block table of the base-channel batches takes the place of the
    full-width batch's rows and weight table -- a full last full-width batch under a short base-channel batch and the reverse; the grid
    also has a brick with full-width records only, one with base-channel records only and two that nothing reaches"""
    dims = (8, 16, 24)
    wide, narrow, total, bound = case(dims, m, n)
    grid = make_grid(dims, hip_device)
    got = gradient_sums(grid, BRICK, device_lists(wide, narrow, dims, EDGES, hip_device))
    check(f"batches-8x16x24-m{m}-n{n}", got, total, bound)
    check_empty_bricks(dims, got)
    assert float(np.abs(got[:4, :8, :8, 4:]).max()) > 0.0 and float(np.abs(got[:4, 8:, :8, 4:]).max()) == 0.0  # the bricks of one kind
    assert float(np.abs(got[:4, 8:, :8, :4]).max()) > 0.0


# ---- the quads of a full-width record, by the role each has in the two threads' record pass ---------------------------------------------
def role_records(dims, seed):
    """full-width records whose fields differ by decades (d density ~ 1000, d raw r, g, b ~ 1, 10, 100) with oblique viewing
    directions: a quad read in the wrong role, or a shifted field, leaves the bound by orders of magnitude"""
    rng = np.random.default_rng(seed)
    lat = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    lower = np.concatenate([lat[::3], rng.integers(0, np.array(dims), size=(600, 3))])
    return make_records(lower, True, rng, scale=(1000.0, 1.0, 10.0, 100.0))


@pytest.mark.parametrize("brick", [BRICK, 8])
def test_full_width_quads_by_role(hip_device, brick):
    dims = (10, 13, 17)
    wide = role_records(dims, 31)
    total, bound, _ = bl.scatter(wide, True, dims, K)
    grid = make_grid(dims, hip_device)
    lists = bl.to_device(bl.sorted_lists(wide, dims, bl.edges_of(brick), 1, 0, seed=3), False, hip_device)
    check(f"roles-b{brick}", gradient_sums(grid, brick, lists), total, bound)


class AdamRun:
    """optimizer state of test_hip_brick_narrow.py (m ~ U(-1, 1), v ~ U(0.5, 1.5)) and passes from it"""

    def __init__(self, dims, device):
        self.grid = make_grid(dims, device)
        rng = np.random.default_rng(5)
        self.p0 = [t.detach().clone() for t in self.grid.kernel_tensors()]
        self.m0 = [torch.from_numpy(rng.uniform(-1, 1, size=t.shape).astype(np.float32)).to(device) for t in self.p0]
        self.v0 = [torch.from_numpy(rng.uniform(0.5, 1.5, size=t.shape).astype(np.float32)).to(device) for t in self.p0]

    def run(self, brick, lists, probe=False, **kwargs):
        """(p, m, v) of one pass from the initial state; ``probe``: beta1 = 0 and m = 0, so the first moment left IS the gradient sum"""
        with torch.no_grad():
            for dst, src in zip(self.grid.kernel_tensors(), self.p0):
                dst.copy_(src)
            m = [torch.zeros_like(t) if probe else t.clone() for t in self.m0]
            v = [t.clone() for t in self.v0]
            ops.brick_accumulate_adam_raw(self.grid, brick, lists, m, v, LR, 0.0 if probe else B1, B2, EPS, STEP, **kwargs)
        torch.cuda.synchronize()
        return [t.detach().clone() for t in self.grid.kernel_tensors()], m, v

    def chan(self, pair):
        return channels(self.grid, *pair)

    def check_step(self, state, total):
        p1, m1, v1 = (self.chan(t) for t in state)
        p, m, v = bl.adam_reference(self.chan(self.p0), self.chan(self.m0), self.chan(self.v0), total, LR, B1, B2, EPS, STEP)
        for ch in (slice(0, 4), slice(4, None)):
            bl.assert_adam_close(p1[..., ch], m1[..., ch], v1[..., ch], p[..., ch], m[..., ch], v[..., ch], LR)


def test_full_width_quads_by_role_split(hip_device):
    """several workgroups per 8^3 brick (rf_brick_accumulate_adam_split): the gradient sum read off a probe step"""
    dims, brick, parts = (10, 13, 17), 8, 2
    wide = role_records(dims, 32)
    total, bound, _ = bl.scatter(wide, True, dims, K)
    st = AdamRun(dims, hip_device)
    nb = bl.brick_counts(dims, bl.edges_of(brick))
    nbricks = nb[0] * nb[1] * nb[2]
    lists = bl.to_device(bl.sorted_lists(wide, dims, bl.edges_of(brick), 4, 0, seed=3), False, hip_device)  # (list 2 is empty)
    scratch = ops.brick_split_scratch(st.grid, nbricks, parts)
    probe = st.run(brick, lists, probe=True, brick_range=(0, nbricks), split=(parts, scratch))
    check("roles-b8-split", st.chan(probe[1]), total, bound)


@pytest.mark.parametrize("dims,mirror", [((10, 13, 17), False), ((8, 16, 24), True)])
def test_adam_over_batch_boundaries(hip_device, dims, mirror):
    """the optimizer flush (and its mirror write-out) behind 129 full-width and 257 base-channel records in the target brick"""
    wide, narrow, total, bound = case(dims, 129, 257)
    st = AdamRun(dims, hip_device)
    lists = device_lists(wide, narrow, dims, EDGES, hip_device)
    mir = None
    if mirror:
        mir = (torch.full(tuple(dims) + (1,), 9.0, device=hip_device), torch.full(tuple(dims) + (3 * K,), 9.0, device=hip_device))
        assert ops.mirror_flush_applies(st.grid, BRICK, *mir)
    first = st.run(BRICK, lists, mirror=mir)
    st.check_step(first, total)
    if mirror:  # the mirror tensors are the updated parameters, bit for bit
        dens, feat = st.grid.unpack(*first[0])
        assert torch.equal(mir[0], dens) and torch.equal(mir[1], feat)
    second = st.run(BRICK, lists, mirror=mir)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for x, y in zip(first, second) for a, b in zip(x, y))
    probe = st.run(BRICK, lists, probe=True, mirror=mir)
    check(f"batches-adam-{'x'.join(map(str, dims))}{'-mirror' if mirror else ''}", st.chan(probe[1]), total, bound)
