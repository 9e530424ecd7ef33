"""The trainer-shaped instantiations of the two pair kernels (rf_step_kernel_specialised, $RF_STEP_SPECIALISED) against the generic
ones.  Both run the same per-ray source, compiled without contraction, so every comparison here is BITWISE: outputs, caches and
counters as they are, the gradient records of a key class as multisets (their order within a class comes from atomics)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from thr3ed_atom_amd import _lib, voxels
from thr3ed_atom_amd import ops as O
from thr3ed_atom_amd.optim import FlatGrid
from tests.helpers import hash_uniform

pytestmark = pytest.mark.gpu

BRICK = O.BRICK_4X8X8
# (dims, voxel edges, location): anisotropic voxels in an off-centre box, and 24^3 -- both leave partial 4 x 8 x 8 bricks
GRIDS = {
    "12x9x20": ((12, 9, 20), (0.25, 0.3, 0.1), (0.4, -0.3, 0.2)),
    "24^3": ((24, 24, 24), (0.125, 0.125, 0.125), (0.0, 0.0, 0.0)),
}
SAMPLES = (1, 63, 64, 65, 130)
RAY_COUNTS = (1, 3, 257)  # (odd: the second ray of the last block is empty)
NEAR, FAR = 0.05, 6.5
ACTS = {"relu": torch.nn.ReLU, "softplus": torch.nn.Softplus}


def T(a):
    return torch.from_numpy(np.asarray(a))


@functools.lru_cache(maxsize=None)
def field(name, deg, seed=0, dense=False):
    dims = GRIDS[name][0]
    F = 3 * (deg + 1) ** 2
    if dense:  # every node positive: with a large density scale the first sample inside the box takes all the transmittance
        dens = hash_uniform(dims + (1,), 11 + seed, 0.5, 1.0)
    else:  # about half the nodes negative: cells with sigma = 0, samples that are not cached
        dens = hash_uniform(dims + (1,), 11 + seed)
    return T(dens), T(hash_uniform(dims + (F,), 12 + seed))


def make_grid(dev, name, deg, mode="relu", storage="split", rho=100.0 / 3.0, dense=False):
    dims, voxel, location = GRIDS[name]
    dens, feat = field(name, deg, dense=dense)
    grid = rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*voxel), rf.VoxelGridLocation(*location), density_preactivation=torch.nn.Identity(),
                        density_postactivation=ACTS[mode](), expected_density_scale=rho, tunable=True, storage=storage)
    # as in the trainer, both tensors live in ONE flat buffer: near addressing (a condition of the rule) needs them inside one 4 GB
    # window, which two separate allocations do not promise
    FlatGrid(grid)
    return grid


@functools.lru_cache(maxsize=None)
def rays_of(name, n):
    """ray i: i % 3 == 0 crosses the box from outside, 1 starts INSIDE the box, 2 points away from it (misses)"""
    dims, voxel, location = GRIDS[name]
    half = 0.5 * np.array(dims) * np.array(voxel)
    centre = np.array(location)
    u = hash_uniform((n, 3), 70 + n).astype(np.float64)
    v = hash_uniform((n, 3), 71 + n).astype(np.float64)
    o = np.empty((n, 3))
    d = np.empty((n, 3))
    for i in range(n):
        kind = i % 3
        direction = u[i] / max(np.linalg.norm(u[i]), 1e-3)
        if kind == 1:
            o[i] = centre + 0.6 * half * v[i]
            d[i] = direction
        else:
            o[i] = centre - 4.0 * direction + 0.3 * half * v[i]
            d[i] = direction if kind == 0 else -direction
    return T(o.astype(np.float32)), T(d.astype(np.float32))


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def cached_slots(cmask, S):
    """[N, S] bool: slot 64 c + j of a ray holds the j-th cached sample of chunk c, j < popcount(mask of chunk c)"""
    m = cmask.cpu().numpy().view(np.uint64)
    counts = np.unpackbits(m.view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(-1)  # [N, chunks]
    j = np.arange(64)[None, None, :]
    return torch.from_numpy((j < counts[:, :, None]).reshape(m.shape[0], -1)[:, :S])


def assert_forward_equal(a, b, S, hist_a, hist_b, what):
    (out_a, caches_a), (out_b, caches_b) = a, b
    for name, x, y in zip(("colour", "depth", "acc", "disparity"), out_a, out_b):
        assert torch.equal(bits(x), bits(y)), f"{what}: {name}"
    assert torch.equal(caches_a[2], caches_b[2]), f"{what}: stop"
    assert torch.equal(caches_a[3], caches_b[3]), f"{what}: cmask"
    keep = cached_slots(caches_a[3], S).to(caches_a[0].device)
    assert torch.equal(bits(caches_a[0])[keep], bits(caches_b[0])[keep]), f"{what}: sample cache"
    assert torch.equal(bits(caches_a[1])[keep], bits(caches_b[1])[keep]), f"{what}: transmittance cache"
    assert torch.equal(hist_a, hist_b), f"{what}: key histogram"
    assert int(hist_a.sum()) == int(keep.sum()), f"{what}: one count per cached sample"


def sorted_classes(records, offsets):
    """the valid rows of a record list as int32, the rows of every key class sorted"""
    off = offsets.cpu().numpy()
    total = int(off[-1])
    rec = records[:total].cpu().numpy().view(np.int32)
    cls = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.lexsort(tuple(rec[:, c] for c in range(rec.shape[1] - 1, -1, -1)) + (cls,))
    return rec[order]


def assert_lists_equal(a, b, what):
    (cursor_a, offsets_a, records_a), (cursor_b, offsets_b, records_b) = a, b
    assert torch.equal(cursor_a, cursor_b), f"{what}: cursors"
    assert torch.equal(offsets_a, offsets_b), f"{what}: offsets"
    assert torch.equal(cursor_a.to(torch.int64), offsets_a[1:]), f"{what}: every class filled exactly"
    assert np.array_equal(sorted_classes(records_a, offsets_a), sorted_classes(records_b, offsets_b)), f"{what}: records"


class Case:
    """one pair of renders (specular + render_diffuse of the same rays) through the pair entry points or launch by launch"""

    def __init__(self, dev, grid, name, n, S, white, aabb=False, occ=False, tables=False):
        self.dev, self.grid, self.n, self.S = dev, grid, n, S
        o, d = rays_of(name, n)
        self.o, self.d = o.to(dev), d.to(dev)
        self.flags = [O.render_flags(white, diffuse, aabb, occ) for diffuse in (False, True)]
        if tables:
            self.jit = [T(hash_uniform((n, S), 90 + i, 0.0, 1.0)).to(dev) for i in range(2)]
        else:
            self.jit = [O.KeyedJitter(0x1234567 + 977 * i, 5) for i in range(2)]
        nb = O.brick_counts(grid, BRICK)
        self.nkeys = 8 * nb[0] * nb[1] * nb[2]
        self.g_colours = [T(hash_uniform((n, 3), 95 + i)).to(dev) for i in range(2)]
        self.floats = [O.expanded_record_floats(grid, diffuse) for diffuse in (False, True)]

    def query(self):
        """rf_step_kernel_specialised for the descriptors the forward pair launch gets"""
        rf_grid = self.grid.forward_rf_grid(use_occupancy=bool(self.flags[0] & _lib.FLAG_OCCUPANCY_SKIP))
        rays, fl, keep = (_lib.RFRayBatch * 2)(), (C.c_uint32 * 2)(), []
        for i in range(2):
            rays[i], tv = O._ray_batch(self.o, self.d, self.S, NEAR, FAR, self.jit[i])
            fl[i] = O._jitter_flags(self.flags[i], self.jit[i])
            keep.append(tv)
        return _lib.load().rf_step_kernel_specialised(C.byref(rf_grid), rays, fl)

    def hists(self):
        return [torch.zeros(self.nkeys, dtype=torch.int32, device=self.dev) for _ in range(2)]

    def forward_pair(self):
        hists = self.hists()
        res = O.render_forward_pair_raw(self.grid, self.o, self.d, self.jit, self.S, NEAR, FAR, self.flags, hists, BRICK)
        assert res is not None
        return res, hists

    def forward_singles(self):
        hists, res = self.hists(), []
        for i in range(2):
            *out, caches = O.render_forward_raw(self.grid, self.o, self.d, self.jit[i], self.S, NEAR, FAR, self.flags[i], save=True, key_hist=hists[i], brick_size=BRICK)
            res.append((tuple(out), caches))
        return res, hists

    def _lists(self):
        offsets = torch.zeros((2, self.nkeys + 1), dtype=torch.int64, device=self.dev)
        cursor = torch.zeros((2, self.nkeys), dtype=torch.int32, device=self.dev)
        records = [torch.empty((self.n * self.S, f), device=self.dev) for f in self.floats]
        return offsets, cursor, records

    def emit_pair(self, fwd, hists):
        hists = [h.clone() for h in hists]
        offsets, cursor, records = self._lists()
        caches2 = [fwd[i][1] for i in range(2)]
        assert O.render_backward_emit_direct_pair_raw(self.grid, self.o, self.d, self.jit, self.S, NEAR, FAR, self.flags, caches2, self.g_colours, BRICK, hists,
                                                      offsets, cursor, records)
        assert all(int(h.abs().sum()) == 0 for h in hists)  # (the adjoint clears the forward pass's counters)
        return [(cursor[i], offsets[i], records[i]) for i in range(2)]

    def emit_singles(self, fwd, hists):
        hists = [h.clone() for h in hists]
        offsets, cursor, records = self._lists()
        for i in range(2):
            O.bin_offsets(hists[i], offsets[i], cursor[i])
            O.render_backward_emit_direct_raw(self.grid, self.o, self.d, self.jit[i], self.S, NEAR, FAR, self.flags[i], fwd[i][1], self.g_colours[i], None, None, BRICK,
                                              cursor[i], records[i], hist_clear=hists[i])
        return [(cursor[i], offsets[i], records[i]) for i in range(2)]


def on_against_off(case, monkeypatch, what):
    """forward pair and adjoint pair with the specialised instantiations against the generic ones; returns the forward results"""
    monkeypatch.delenv("RF_STEP_SPECIALISED", raising=False)
    assert case.query() == 1, what
    fwd_on, hist_on = case.forward_pair()
    lists_on = case.emit_pair(fwd_on, hist_on)
    monkeypatch.setenv("RF_STEP_SPECIALISED", "0")
    assert case.query() == 0, what
    fwd_off, hist_off = case.forward_pair()
    lists_off = case.emit_pair(fwd_on, hist_on)  # (the same caches and counters: the adjoints are compared on equal inputs)
    monkeypatch.delenv("RF_STEP_SPECIALISED")
    for i, render in enumerate(("specular", "diffuse")):
        assert_forward_equal(fwd_on[i], fwd_off[i], case.S, hist_on[i], hist_off[i], f"{what} {render}")
        assert_lists_equal(lists_on[i], lists_off[i], f"{what} {render}")
    return fwd_on


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(GRIDS))
def test_specialised_pair_kernels_equal_generic_bitwise(hip_device, monkeypatch, name, deg):
    """switch on against switch off, forward pair and adjoint pair, every sample count x ray count, white background alternating with
    the ray count and taken both ways at the largest case"""
    grid = make_grid(hip_device, name, deg)
    cached = 0
    for S in SAMPLES:
        for k, n in enumerate(RAY_COUNTS):
            for white in ((False, True) if (S, n) == (130, 257) else (bool((k + S) & 1),)):
                case = Case(hip_device, grid, name, n, S, white)
                fwd = on_against_off(case, monkeypatch, f"{name} deg={deg} S={S} n={n} white={white}")
                cached += int(cached_slots(fwd[0][1][3], S).sum())
                if n == 257 and S > 1:  # (a ray's only sample sits at `near`: in front of the box for the rays from outside)
                    acc = fwd[0][0][2].flatten().cpu()
                    assert float(acc[0::3].max()) > 0.0 and float(acc[1::3].max()) > 0.0  # rays from outside and from inside hit the field
                    assert float(acc[2::3].abs().max()) == 0.0  # rays that miss the box
    assert cached > 0


@pytest.mark.parametrize("name", list(GRIDS))
def test_specialised_pair_kernels_early_exit(hip_device, monkeypatch, name):
    """a dense field with a huge density scale: the transmittance reaches exactly 0 and the walk stops before the ray's last chunk"""
    grid = make_grid(hip_device, name, 2, rho=1.0e6, dense=True)
    S = 130
    case = Case(hip_device, grid, name, 257, S, True)
    fwd = on_against_off(case, monkeypatch, f"{name} dense")
    stop = fwd[0][1][2].cpu()
    assert int(stop[0::3].min()) < S  # (a ray through the box stopped early)
    assert float(fwd[0][0][2].max()) > 0.99


RULE_CASES = {
    "trainer-shaped": (1, {}),
    "reference layout": (0, {"storage": "reference"}),
    "bricked": (0, {"storage": "bricked"}),
    "softplus": (0, {"mode": "softplus"}),
    "jitter table": (0, {"tables": True}),
    "occupancy skip": (0, {"occ": True}),
    "AABB sampling": (0, {"aabb": True}),
    "far addressing": (0, {"far": True}),
}


@pytest.mark.parametrize("broken", list(RULE_CASES))
def test_rule_and_pair_against_single_launches(hip_device, monkeypatch, broken):
    """the query says 1 for the trainer-shaped case and 0 when exactly one condition is broken; either way the pair entry points equal
    the two single-render launches (which have no specialised instantiation) bitwise"""
    expect, how = RULE_CASES[broken]
    monkeypatch.delenv("RF_STEP_SPECIALISED", raising=False)
    if how.get("far"):
        monkeypatch.setenv("RF_FAR_ADDRESSING", "1")
    if how.get("storage") == "reference":
        monkeypatch.setattr(voxels, "SPLIT_SHADOW", False)  # (the forward pass gathers from the reference's own tensors)
    name, S, n = "12x9x20", 65, 257
    grid = make_grid(hip_device, name, 2, mode=how.get("mode", "relu"), storage=how.get("storage", "split"))
    if how.get("occ"):
        grid.build_occupancy()
    case = Case(hip_device, grid, name, n, S, True, aabb=bool(how.get("aabb")), occ=bool(how.get("occ")), tables=bool(how.get("tables")))
    assert case.query() == expect
    fwd_pair, hist_pair = case.forward_pair()
    fwd_one, hist_one = case.forward_singles()
    lists_pair = case.emit_pair(fwd_pair, hist_pair)
    lists_one = case.emit_singles(fwd_pair, hist_pair)
    for i, render in enumerate(("specular", "diffuse")):
        assert_forward_equal(fwd_pair[i], fwd_one[i], S, hist_pair[i], hist_one[i], f"{broken} {render}")
        assert_lists_equal(lists_pair[i], lists_one[i], f"{broken} {render}")
    assert int(hist_pair[0].sum()) > 0


def test_query_argument_checks(hip_device):
    """error codes before anything else"""
    lib = _lib.load()
    assert lib.rf_step_kernel_specialised(None, None, None) == -1
    grid = make_grid(hip_device, "24^3", 0)
    assert lib.rf_step_kernel_specialised(C.byref(grid.to_rf_grid()), None, None) == -1
    case = Case(hip_device, grid, "24^3", 3, 8, False)
    case.flags = case.flags[::-1]  # ([0] must be the specular render, [1] render_diffuse)
    assert case.query() == _lib.ERR_UNSUPPORTED
