"""rf_label_components and floater removal on the GPU against the numpy model (tests/components_model.py).  Every comparison is
exact: labels, sizes, removed densities and statistics bit for bit -- there is no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import components_model as cm
from tests.helpers import hash_uniform, hotdog_like_camera, procedural_grid, sparse_scene_grid
from thr3ed_atom_amd import _lib, ops
from thr3ed_atom_amd.mesh import read_ply
from thr3ed_atom_amd.trainers import PosedImagesInMemory, train_sh_vox_grid_vol_mod_with_posed_images
from thr3ed_atom_amd.voxels import brick_nodes

pytestmark = pytest.mark.gpu

STORAGES = ["reference", "split", "bricked"]
CONNECTIVITIES = [6, 18, 26]
MODES = ["relu", "abs", "softplus", "identity"]
ACTIVATIONS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
               "abs": (torch.abs, torch.nn.Identity()), "identity": (torch.nn.Identity(), torch.nn.Identity())}
FEATURES = [3, 12, 27]
OCCUPATIONS = [0.2, 0.31, 0.6]  # 0.31: the site-percolation threshold of the cubic lattice -- large ragged clusters across many tile faces
# (17, 9, 33): more than one tile along every axis, with partial tiles
DIMS = [(1, 1, 1), (2, 2, 2), (3, 4, 5), (9, 8, 17), (16, 16, 24), (17, 9, 33)]
TILE = _lib.COMPONENT_TILE
SENTINEL = 0x7F7F7F7F
# (rho, threshold) per mode; softplus: tau = softplus(0), and every raw value below is at least 0.05 away from 0
SETTINGS = {"relu": (2.0, 0.5), "abs": (1.0, 0.5), "softplus": (1.0, float(np.float32(np.log(2.0)))), "identity": (1.5, 0.0)}


def case_table():
    """(dims, connectivity, mode, occupation) for every dims x connectivity; a storage then takes F = FEATURES[(i + j + s) % 3]"""
    return [(dims, c, MODES[(i + j) % 4], OCCUPATIONS[(i + 2 * j) % 3]) for i, dims in enumerate(DIMS) for j, c in enumerate(CONNECTIVITIES)]


def features_of(dims, connectivity, storage):
    return FEATURES[(DIMS.index(dims) + CONNECTIVITIES.index(connectivity) + STORAGES.index(storage)) % 3]


def test_the_case_table_meets_every_value_of_every_factor():
    table = case_table()
    assert {(c, m) for _, c, m, _ in table} == {(c, m) for c in CONNECTIVITIES for m in MODES}
    assert {(c, p) for _, c, _, p in table} == {(c, p) for c in CONNECTIVITIES for p in OCCUPATIONS}
    assert {d for d, *_ in table} == set(DIMS) and len(table) == len(DIMS) * len(CONNECTIVITIES)
    # every storage runs the whole table, and meets every F under every connectivity
    assert {(s, c, features_of(d, c, s)) for d, c, _, _ in table for s in STORAGES} == {(s, c, F) for s in STORAGES for c in CONNECTIVITIES for F in FEATURES}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def raw_densities(dims, mode, p, seed=5):
    """float32 [X,Y,Z,1]: about a fraction p of the nodes occupied under SETTINGS[mode], every value well away from the threshold"""
    u, s = hash_uniform(dims, seed, 0.0, 1.0), np.where(hash_uniform(dims, seed + 1) < 0, np.float32(-1.0), np.float32(1.0))
    occ = u < p
    if mode == "relu":      # sigma = max(2 D, 0) against 0.5: occupied >= 0.6, the rest <= 0.2 (negative and small positive values)
        d = np.where(occ, 0.3 + u, 0.1 * s * u)
    elif mode == "abs":     # sigma = |D| against 0.5: negative raw values count
        d = np.where(occ, s * (0.6 + u), 0.3 * s * u)
    elif mode == "softplus":
        d = np.where(occ, 0.05 + u, -0.05 - u)
    else:                   # identity: sigma = 1.5 D against 0
        d = np.where(occ, 0.1 + u, -u)
    return np.ascontiguousarray(d.astype(np.float32)[..., None])


@functools.lru_cache(maxsize=None)
def model_of(dims, mode, p, connectivity):
    """(labels, sizes) of the model: computed once, shared by the storages, never written"""
    rho, tau = SETTINGS[mode]
    labels = cm.label(cm.occupied(raw_densities(dims, mode, p), rho, mode, tau), connectivity)
    sizes = cm.sizes_of(labels)
    labels.setflags(write=False)
    sizes.setflags(write=False)
    return labels, sizes


def make_grid(dev, dens, F, storage, mode="relu", rho=1.0, seed=9):
    dens = T(np.asarray(dens, dtype=np.float32)) if not torch.is_tensor(dens) else dens
    dims = tuple(dens.shape[:3])
    feat = T(hash_uniform((*dims, F), seed))
    return rf.VoxelGrid(dens.clone().to(dev), feat.to(dev), rf.VoxelSize(0.25, 0.25, 0.25), density_preactivation=ACTIVATIONS[mode][0],
                        density_postactivation=ACTIVATIONS[mode][1], expected_density_scale=rho, tunable=False, storage=storage)


def padding_mask(grid, like):
    X, Y, Z = grid.grid_dims
    real = brick_nodes(torch.ones((X, Y, Z, 1), device=like.device))
    return (real == 0).expand_as(like)


def poison_padding(grid, value):
    """bricked storage: fill the padding nodes; a kernel that addressed one would see an occupied node (1e9) or leave a trace (NaN)"""
    if grid.storage == "bricked":
        for t in grid.kernel_tensors():
            if t is not None:
                t.data[padding_mask(grid, t)] = value


def launch(grid, threshold, connectivity, with_sizes=True):
    """labels / sizes of one call into sentinel-filled buffers with sentinels behind their ends; returns host arrays"""
    dims = tuple(int(v) for v in grid.grid_dims)
    n = int(np.prod(dims))
    dev = grid.kernel_tensors()[0].device
    whole_l = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=dev)
    whole_s = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=dev)
    ops.label_components_raw(grid, threshold, connectivity, whole_l[:n].view(dims), whole_s[:n] if with_sizes else None)
    assert bool((whole_l[n:] == SENTINEL).all()) and bool((whole_s[n if with_sizes else 0:] == SENTINEL).all()), "written outside the buffers"
    return whole_l[:n].view(dims).cpu().numpy(), (whole_s[:n].cpu().numpy() if with_sizes else None)


def relu_mask_grid(dev, mask, storage, F=3):
    """a ReLU grid (rho 1, threshold 0) whose occupied nodes are exactly ``mask``: +1 / -1"""
    grid = make_grid(dev, np.where(mask, np.float32(1.0), np.float32(-1.0))[..., None], F, storage)
    poison_padding(grid, 1e9)
    return grid


# --------------------------------------------------------------------------------------------
# the kernel against the model
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_labels_and_sizes_equal_the_model_bit_for_bit(hip_device, dims, storage):
    for d, connectivity, mode, p in case_table():
        if d != dims:
            continue
        rho, tau = SETTINGS[mode]
        grid = make_grid(hip_device, raw_densities(dims, mode, p), features_of(dims, connectivity, storage), storage, mode, rho)
        poison_padding(grid, 1e9)
        want_labels, want_sizes = model_of(dims, mode, p, connectivity)
        labels, sizes = launch(grid, tau, connectivity)
        assert labels.dtype == np.int32 and np.array_equal(labels, want_labels), (connectivity, mode, p)
        assert np.array_equal(sizes, want_sizes), (connectivity, mode, p)


@functools.lru_cache(maxsize=None)
def serpentine(dims):
    """a one-node-thick face-connected path through the whole grid: every other x plane is swept row by row (every other y row, joined
    alternately at the two z ends), consecutive planes are joined by one node at alternating ends of the sweep"""
    X, Y, Z = dims
    mask = np.zeros(dims, dtype=bool)
    rows = list(range(0, Y, 2))
    for x in range(0, X, 2):
        for y in rows:
            mask[x, y, :] = True
        for j, y in enumerate(rows[:-1]):
            mask[x, y + 1, Z - 1 if j % 2 == 0 else 0] = True
    end = (rows[-1], Z - 1 if len(rows) % 2 == 1 else 0)  # where the sweep that starts at (0, 0) ends
    for k, x in enumerate(range(1, X - 1, 2)):
        y, z = end if k % 2 == 0 else (0, 0)
        mask[x, y, z] = True
    mask.setflags(write=False)
    return mask


# pairs of nodes that touch by a face, an edge or a corner only, placed ACROSS a face, an edge and a corner of the kernel's tiles,
# every pair at least two nodes away from every other
def boundary_pairs():
    t = TILE
    return [
        ("face", (t - 1, 2, 2), (t, 2, 2)),                    # across the x face of a tile
        ("face", (12, t - 1, 2), (12, t, 2)),                  # ... the y face
        ("face", (2, 2, 2 * t - 1), (2, 2, 2 * t)),            # ... a z face
        ("edge", (t - 1, 2, 6), (t, 3, 6)),                    # an edge pair across a tile face
        ("edge", (t - 1, t - 1, 14), (t, t, 14)),              # ... across a tile edge
        ("edge", (t - 1, t, 28), (t, t - 1, 28)),              # ... across a tile edge, the anti-diagonal (a backward y step)
        ("corner", (t - 1, 2, 10), (t, 3, 11)),                # a corner pair across a tile face
        ("corner", (t - 1, t - 1, 18), (t, t, 19)),            # ... across a tile edge
        ("corner", (t - 1, t - 1, 3 * t - 1), (t, t, 3 * t)),  # ... across a tile corner
        ("corner", (2 * t - 1, t, 30), (2 * t, t - 1, 29)),    # ... across a tile edge with backward y and z steps
    ]


PAIR_DIMS = (17, 10, 33)


@functools.lru_cache(maxsize=None)
def special_masks():
    x, y, z = np.indices((9, 10, 17))
    pairs = np.zeros(PAIR_DIMS, dtype=bool)
    for _, a, b in boundary_pairs():
        pairs[a] = pairs[b] = True
    return {"empty": np.zeros((9, 10, 17), dtype=bool), "full": np.ones((9, 10, 17), dtype=bool), "checkerboard": (x + y + z) % 2 == 0,
            "serpentine": serpentine((17, 9, 33)), "pairs": pairs}


@functools.lru_cache(maxsize=None)
def special_model(name, connectivity):
    labels = cm.label(special_masks()[name], connectivity)
    labels.setflags(write=False)
    return labels


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["empty", "full", "checkerboard", "serpentine", "pairs"])
def test_special_masks(hip_device, name, storage):
    mask = special_masks()[name]
    grid = relu_mask_grid(hip_device, mask, storage)
    for connectivity in CONNECTIVITIES:
        labels, sizes = launch(grid, 0.0, connectivity)
        want = special_model(name, connectivity)
        assert np.array_equal(labels, want) and np.array_equal(sizes, cm.sizes_of(want)), (name, connectivity)
        count = int((sizes > 0).sum())
        if name == "empty":
            assert (labels == -1).all() and count == 0 and not sizes.any()
        elif name == "full":
            assert (labels == 0).all() and count == 1 and sizes[0] == mask.size
        elif name == "checkerboard":
            assert count == (mask.sum() if connectivity == 6 else 1)
        elif name == "serpentine":  # one component whose longest chain is about a quarter of the nodes: no fixed iteration count labels it
            assert count == 1 and sizes[0] == mask.sum() and mask.sum() > mask.size // 4 and (labels[mask] == 0).all()
        else:
            kinds = [k for k, _, _ in boundary_pairs()]
            joined = {6: ("face",), 18: ("face", "edge"), 26: ("face", "edge", "corner")}[connectivity]
            for kind, a, b in boundary_pairs():
                assert (labels[a] == labels[b]) == (kind in joined), (kind, a, b, connectivity)
            assert count == sum(1 if k in joined else 2 for k in kinds)
    comps = rf.label_components(grid, 0.0, 26)
    assert comps.roots.dtype == torch.int64 and comps.sizes.dtype == torch.int64 and comps.labels.dtype == torch.int32
    assert len(comps.roots) == len(cm.ranked(special_model(name, 26))[0])


def test_a_node_at_the_threshold_is_not_occupied(hip_device):
    """sigma == threshold exactly (strict comparison): the node in the middle does not join its two neighbours"""
    tau = float(np.float32(0.3) * np.float32(3.0))
    dens = np.full((1, 1, 5), -1.0, dtype=np.float32)
    dens[0, 0, 1:4] = (1.0, 0.3, 1.0)
    for storage in STORAGES:
        grid = make_grid(hip_device, dens[..., None], 3, storage, "relu", rho=3.0)
        labels, sizes = launch(grid, tau, 26)
        assert labels.reshape(-1).tolist() == [-1, 1, -1, 3, -1] and sizes.tolist() == [0, 1, 0, 1, 0]
        below = float(np.nextafter(np.float32(tau), np.float32(0.0)))
        assert launch(grid, below, 26)[0].reshape(-1).tolist() == [-1, 1, 1, 1, -1]


def test_invariances(hip_device):
    dims, mode, p = (17, 9, 33), "relu", 0.31
    rho, tau = SETTINGS[mode]
    results = {}
    for storage in STORAGES:
        grid = make_grid(hip_device, raw_densities(dims, mode, p), 12, storage, mode, rho)
        poison_padding(grid, 1e9)
        for connectivity in CONNECTIVITIES:
            first = launch(grid, tau, connectivity)
            again = launch(grid, tau, connectivity)
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])  # two calls: identical bits
            alone, none = launch(grid, tau, connectivity, with_sizes=False)  # sizes=None works, labels unchanged
            assert none is None and np.array_equal(alone, first[0])
            assert first[0].max() < SENTINEL and first[1].max() < SENTINEL  # the sentinel prefill is gone everywhere
            results[storage, connectivity] = first
    for connectivity in CONNECTIVITIES:
        for storage in STORAGES[1:]:
            assert np.array_equal(results[storage, connectivity][0], results["reference", connectivity][0])
            assert np.array_equal(results[storage, connectivity][1], results["reference", connectivity][1])
    # the Python entry: ranked components of the same field
    grid = make_grid(hip_device, raw_densities(dims, mode, p), 12, "split", mode, rho)
    comps = rf.label_components(grid, tau, 18)
    roots, sizes = cm.ranked(model_of(dims, mode, p, 18)[0])
    assert np.array_equal(comps.labels.cpu().numpy(), model_of(dims, mode, p, 18)[0])
    assert comps.roots.tolist() == roots.tolist() and comps.sizes.tolist() == sizes.tolist() and len(set(sizes.tolist())) < len(sizes)  # (ties occur)


# --------------------------------------------------------------------------------------------
# remove_small_components
# --------------------------------------------------------------------------------------------
REMOVE_DIMS = (9, 8, 17)
FILLS = {"relu": None, "abs": None, "softplus": -3.0, "identity": -0.25}
RULES = [dict(keep_largest=1), dict(min_nodes=3), dict(min_nodes=2, keep_largest=4)]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", MODES)
def test_removal_equals_the_model_bit_for_bit(hip_device, mode, storage):
    rho, tau = SETTINGS[mode]
    connectivity = CONNECTIVITIES[(MODES.index(mode) + STORAGES.index(storage)) % 3]
    F = FEATURES[(MODES.index(mode) + STORAGES.index(storage)) % 3]
    dens = raw_densities(REMOVE_DIMS, mode, 0.2, seed=21)
    labels = cm.label(cm.occupied(dens, rho, mode, tau), connectivity)
    fill = FILLS[mode]
    for rule in RULES:
        want_dens, want_stats = cm.remove(dens, labels, mode, fill=0.0 if fill is None else fill, **rule)
        assert 0 < want_stats[1] < want_stats[0]  # something goes, something stays
        grid, expected = make_grid(hip_device, dens, F, storage, mode, rho), make_grid(hip_device, want_dens, F, storage, mode, rho)
        for g in (grid, expected):
            poison_padding(g, float("nan"))
        grid.build_occupancy(tau)
        assert grid.occupancy_current()
        stats = rf.remove_small_components(grid, tau, connectivity, fill_density=fill, **rule)
        assert stats == rf.ComponentStats(*want_stats), rule
        assert not grid.occupancy_current()  # the mask is marked stale
        # densities bit for bit; kept bits, features and the bricked padding unchanged: the whole storage equals that of the expected field
        for got, want in zip(grid.kernel_tensors(), expected.kernel_tensors()):
            assert (got is None) == (want is None) and (got is None or same_bits(got, want)), rule
        assert np.array_equal(grid.densities.detach().cpu().numpy().view(np.uint32), want_dens.view(np.uint32))
        # a second call removes nothing and changes no bit
        again = rf.remove_small_components(grid, tau, connectivity, fill_density=fill, **rule)
        assert again == rf.ComponentStats(want_stats[0] - want_stats[1], 0, want_stats[2], 0)
        for got, want in zip(grid.kernel_tensors(), expected.kernel_tensors()):
            assert got is None or same_bits(got, want)


def test_removal_argument_errors_and_foreign_modules(hip_device):
    dens = raw_densities(REMOVE_DIMS, "relu", 0.2, seed=21)
    grid = make_grid(hip_device, dens, 3, "split", "relu", 2.0)
    with pytest.raises(ValueError, match="min_nodes, keep_largest"):
        rf.remove_small_components(grid, 0.5)
    for bad in (dict(min_nodes=0), dict(keep_largest=0), dict(min_nodes=2, keep_largest=-1)):
        with pytest.raises(ValueError, match="at least 1"):
            rf.remove_small_components(grid, 0.5, **bad)
    with pytest.raises(ValueError, match="connectivity"):
        rf.remove_small_components(grid, 0.5, 8, keep_largest=1)
    with pytest.raises(ValueError, match="threshold"):
        rf.label_components(grid, -0.5)
    with pytest.raises(ValueError, match="threshold"):
        rf.label_components(grid, float("nan"))
    soft = make_grid(hip_device, raw_densities(REMOVE_DIMS, "softplus", 0.2, seed=21), 3, "split", "softplus")
    with pytest.raises(ValueError, match="fill_density"):
        rf.remove_small_components(soft, 0.7, keep_largest=1)
    with pytest.raises(ValueError, match="positive threshold"):
        rf.label_components(soft, 0.0)
    absolute = make_grid(hip_device, raw_densities(REMOVE_DIMS, "abs", 0.2, seed=21), 3, "split", "abs")
    with pytest.raises(ValueError, match="only fill is 0"):
        rf.remove_small_components(absolute, 0.5, keep_largest=1, fill_density=-1.0)
    on_cpu = make_grid(torch.device("cpu"), dens, 3, "reference", "relu", 2.0)
    with pytest.raises(ValueError, match="HIP device"):
        rf.label_components(on_cpu, 0.5)
    with pytest.raises(ValueError, match="HIP device"):
        rf.remove_small_components(on_cpu, 0.5, keep_largest=1)
    assert same_bits(grid.densities.detach().cpu(), T(dens))  # no refused call wrote anything

    class Foreign(torch.nn.Module):  # the reference VoxelGrid's attribute names, nothing else
        def __init__(self, src):
            super().__init__()
            self.densities, self.features = torch.nn.Parameter(src.densities.detach().clone()), torch.nn.Parameter(src.features.detach().clone())
            self.aabb, self._expected_density_scale = src.aabb, src.expected_density_scale
            self._density_preactivation, self._density_postactivation = torch.nn.Identity(), torch.nn.ReLU()

    foreign = Foreign(make_grid(hip_device, dens, 3, "reference", "relu", 2.0))
    labels = cm.label(cm.occupied(dens, 2.0, "relu", 0.5), 26)
    assert np.array_equal(rf.label_components(foreign, 0.5).labels.cpu().numpy(), labels)
    want_dens, want_stats = cm.remove(dens, labels, "relu", keep_largest=2)
    assert rf.remove_small_components(foreign, 0.5, keep_largest=2) == rf.ComponentStats(*want_stats)
    assert np.array_equal(foreign.densities.detach().cpu().numpy().view(np.uint32), want_dens.view(np.uint32))


# --------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------
E2E_DIMS, E2E_F, RHO = (16, 16, 16), 12, 100.0 / 3.0
VOXEL = (3.0 / 16,) * 3
SPECKS = [[(1, 1, 1)], [(14, 1, 1), (14, 1, 2)], [(1, 13, 13), (1, 13, 14), (1, 14, 13), (2, 13, 13)]]


@functools.lru_cache(maxsize=None)
def speck_field():
    """the blob of tests/test_hip_tighten.py (positive densities in the nodes [5..10]^3, negative ones everywhere else; SH degree 1)
    plus three planted specks of 1, 2 and 4 nodes away from it"""
    dens, feat = procedural_grid(E2E_DIMS, E2E_F, 51)
    dens = -dens.abs() - 0.01
    dens[5:11, 5:11, 5:11] = torch.from_numpy(hash_uniform((6, 6, 6, 1), 52, 0.02, 0.3))
    for k, speck in enumerate(SPECKS):
        for node in speck:
            dens[node] = 0.1 + 0.05 * k
    return dens, feat


def speck_grid(dev, storage="split"):
    dens, feat = speck_field()
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*VOXEL), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=False, storage=storage)


def mesh_pieces(mesh):
    """connected pieces of a triangle mesh: union-find over the faces' vertices, on the host"""
    faces = mesh.faces.cpu().numpy()
    parent = np.arange(len(mesh.vertices))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b, c in faces:
        ra, rb, rc = find(a), find(b), find(c)
        parent[ra] = parent[rb] = rc
    return len({find(v) for v in np.unique(faces)})


@pytest.mark.parametrize("storage", STORAGES)
def test_floaters_leave_the_mesh_the_box_and_nothing_else(hip_device, storage):
    grid = speck_grid(hip_device, storage)
    assert mesh_pieces(rf.extract_mesh(grid, 0.0)) == 4
    assert rf.content_bounds(grid, 0.0) == ((1, 1, 1), (14, 14, 14), 216 + 7)
    # one point in every cell, well inside it
    cells = np.indices((15, 15, 15)).reshape(3, -1).T
    points = -1.5 + (cells + 1.0 + hash_uniform(cells.shape, 61, -0.3, 0.3)) * VOXEL[0]
    points = T(points.astype(np.float32)).to(hip_device)
    with torch.no_grad():
        before = ops.grid_query(grid, points)
    comps = rf.label_components(grid)
    assert comps.sizes.tolist() == [216, 4, 2, 1] and comps.roots[0].item() == (5 * 16 + 5) * 16 + 5
    stats = rf.remove_small_components(grid, keep_largest=1)
    assert stats == rf.ComponentStats(4, 3, 216, 7)
    with torch.no_grad():
        after = ops.grid_query(grid, points)
    assert mesh_pieces(rf.extract_mesh(grid, 0.0)) == 1
    assert rf.content_bounds(grid, 0.0) == ((5, 5, 5), (10, 10, 10), 216)
    # a cell none of whose corners was removed interpolates the same bits; the cells of the specks do not
    removed = np.zeros(E2E_DIMS, dtype=bool)
    for speck in SPECKS:
        for node in speck:
            removed[node] = True
    touched = np.zeros((15, 15, 15), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                touched |= removed[dx:15 + dx, dy:15 + dy, dz:15 + dz]
    touched = T(touched.reshape(-1)).to(hip_device)
    assert same_bits(before[~touched], after[~touched]) and int((~touched).sum()) > 3000
    assert not same_bits(before[touched], after[touched])
    # only the seven nodes changed, to the fill
    dens, feat = speck_field()
    want = dens.clone()
    want[T(removed)] = 0.0
    assert same_bits(grid.densities.detach().cpu(), want) and same_bits(grid.features.detach().cpu(), feat)


# --------------------------------------------------------------------------------------------
# integration
# --------------------------------------------------------------------------------------------
def _training_scene(dev):
    cam = hotdog_like_camera()
    gd, gf = sparse_scene_grid((16, 16, 16), 3, 11)
    gt = rf.VoxelGrid((gd * 3.0).to(dev), gf.to(dev), rf.VoxelSize(*VOXEL), density_preactivation=torch.nn.Identity(),
                      density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=False)
    bounds = rf.CameraBounds(cam["near"], cam["far"])
    cfg = rf.SHVoxGridRenderConfig(32, bounds, perturb_sampled_points=False, white_bkgd=True)
    gt_model = rf.VolumetricModel(gt, rf.render_sh_voxel_grid, cfg, device=dev)
    intr = rf.CameraIntrinsics(24, 24, 33.0)
    poses = [rf.pose_spherical(90.0 * k, -30.0, cam["radius"]) for k in range(4)]
    images = torch.stack([gt_model.render(p, intr).colour.permute(2, 0, 1) for p in poses])
    pose_mat = torch.stack([torch.cat([p.rotation, p.translation], dim=1) for p in poses]).to(dev)
    return PosedImagesInMemory(images, pose_mat, intr, bounds), cfg


def _train(dev, data, cfg, **kwargs):
    torch.manual_seed(3)
    d0, f0 = procedural_grid((16, 16, 16), 3, 77)
    grid = rf.VoxelGrid(d0.to(dev), f0.to(dev), rf.VoxelSize(*VOXEL), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    history = []
    model = train_sh_vox_grid_vol_mod_with_posed_images(model, data, None, ray_batch_size=256, num_stages=2, num_iterations_per_stage=12, image_batch_cache_size=4,
                                                        learning_rate=0.03, lr_decay_steps_per_stage=10, summary_freq=100, log=lambda s: None, history=history, **kwargs)
    g = model.thre3d_repr
    return g.densities.detach().clone(), g.features.detach().clone(), history, g


def test_the_trainer_filters_per_stage_and_is_untouched_when_off(hip_device, monkeypatch):
    data, cfg = _training_scene(hip_device)
    dens_on, _, history, grid = _train(hip_device, data, cfg, component_keep_largest=1)
    rows = [h for h in history if "removed_components" in h]
    assert [r["stage"] for r in rows] == [1, 2]  # 8^3 before the upsampling, 16^3 after the last stage
    assert all(set(r) == {"stage", "components", "removed_components", "removed_nodes"} for r in rows)
    assert all(r["removed_components"] == r["components"] - 1 and r["removed_nodes"] >= r["removed_components"] for r in rows)
    assert rows[1]["removed_components"] > 0  # (a U(-1, 1) initialisation after 24 iterations: specks everywhere)
    assert len(rf.label_components(grid).roots) == 1
    # off: the parent's code path -- the same bits as a run without the arguments, and nothing of the feature is launched
    plain = _train(hip_device, data, cfg)
    calls = []
    monkeypatch.setattr(ops, "label_components_raw", lambda *a, **k: calls.append(a))
    off = _train(hip_device, data, cfg, component_keep_largest=None, component_min_nodes=None, component_threshold=0.5, component_connectivity=6)
    assert calls == []
    monkeypatch.undo()
    again = _train(hip_device, data, cfg)
    if torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1]):
        assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    else:  # (the binned adjoint orders a brick's records by atomic timing: where the parent's own runs differ in bits, so may this one)
        spread = max(float((again[i] - plain[i]).abs().max()) for i in (0, 1))
        assert max(float((off[i] - plain[i]).abs().max()) for i in (0, 1)) <= 4 * spread
    assert not any("removed_components" in h for h in off[2]) and len(off[2]) == len(plain[2])
    assert not torch.equal(dens_on, plain[0])


def _speck_checkpoint(dev, tmp_path):
    cam = hotdog_like_camera()
    cfg = rf.SHVoxGridRenderConfig(32, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False)
    grid = speck_grid(dev, "reference")
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    src = tmp_path / "model.pth"
    torch.save(model.get_save_info(extra_info={"note": "kept"}), src)
    return grid, src


def _run_script(*args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, *args], cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)


def test_cli_clean_round_trip(hip_device, tmp_path):
    """scripts/clean_sh_based_voxel_grid.py on a written checkpoint gives what remove_small_components gives in process"""
    grid, src = _speck_checkpoint(hip_device, tmp_path)
    dst = tmp_path / "cleaned.pth"
    r = _run_script("scripts/clean_sh_based_voxel_grid.py", "-i", str(src), "-o", str(dst), "--threshold", "0", "--keep_largest", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "before: 4 components, 223 occupied nodes" in r.stdout and "after: 1 components, 216 occupied nodes" in r.stdout
    assert "removed components: 3 of 4  removed nodes: 7  kept nodes: 216" in r.stdout and "#0: 216 nodes, first node (5, 5, 5)" in r.stdout
    assert rf.remove_small_components(grid, keep_largest=1) == rf.ComponentStats(4, 3, 216, 7)
    loaded, extra = rf.create_volumetric_model_from_saved_model(dst, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    got = loaded.thre3d_repr
    assert extra == {"note": "kept"} and got.grid_dims == E2E_DIMS
    assert same_bits(got.densities.detach(), grid.densities.detach()) and same_bits(got.features.detach(), grid.features.detach())
    # neither rule: a usage error, nothing written
    r = _run_script("scripts/clean_sh_based_voxel_grid.py", "-i", str(src), "-o", str(tmp_path / "none.pth"))
    assert r.returncode != 0 and "--keep_largest" in r.stderr and not (tmp_path / "none.pth").exists()


def test_cli_mesh_flags(hip_device, tmp_path):
    """scripts/extract_mesh_from_sh_based_voxel_grid.py --keep_largest / --min_component_nodes drop the specks' shells without
    touching the checkpoint"""
    grid, src = _speck_checkpoint(hip_device, tmp_path)
    mesh = ("scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", str(src), "--iso_level", "0", "--subdivisions", "1")
    whole = len(rf.extract_mesh(grid, 0.0, subdivisions=1).faces)
    r = _run_script(*mesh, "-o", str(tmp_path / "one.ply"), "--keep_largest", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "connected components above the iso level: 4, removed 3 (7 nodes; 216 kept)" in r.stdout
    rf.remove_small_components(grid, keep_largest=1)
    one = read_ply(str(tmp_path / "one.ply"))
    assert len(one[3]) == len(rf.extract_mesh(grid, 0.0, subdivisions=1).faces) < whole
    r = _run_script(*mesh, "-o", str(tmp_path / "few.ply"), "--min_component_nodes", "3")
    assert r.returncode == 0 and "connected components above the iso level: 4, removed 2 (3 nodes; 220 kept)" in r.stdout
    assert len(one[3]) < len(read_ply(str(tmp_path / "few.ply"))[3]) < whole
    r = _run_script("scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", str(src), "-o", str(tmp_path / "bad.ply"), "--iso_level", "-1", "--keep_largest", "1")
    assert r.returncode != 0 and "non-negative --iso_level" in r.stderr and not (tmp_path / "bad.ply").exists()
    # the checkpoint the script read is as it was
    reread, _ = rf.create_volumetric_model_from_saved_model(src, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    assert same_bits(reread.thre3d_repr.densities.detach().cpu(), speck_field()[0])
