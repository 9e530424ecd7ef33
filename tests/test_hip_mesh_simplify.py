"""GPU: rf.simplify_mesh (rf_mesh_cluster_keys / rf_mesh_cluster_vertices, csrc/mesh_simplify_kernels.hip) against the numpy
float64 model of tests/mesh_simplify_model.py.  Topology -- keys, cluster_of_vertex, faces, counts -- matches EXACTLY; positions and
attributes match within the bound derived in docs/mesh_simplify_errors.md (computed by the model, per coordinate); two runs give
identical bits.  The shapes are the smallest that reach each path of the kernel: segment lengths around the 16-lane group, the
64-lane wave and the kLongSegment hand-over, cluster counts around a group, a wave and a workgroup."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_simplify_model as mm
from tests.helpers import REPO_ROOT, hash_uniform, procedural_grid
from thr3ed_atom_amd import _lib, mesh_simplify as ms, ops
from thr3ed_atom_amd.mesh import read_ply, write_ply

pytestmark = pytest.mark.gpu

STORAGES = ["reference", "split", "bricked"]
LONG = _lib.MESH_LONG_SEGMENT
# corner records of a fan's centre vertex (which is alone in its cell: one member record on top)
FAN_SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 129, LONG - 2, LONG - 1, 1500]


def T(a):
    return torch.from_numpy(np.array(a))  # (a copy: the shared inputs are read-only)


def merge(parts):
    """the disjoint union of (vertices, faces) meshes"""
    vertices, faces, base = [], [], 0
    for v, f in parts:
        vertices.append(v)
        faces.append(f + base)
        base += len(v)
    return np.concatenate(vertices).astype(np.float32), np.concatenate(faces).astype(np.int64)


@functools.lru_cache(maxsize=None)
def fan_field():
    """fans of FAN_SIZES triangles, 10 apart, around negative and positive coordinates, radius 2.5 against cells of 1: every centre
    vertex is alone in its cell (k corner records, 1 member), the rims share cells in varying numbers; the last two fans' centres sit in
    consecutive cells of one column; plus three vertices that no face uses (0 corner records)"""
    parts = []
    for i, k in enumerate(FAN_SIZES):
        centre = (-31.3 + 10.0 * (i % 6), -4.2 + 10.0 * (i // 6), 0.37 * i - 2.0)
        if i == len(FAN_SIZES) - 1:
            before = (-31.3 + 10.0 * ((i - 1) % 6), -4.2 + 10.0 * ((i - 1) // 6), 0.37 * (i - 1) - 2.0)
            centre = (before[0], before[1], before[2] + 1.0)
        parts.append(mm.triangle_fan(k, centre=centre, radius=2.5))
    v, f = merge(parts)
    v = np.concatenate([v, np.asarray([[3.3, 17.7, 1.1], [-20.5, 15.5, -0.5], [-33.75, -6.6, -2.2]], dtype=np.float32)])
    colours, normals = hash_uniform((len(v), 3), 3, 0.0, 1.0), hash_uniform((len(v), 3), 4)
    for a in (v, f, colours, normals):
        a.setflags(write=False)
    return v, f, colours, normals


@functools.lru_cache(maxsize=None)
def sphere_in_a_cell():
    """a 16 384-face sphere inside the cell [0, 1)^3 of a lattice at the origin, tied to three vertices in other cells by two faces:
    49 153 corner and 8 194 member records in one cluster"""
    v, f, n = mm.uv_sphere(65, 128, radius=0.4, centre=(0.5, 0.5, 0.5))
    extra = np.asarray([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]], dtype=np.float32)
    base = len(v)
    f = np.concatenate([f, [[0, base, base + 1], [base, base + 2, base + 1]]])
    n = 0.5 * n + np.asarray([0.3, -0.2, 0.6], dtype=np.float32)  # (the unit normals of a sphere sum to nothing: no direction to compare)
    v, n = np.concatenate([v, extra]), np.concatenate([n, [[1, 0, 0], [0, 1, 0], [0, 0, 1]]]).astype(np.float32)
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


@functools.lru_cache(maxsize=None)
def small_sphere():
    v, f, n = mm.uv_sphere(24, 32, radius=0.9, centre=(0.11, -0.23, 0.05))
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


def strip(count):
    """a triangle strip of `count` vertices 1.7 apart with every vertex in a cell of its own (cells of 1): `count` clusters"""
    i = np.arange(count)
    v = np.stack([1.7 * i - 0.6 * count, 1.9 * (i % 2) + 0.05 * i, 0.3 * np.sin(i)], -1).astype(np.float32)
    f = np.asarray([(j, j + 1, j + 2) if j % 2 == 0 else (j + 1, j, j + 2) for j in range(count - 2)], dtype=np.int64).reshape(-1, 3)
    return v, f


@functools.lru_cache(maxsize=None)
def model_of(name, h, placement="quadric", regularisation=1e-3, origin=None, attributes=True):
    """the model of a named case: computed once, shared, never written"""
    if name == "fans":
        v, f, c, n = fan_field()
    elif name == "sphere_in_a_cell":
        (v, f, n), c = sphere_in_a_cell(), None
    else:
        (v, f, n), c = small_sphere(), np.abs(small_sphere()[2])
    if not attributes:
        c = n = None
    return mm.simplify(v, f, h, placement=placement, regularisation=regularisation, origin=origin, colours=c, normals=n)


def gpu_mesh(dev, v, f, c=None, n=None):
    on = lambda a: None if a is None else T(a).to(dev)
    return rf.Mesh(on(v), on(f), on(c), on(n))


def host(t):
    return None if t is None else t.cpu().numpy()


def check(model, out, stats):
    counts = (stats.clusters, stats.vertices, stats.input_faces, stats.collapsed_faces, stats.merged_duplicates, stats.faces)
    problems = mm.compare(model, host(out.vertices), host(out.faces), host(out.colours), host(out.normals), host(stats.cluster_of_vertex), counts)
    assert problems == [], problems
    assert stats.cell_size == model.cell_size and stats.vertices == len(out.vertices) and stats.faces == len(out.faces)
    print(f"largest |hip - model| / bound over the coordinates: {mm.error_ratio(model, host(out.vertices)):.3g}")


def every_cluster(mesh, h, origin, placement, regularisation):
    """the representatives of ALL clusters, through the stages simplify_mesh is made of"""
    lattice = ms._lattice(ms._host_bounds(mesh), h, origin)
    cluster_keys, cluster = ms._cluster_keys(mesh.vertices, lattice)
    lists = ms._cluster_lists(cluster, mesh.faces, cluster_keys.numel())
    return cluster_keys, ms._cluster_vertices(mesh, lists, cluster_keys, lattice, placement, regularisation)


# ------------------------------------------------------------------------------------------------------ segment lengths

def test_the_fan_field_holds_every_segment_length():
    model = model_of("fans", 1.0)
    lengths = set(model.corner_records.tolist())
    assert {0, *FAN_SIZES} <= lengths
    records = (model.corner_records + model.member_records).tolist()
    assert LONG - 1 in records and LONG in records and 1501 in records  # both sides of the whole-wave hand-over
    # two whole-wave clusters that are neighbours in key order inside one wave's four, and waves with one, and with none
    heavy = model.corner_records + model.member_records >= LONG
    per_wave = np.add.reduceat(heavy.astype(np.int64), np.arange(0, model.clusters, 64 // _lib.MESH_CLUSTER_GROUP))
    assert {0, 1} <= set(per_wave.tolist()) and per_wave.max() >= 2
    assert model.clusters > 2 * _lib.MESH_CLUSTERS_PER_BLOCK and model.clusters % _lib.MESH_CLUSTERS_PER_BLOCK != 0
    assert (model.member_records > 1).any() and (np.asarray(fan_field()[0]) < 0).any()


@pytest.mark.parametrize("placement,regularisation,attributes", [("quadric", 1e-3, True), ("mean", 1e-3, True), ("quadric", 1e-6, False), ("quadric", 1.0, True)])
def test_fans_match_the_model(hip_device, placement, regularisation, attributes):
    v, f, c, n = fan_field()
    mesh = gpu_mesh(hip_device, v, f, c if attributes else None, n if attributes else None)
    model = model_of("fans", 1.0, placement, regularisation, None, attributes)
    out, stats = rf.simplify_mesh(mesh, 1.0, placement=placement, regularisation=regularisation, return_stats=True)
    check(model, out, stats)
    assert (out.colours is None) == (not attributes) and (out.normals is None) == (not attributes)
    # the clusters that no face uses, too
    cluster_keys, (cv, cc, cn) = every_cluster(mesh, 1.0, None, placement, regularisation)
    assert np.array_equal(host(cluster_keys), model.cluster_keys)
    assert mm.compare_clusters(model, host(cv), host(cc), host(cn)) == []
    # bitwise repeatable
    again, stats2 = rf.simplify_mesh(mesh, 1.0, placement=placement, regularisation=regularisation, return_stats=True)
    for a, b in zip(out, again):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(stats.cluster_of_vertex, stats2.cluster_of_vertex) and stats[:7] == stats2[:7]


@pytest.mark.parametrize("placement,regularisation", [("quadric", 1e-3), ("quadric", 1e-6), ("mean", 1e-3)])
def test_a_whole_sphere_in_one_cell(hip_device, placement, regularisation):
    v, f, n = sphere_in_a_cell()
    model = model_of("sphere_in_a_cell", 1.0, placement, regularisation, (0.0, 0.0, 0.0))
    assert model.corner_records.max() == 3 * 16384 + 1 and model.member_records.max() == 8194 and model.clusters == 4
    mesh = gpu_mesh(hip_device, v, f, None, n)
    out, stats = rf.simplify_mesh(mesh, 1.0, origin=(0.0, 0.0, 0.0), placement=placement, regularisation=regularisation, return_stats=True)
    check(model, out, stats)
    assert stats.faces == 2 and stats.collapsed_faces == 16384
    again = rf.simplify_mesh(mesh, 1.0, origin=(0.0, 0.0, 0.0), placement=placement, regularisation=regularisation)
    assert torch.equal(out.vertices, again.vertices) and torch.equal(out.normals, again.normals)


# ------------------------------------------------------------------------------------------------------ cluster counts

@pytest.mark.parametrize("count", [3, 4, 6, 16, 17, 64, 65, 257])
def test_cluster_counts_around_a_group_a_wave_and_a_workgroup(hip_device, count):
    v, f = strip(count)
    model = mm.simplify(v, f, 1.0)
    assert model.clusters == count and len(model.vertices) == count and len(model.faces) == count - 2
    out, stats = rf.simplify_mesh(gpu_mesh(hip_device, v, f), 1.0, return_stats=True)
    check(model, out, stats)
    assert out.colours is None and out.normals is None


def test_one_cluster_and_everything_collapsing(hip_device):
    v, f, n = small_sphere()
    n = (0.5 * n + np.asarray([0.3, -0.2, 0.6])).astype(np.float32)  # (the unit normals of a sphere sum to nothing: no direction to compare)
    mesh = gpu_mesh(hip_device, v, f, np.abs(n), n)
    model = mm.simplify(v, f, 4.0, colours=np.abs(n), normals=n)
    assert model.clusters == 1 and len(model.faces) == 0
    out, stats = rf.simplify_mesh(mesh, 4.0, return_stats=True)
    check(model, out, stats)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.faces.dtype == torch.int64 and out.colours.shape == (0, 3)
    assert stats.clusters == 1 and stats.collapsed_faces == len(f) and bool((stats.cluster_of_vertex == -1).all())
    cluster_keys, (cv, cc, cn) = every_cluster(mesh, 4.0, None, "quadric", 1e-3)
    assert cluster_keys.tolist() == [0] and mm.compare_clusters(model, host(cv), host(cc), host(cn)) == []


def test_empty_inputs(hip_device):
    v, f, n = small_sphere()
    none = gpu_mesh(hip_device, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32), None)
    out, stats = rf.simplify_mesh(none, 0.5, return_stats=True)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.colours.shape == (0, 3) and out.normals is None
    assert stats[:7] == (0.5, 0, 0, 0, 0, 0, 0) and stats.cluster_of_vertex.shape == (0,)
    no_faces = gpu_mesh(hip_device, v, np.zeros((0, 3), np.int64))
    out, stats = rf.simplify_mesh(no_faces, target_faces=10, return_stats=True)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and stats.cluster_of_vertex.tolist() == [-1] * len(v)


# ------------------------------------------------------------------------------------------------------ the sphere: origins, cells, targets

@pytest.mark.parametrize("h,origin", [(0.3, None), (0.083, None), (0.3, (-1.0, -1.5, -0.875)), (0.17, (-0.79, -1.13, -0.85))])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_sphere_with_default_and_explicit_origins(hip_device, h, origin, placement):
    v, f, n = small_sphere()
    model = model_of("sphere", h, placement, 1e-3, origin)
    out, stats = rf.simplify_mesh(gpu_mesh(hip_device, v, f, np.abs(n), n), h, origin=origin, placement=placement, return_stats=True)
    check(model, out, stats)
    assert mm.directed_edge_balance(host(out.faces)) or stats.merged_duplicates > 0


def test_keys_match_the_model(hip_device):
    v, f, _, _ = fan_field()
    for h, origin in ((1.0, None), (0.37, (-40.0, -10.0, -5.0))):
        lat = mm.lattice_of(v, h, origin)
        vertices = T(v).to(hip_device)
        keys = torch.empty(len(v), dtype=torch.int64, device=hip_device)
        status = torch.zeros(1, dtype=torch.int32, device=hip_device)
        ops.mesh_cluster_keys_raw(vertices, lat.origin, lat.r, lat.cells, keys, status)
        assert np.array_equal(host(keys), lat.keys) and status.item() == 0
    # a vertex below the origin, beyond the cells or not finite: key -1 and the status word, in the same pass
    bad = v[:64].copy()
    bad[3, 1], bad[17, 0], bad[40, 2], bad[41, 0] = -1e3, np.nan, np.inf, 1e3
    lat = mm.lattice_of(v[:64], 1.0)
    keys = torch.empty(64, dtype=torch.int64, device=hip_device)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    ops.mesh_cluster_keys_raw(T(bad).to(hip_device), lat.origin, lat.r, lat.cells, keys, status)
    expected = lat.keys.copy()
    expected[[3, 17, 40, 41]] = -1
    assert np.array_equal(host(keys), expected) and status.item() == 1


@pytest.mark.parametrize("target", [0, 40, 500, 100000])
def test_target_faces_on_the_sphere(hip_device, target):
    v, f, n = small_sphere()
    model = mm.simplify(v, f, target_faces=target, normals=n)
    out, stats = rf.simplify_mesh(gpu_mesh(hip_device, v, f, None, n), target_faces=target, return_stats=True)
    assert stats.faces <= target
    check(model, out, stats)


# ------------------------------------------------------------------------------------------------------ extract_mesh -> simplify_mesh

@pytest.mark.parametrize("dims,subdivisions", [((12, 12, 12), 1), ((12, 12, 12), 2), ((9, 8, 17), 1), ((9, 8, 17), 2)])
def test_extracted_meshes_simplify_to_the_same_bits_on_every_storage(hip_device, dims, subdivisions):
    dens, feat = procedural_grid(dims, 12, seed=21)
    voxel = (0.2, 0.25, 0.2)
    results = {}
    for storage in STORAGES:
        grid = rf.VoxelGrid(dens.clone().to(hip_device), feat.clone().to(hip_device), rf.VoxelSize(*voxel), density_preactivation=torch.nn.Identity(),
                            density_postactivation=torch.nn.ReLU(), expected_density_scale=3.0, storage=storage)
        mesh = rf.extract_mesh(grid, 0.4, subdivisions=subdivisions)
        assert len(mesh.faces) > 100
        origin = [r[0] - 2 * 0.2 for r in grid.aabb]  # below the guard layer of the extraction
        for voxels in (1.5, 3.0):
            out, stats = rf.simplify_mesh(mesh, voxels * min(voxel), origin=origin, return_stats=True)
            assert 0 < stats.faces < len(mesh.faces)
            if storage == STORAGES[0]:
                model = mm.simplify(host(mesh.vertices), host(mesh.faces), voxels * min(voxel), origin=origin, colours=host(mesh.colours), normals=host(mesh.normals))
                check(model, out, stats)
                results[voxels] = (out, stats)
            else:
                first, first_stats = results[voxels]
                assert all(torch.equal(a, b) for a, b in zip(out, first)) and torch.equal(stats.cluster_of_vertex, first_stats.cluster_of_vertex)


# ------------------------------------------------------------------------------------------------------ errors

def test_bad_arguments_raise(hip_device):
    v, f, n = small_sphere()
    mesh = gpu_mesh(hip_device, v, f, None, n)
    with pytest.raises(ValueError, match="HIP device"):
        rf.simplify_mesh(rf.Mesh(T(v), T(f), None, None), 0.3)
    with pytest.raises(ValueError, match="below the origin"):
        rf.simplify_mesh(mesh, 0.3, origin=(0.0, -2.0, -2.0))
    with pytest.raises(ValueError, match="2\\^20"):
        rf.simplify_mesh(mesh, 1e-7)
    poisoned = v.copy()
    poisoned[5, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        rf.simplify_mesh(gpu_mesh(hip_device, poisoned, f), 0.3)
    poisoned[5, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        rf.simplify_mesh(gpu_mesh(hip_device, poisoned, f), 0.3)
    for wrong in (f + 1, f - 1):
        with pytest.raises(ValueError, match="faces index outside"):
            rf.simplify_mesh(gpu_mesh(hip_device, v, wrong), 0.3)
    for kwargs in ({}, {"cell_size": 0.3, "target_faces": 10}, {"cell_size": 0.0}, {"cell_size": -1.0}, {"cell_size": float("nan")}, {"target_faces": -1},
                   {"cell_size": 0.3, "placement": "median"}, {"cell_size": 0.3, "regularisation": 1e-7}, {"cell_size": 0.3, "regularisation": 2.0},
                   {"cell_size": 0.3, "origin": (0.0, float("nan"), 0.0)}):
        with pytest.raises(ValueError):
            rf.simplify_mesh(mesh, **kwargs)
    flat = gpu_mesh(hip_device, np.zeros((3, 3), np.float32), np.asarray([[0, 1, 2]]))
    with pytest.raises(ValueError, match="positive extent"):
        rf.simplify_mesh(flat, target_faces=5)
    with pytest.raises(ValueError):
        rf.simplify_mesh(rf.Mesh(mesh.vertices.double(), mesh.faces, None, None), 0.3)
    with pytest.raises(ValueError):
        rf.simplify_mesh(rf.Mesh(mesh.vertices, mesh.faces, mesh.vertices[:5], None), 0.3)
    # int32 faces are taken
    out = rf.simplify_mesh(rf.Mesh(mesh.vertices, mesh.faces.to(torch.int32), None, None), 0.3)
    assert np.array_equal(host(out.faces), model_of("sphere", 0.3).faces)


# ------------------------------------------------------------------------------------------------------ the scripts

def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    return subprocess.run([sys.executable] + args, cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_simplify_mesh_script_round_trip(hip_device, tmp_path):
    v, f, n = small_sphere()
    source, out_path = tmp_path / "sphere.ply", tmp_path / "small.ply"
    write_ply(rf.Mesh(T(v), T(f), T(np.abs(n)), T(n)), str(source))
    pv, pn, pc, pf = read_ply(str(source))  # what the script reads: uint8 colours
    r = _run(["scripts/simplify_mesh.py", "-i", str(source), "-o", str(out_path), "--cell_size", "0.3"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"T = {len(f)} -> " in r.stdout
    model = mm.simplify(pv, pf, 0.3, colours=pc.astype(np.float32) / np.float32(255.0), normals=pn)
    ov, on, oc, of = read_ply(str(out_path))
    assert mm.compare(model, ov, of, None if model.colours is None else model.colours, on) == []
    assert np.abs(oc.astype(np.float64) - 255.0 * model.colours64).max() <= 1.0 + 1e-3  # write_ply truncates to uint8
    r = _run(["scripts/simplify_mesh.py", "-i", str(source), "-o", str(out_path), "--target_faces", "300", "--placement", "mean"])
    assert r.returncode == 0, r.stderr[-2000:]
    model = mm.simplify(pv, pf, target_faces=300, placement="mean", normals=pn)
    ov, on, oc, of = read_ply(str(out_path))
    assert len(of) <= 300 and mm.compare(model, ov, of, None, on) == []
    r = _run(["scripts/simplify_mesh.py", "-i", str(source), "-o", str(out_path)])
    assert r.returncode != 0 and "cell_size" in r.stderr


def test_extraction_script_simplifies_on_request(hip_device, tmp_path):
    checkpoint = os.path.join(REPO_ROOT, "tests", "golden", "reference_checkpoint.pth")
    small = tmp_path / "small.ply"
    r = _run(["scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", checkpoint, "-o", str(small), "--simplify_voxels", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.search(r"simplified \(quadric, cell size [0-9.e+-]+\): V = (\d+) -> (\d+), T = (\d+) -> (\d+) in ", r.stdout)
    assert found, r.stdout
    full_vertices, vertices, full_faces, faces = (int(g) for g in found.groups())
    assert f"V = {full_vertices}, T = {full_faces} in" in r.stdout  # the extraction's own line still reports the extracted mesh
    sv, _, _, sf = read_ply(str(small))
    assert 0 < len(sf) == faces < full_faces and len(sv) == vertices and np.isfinite(sv).all() and sf.max() == len(sv) - 1
    r = _run(["scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", checkpoint, "-o", str(small), "--target_faces", "200"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert 0 < len(read_ply(str(small))[3]) <= 200
