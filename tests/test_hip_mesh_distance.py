"""rf.MeshDistanceGrid / closest_points_on_mesh / sample_mesh_surface / mesh_distance on the GPU against the numpy model of
tests/mesh_distance_model.py: every query against the float64 brute force within the derived bound B(p, mesh) of
docs/mesh_distance_errors.md, bit-identical results for every cell size, exact closed forms, ties, max_distance, degenerate faces,
bad input, the sampler and the reductions."""
import math

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_distance_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32
SOUP_H = f32(0.25)


def dev():
    return torch.device("cuda:0")


def mesh_of(v, f):
    return rf.Mesh(torch.from_numpy(np.ascontiguousarray(v, dtype=f32)).to(dev()), torch.from_numpy(np.ascontiguousarray(f, dtype=np.int64)).to(dev()), None, None)


def on_device(points):
    return torch.from_numpy(np.array(points, dtype=f32)).to(dev())  # (a copy: the references are read-only)


def host(result):
    return tuple(t.cpu().numpy() for t in result)


def stretched_cube():
    v, f = M.cube()
    return (v * np.array([4.1, 1.1, 0.6], dtype=f32)).astype(f32), f


TRIANGLE = (np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=f32), np.array([[0, 1, 2]], dtype=np.int64))
# name: (mesh, the cell sizes (None: the default) with the lattice each must give (None: not pinned), the number of queries)
CASES = {
    "triangle": (TRIANGLE, ((None, None), (f32(1.0), (5, 5, 1))), 200),
    "cube-1": (M.cube(), ((f32(2.0), (1, 1, 1)),), 1),
    "cube-63": (M.cube(), ((f32(0.3), (4, 4, 4)),), 63),
    "cube-64": (M.cube(), ((f32(0.3), (4, 4, 4)),), 64),
    "cube-65": (M.cube(), ((f32(0.3), (4, 4, 4)),), 65),
    "cube": (M.cube(), ((f32(0.3), (4, 4, 4)), (f32(2.0), (1, 1, 1)), (None, None), (f32(0.03125), (33, 33, 33))), 4097),
    "stretched": (stretched_cube(), ((f32(0.25), (17, 5, 3)), (f32(8.0), (1, 1, 1)), (None, None)), 4097),
    "icosphere": (M.icosphere(), ((None, None), (f32(4.0), (1, 1, 1)), (f32(0.07), None)), 1500),
    "perturbed": ((M.perturbed(M.icosphere()[0]), M.icosphere()[1]), ((None, None), (f32(4.0), (1, 1, 1)), (f32(0.5), None)), 1500),
    "soup": (M.soup(SOUP_H), ((SOUP_H, (9, 9, 9)), (f32(4.0), (1, 1, 1)), (None, None), (f32(0.09), None)), 1500),
}
_cache = {}


def reference(name):
    """(queries, d64 [N, T], B [N], the GPU result on the first lattice) of a case, computed once and left unchanged"""
    if name not in _cache:
        (v, f), sizes, count = CASES[name]
        q = M.queries(v, f, count, seed=len(name) + count, h=sizes[0][0])
        d64 = np.sqrt(M.face_distances2(q, v, f))
        grid = rf.MeshDistanceGrid(mesh_of(v, f), sizes[0][0])
        if sizes[0][1] is not None:
            assert tuple(grid.lattice.cells) == sizes[0][1]
        got, rings = grid.closest(on_device(q), return_rings=True)
        _cache[name] = (q, d64, M.bound(q, v, f, d64), host(got), rings.cpu().numpy())
        for a in _cache[name][:3]:
            a.setflags(write=False)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_query_against_the_float64_brute_force(name):
    (v, f), _, count = CASES[name]
    q, d64, B, (d, face, point), rings = reference(name)
    assert d.shape == (count,) and d.dtype == f32 and face.dtype == np.int64 and point.shape == (count, 3) and point.dtype == f32
    assert np.isfinite(d).all() and np.isfinite(point).all() and (face >= 0).all() and (face < len(f)).all()
    exact = d64.min(axis=1)
    v64, p64 = v.astype(np.float64), point.astype(np.float64)
    errors = {
        "distance": np.abs(d.astype(np.float64) - exact),
        "face": d64[np.arange(count), face] - exact,
        "point to query": np.abs(np.linalg.norm(q.astype(np.float64) - p64, axis=1) - d.astype(np.float64)),
        "point to face": np.sqrt(M.closest_on_face(p64, v64[f[face, 0]], v64[f[face, 1]], v64[f[face, 2]])[0]),
    }
    worst = {k: float((e / B).max()) for k, e in errors.items()}
    print(f"{name}: worst error / B {worst}, largest B {B.max():.3g}, largest error {max(float(e.max()) for e in errors.values()):.3g}, rings up to {rings.max()}")
    for k, e in errors.items():
        assert (e <= B).all(), (name, k, worst[k])
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", ["cube", "stretched", "icosphere", "perturbed", "soup"])
def test_the_result_does_not_depend_on_the_cell_size(name):
    (v, f), sizes, _ = CASES[name]
    q, _, _, (d, face, point), rings = reference(name)
    points = on_device(q)
    seen = []
    for h, cells in sizes:
        grid = rf.MeshDistanceGrid(mesh_of(v, f), h)
        if cells is not None:
            assert tuple(grid.lattice.cells) == cells, (name, h)
        got = host(grid.closest(points))
        assert got[0].tobytes() == d.tobytes() and (got[1] == face).all() and got[2].tobytes() == point.tobytes(), (name, h)
        seen.append(tuple(grid.lattice.cells))
    assert (1, 1, 1) in seen and max(int(np.prod(c)) for c in seen) > 100  # the brute force and a lattice that really walks
    again = host(rf.closest_points_on_mesh(points, mesh_of(v, f), cell_size=sizes[0][0]))  # two calls, the one-shot form
    assert again[0].tobytes() == d.tobytes() and (again[1] == face).all() and again[2].tobytes() == point.tobytes()


@pytest.mark.parametrize("name", ["cube", "soup"])
def test_the_kernel_restates_the_float32_model(name):
    (v, f), _, _ = CASES[name]
    q, _, _, (d, face, point), _ = reference(name)
    q = q[:600]
    model = M.brute_force(q, v, f, np.float32)
    assert model[0].tobytes() == d[:600].tobytes() and (model[1] == face[:600]).all() and model[2].tobytes() == point[:600].tobytes()


def test_exact_closed_forms_and_ties():
    v, f = TRIANGLE
    queries = np.array([[1, 1, 3], [-3, -4, 0], [1, -2, 0], [3, 0.5, -3], [4, 4, 0]], dtype=f32)
    for h in (None, 0.5, 100.0):
        d, face, point = host(rf.closest_points_on_mesh(on_device(queries), mesh_of(v, f), cell_size=h))
        assert d.tolist() == [3.0, 5.0, 2.0, 3.0, float(np.sqrt(f32(8.0)))] and (face == 0).all()
        assert point.tolist() == [[1, 1, 0], [0, 0, 0], [1, 0, 0], [3, 0.5, 0], [2, 2, 0]]
    # identical faces: the lower index, wherever the pair stands and whatever the lattice
    other = np.array([[10, 10, 10], [11, 10, 10], [10, 11, 10]], dtype=f32)
    for faces, winner in (([[0, 1, 2], [0, 1, 2]], 0), ([[3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 1, 2]], 1), ([[0, 1, 2], [3, 4, 5], [0, 1, 2]], 0)):
        for h in (None, 0.7, 100.0):
            d, face, _ = host(rf.closest_points_on_mesh(on_device(queries), mesh_of(np.concatenate([v, other]), np.array(faces)), cell_size=h))
            assert (face == winner).all() and d[0] == 3.0


def test_max_distance():
    v, f = TRIANGLE
    grid = rf.MeshDistanceGrid(mesh_of(v, f), 0.5)
    p = on_device(np.array([[1, 1, 3]], dtype=f32))
    d, face, point = host(grid.closest(p, max_distance=3.0))  # exactly at the limit: found
    assert d[0] == 3.0 and face[0] == 0 and point[0].tolist() == [1, 1, 0]
    for limit in (float(np.nextafter(f32(3.0), f32(0.0))), 1.0, 0.0):
        d, face, point = host(grid.closest(p, max_distance=limit))
        assert d[0] == np.inf and face[0] == -1 and np.isnan(point[0]).all()
    (v, f), sizes, _ = CASES["soup"]
    q, _, _, (d, face, point), _ = reference("soup")
    limit = float(np.median(d))
    for h, _ in sizes[:2]:
        cut = host(rf.MeshDistanceGrid(mesh_of(v, f), h).closest(on_device(q), max_distance=limit))
        near = d <= f32(limit)
        assert near.any() and (~near).any()
        assert cut[0][near].tobytes() == d[near].tobytes() and (cut[1][near] == face[near]).all() and cut[2][near].tobytes() == point[near].tobytes()
        assert np.isinf(cut[0][~near]).all() and (cut[1][~near] == -1).all() and np.isnan(cut[2][~near]).all()


def test_degenerate_faces_are_their_segments_or_their_point():
    v, f = M.soup(SOUP_H)
    tris = v[f[2000:2020]].astype(np.float64)  # 7 with a repeated vertex, 7 collinear, 6 points
    assert (tris[:7, 0] == tris[:7, 1]).all() and (tris[14:, 0] == tris[14:, 2]).all() and (tris[7:14, 2] - tris[7:14, 0] == 2 * (tris[7:14, 1] - tris[7:14, 0])).all()
    vd, fd = v[f[2000:2020]].reshape(-1, 3), np.arange(60).reshape(20, 3)
    q = M.queries(vd, fd, 500, seed=9, h=f32(0.1))
    p = q.astype(np.float64)[:, None, :]
    a, b = tris[None, :, 0], tris[None, :, 2]  # the segment from the first to the last corner is the whole face in all three kinds
    e = b - a
    l = (e * e).sum(-1)
    t = np.clip(np.where(l > 0, ((p - a) * e).sum(-1) / np.where(l > 0, l, 1), 0), 0, 1)
    closed = np.sqrt(((p - (a + t[..., None] * e)) ** 2).sum(-1))  # [N, 20]
    B = M.bound(q, vd, fd, closed)
    for h in (None, 0.1, 100.0):
        d, face, point = host(rf.closest_points_on_mesh(on_device(q), mesh_of(vd, fd), cell_size=h))
        assert np.isfinite(d).all() and np.isfinite(point).all() and (face >= 0).all()
        assert (np.abs(d - closed.min(axis=1)) <= B).all() and (closed[np.arange(500), face] <= closed.min(axis=1) + B).all()


def test_bad_input():
    v, f = M.cube()
    good = mesh_of(v, f)
    p = on_device(np.zeros((4, 3)))
    for bad in (np.array([[0, 1, 8]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError):
            rf.MeshDistanceGrid(mesh_of(v, np.concatenate([f, bad])))
    for value in (np.nan, np.inf):
        broken = v.copy()
        broken[3, 1] = value
        with pytest.raises(ValueError):
            rf.closest_points_on_mesh(p, mesh_of(broken, f))
        points = np.zeros((70, 3), dtype=f32)
        points[67, 2] = value
        with pytest.raises(ValueError):
            rf.closest_points_on_mesh(on_device(points), good)
    with pytest.raises(ValueError):
        rf.MeshDistanceGrid(rf.Mesh(torch.from_numpy(v), torch.from_numpy(f), None, None))
    with pytest.raises(ValueError):
        rf.closest_points_on_mesh(torch.zeros(4, 3), good)
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rf.MeshDistanceGrid(good, cell_size=h)
    with pytest.raises(ValueError):
        rf.MeshDistanceGrid(good, cell_size=1e-5)  # 100 001 cells along an axis
    for limit in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            rf.closest_points_on_mesh(p, good, max_distance=limit)
    with pytest.raises(ValueError):
        rf.closest_points_on_mesh(p.double(), good)
    with pytest.raises(ValueError):
        rf.sample_mesh_surface(rf.Mesh(good.vertices, good.faces[:, [0, 0, 0]], None, None), 10)  # no area
    with pytest.raises(ValueError):
        rf.mesh_distance(good, good, samples=0)
    # the kernel's own status word: a face index that goes bad after the lists were built
    grid = rf.MeshDistanceGrid(good, 0.3)
    grid.faces = grid.faces.clone()
    grid.faces[5, 1] = 8
    with pytest.raises(ValueError):
        grid.closest(p)
    # empty sides
    empty = rf.closest_points_on_mesh(p, rf.Mesh(good.vertices, good.faces[:0], None, None))
    assert torch.isinf(empty.distance).all() and (empty.face == -1).all() and torch.isnan(empty.point).all()
    none = rf.closest_points_on_mesh(p[:0], good)
    assert none.distance.shape == (0,) and none.face.shape == (0,) and none.point.shape == (0, 3)


def test_sample_mesh_surface():
    v, f = M.icosphere()
    f = np.concatenate([[[0, 0, 1]], f[:700], [[5, 5, 5], [7, 9, 7]], f[700:], [[2, 3, 3]]])  # zero-area faces in front, inside, at the end
    mesh, count = mesh_of(v, f), 5000
    points, faces, bary = host(rf.sample_mesh_surface(mesh, count, seed=7))
    assert points.shape == (count, 3) and points.dtype == f32 and faces.shape == (count,) and faces.dtype == np.int64 and bary.shape == (count, 3) and bary.dtype == f32
    assert (bary >= 0).all() and (np.abs(bary.astype(np.float64).sum(1) - 1) <= 4 * M.U).all()
    corners = v[f[faces]].astype(np.float64)
    assert np.abs((bary.astype(np.float64)[:, :, None] * corners).sum(1) - points).max() <= 8 * M.U
    c = v[f].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1)
    counts = np.bincount(faces, minlength=len(f))
    assert (area[[0, 701, 702, len(f) - 1]] == 0).all() and counts[area == 0].sum() == 0
    assert (np.abs(counts - count * area / area.sum()) < 2).all()
    assert (np.diff(faces) >= 0).all()  # one stratum after the other
    d = rf.closest_points_on_mesh(torch.from_numpy(points).to(dev()), mesh).distance.cpu().numpy()
    B = M.bound(points, v, f)
    print(f"samples on their faces: worst distance / B {float((d / B).max()):.3g}")
    assert (d <= B).all()
    again = host(rf.sample_mesh_surface(mesh, count, seed=7))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (points, faces, bary)))
    assert host(rf.sample_mesh_surface(mesh, count, seed=8))[0].tobytes() != points.tobytes()
    assert rf.sample_mesh_surface(mesh, 0)[0].shape == (0, 3)


def test_mesh_distance_of_two_squares_is_exact():
    square = lambda z: mesh_of(np.array([[0, 0, z], [4, 0, z], [4, 4, z], [0, 4, z]], dtype=f32), np.array([[0, 1, 2], [0, 2, 3]]))  # noqa: E731
    r = rf.mesh_distance(square(0.0), square(0.5), samples=20000, thresholds=(0.5, 0.49))
    for side in (r.a_to_b, r.b_to_a):
        assert side.mean == 0.5 and side.rms == 0.5 and side.max == 0.5 and side.median == 0.5 and side.q90 == 0.5 and side.q99 == 0.5
    assert r.chamfer_l1 == 0.5 and r.chamfer_l2 == 0.25 and r.hausdorff == 0.5 and r.samples == 20000
    assert r.thresholds[0] == rf.ThresholdScore(0.5, 1.0, 1.0, 1.0) and r.thresholds[1] == rf.ThresholdScore(0.49, 0.0, 0.0, 0.0)


def test_mesh_distance_of_a_mesh_to_itself_and_against_the_model():
    v, f = M.icosphere()
    v2 = M.perturbed(v)
    a, b, n = mesh_of(v, f), mesh_of(v2, f), 3000
    # to itself: nothing above the largest bound of a sample or a vertex
    sample_bounds = [M.bound(np.concatenate([host(rf.sample_mesh_surface(a, n, seed=s))[0], v]), v, f).max() for s in (4, 5)]
    top = float(max(sample_bounds))
    r = rf.mesh_distance(a, a, samples=n, thresholds=(top,), seed=4)
    for side in (r.a_to_b, r.b_to_a):
        assert all(0 <= x <= top for x in side)
    assert r.chamfer_l1 <= top and r.chamfer_l2 <= top * top and r.hausdorff <= top and r.thresholds[0].fscore == 1.0
    # against the model's reductions of the same sample distances
    r = rf.mesh_distance(a, b, samples=n, thresholds=(0.01, 0.03, 1e-9), seed=4)
    pa, pb = rf.sample_mesh_surface(a, n, seed=4)[0], rf.sample_mesh_surface(b, n, seed=5)[0]
    distance = lambda p, m: rf.closest_points_on_mesh(p, m).distance.cpu().numpy()  # noqa: E731
    model = M.reductions(distance(pa, b), distance(pb, a), distance(a.vertices, b), distance(b.vertices, a), thresholds=(0.01, 0.03, 1e-9))
    close = lambda x, y: abs(x - y) <= 1e-13 * max(abs(y), 1e-30) * n  # noqa: E731  (float64 sums of n terms in another order)
    for side, want in ((r.a_to_b, model["a_to_b"]), (r.b_to_a, model["b_to_a"])):
        for key in ("mean", "rms", "max", "median", "q90", "q99"):
            assert close(getattr(side, key), want[key]), key
    assert close(r.chamfer_l1, model["chamfer_l1"]) and close(r.chamfer_l2, model["chamfer_l2"]) and r.hausdorff == model["hausdorff"]
    assert 0 < r.thresholds[0].fscore < r.thresholds[1].fscore <= 1 and r.thresholds[2].fscore == 0.0
    for got, want in zip(r.thresholds, model["thresholds"]):
        assert close(got.precision, want["precision"]) and close(got.recall, want["recall"]) and close(got.fscore, want["fscore"])  # (k / n rounds once in numpy, the mean of n terms in torch)
    assert 0.02 < r.hausdorff <= 0.05 + 1e-6 and r.a_to_b.mean < r.hausdorff  # a radial perturbation of at most 5 %
