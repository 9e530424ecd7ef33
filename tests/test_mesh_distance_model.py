"""The numpy model of the mesh distance (tests/mesh_distance_model.py) against closed forms and against itself: the rule, the lattice's
pair lists, the ring search with its stop test -- and that the comparison can fail: a lattice that skips faces and a stop test without
its slack both give wrong answers that the brute force exposes.  No GPU needed."""
import numpy as np
import pytest

from tests import mesh_distance_model as M

f32 = np.float32


def test_the_rule_against_closed_forms():
    a, b, c = np.array([0.0, 0, 0]), np.array([4.0, 0, 0]), np.array([0.0, 4, 0])
    for dtype in (np.float64, np.float32):
        rule = lambda p: M.closest_on_face(np.array(p, dtype=dtype), a, b, c, dtype)  # noqa: E731
        d2, q = rule([1, 1, 3])          # above the interior: the plane
        assert d2 == 9 and q.tolist() == [1, 1, 0] and d2.dtype == dtype
        d2, q = rule([-3, -4, 0])        # beyond corner a, a 3-4-5 offset
        assert d2 == 25 and q.tolist() == [0, 0, 0]
        d2, q = rule([1, -2, 0])         # beyond edge ab at t = 1/4
        assert d2 == 4 and q.tolist() == [1, 0, 0]
        d2, q = rule([4, 4, 0])          # beyond the hypotenuse: its midpoint
        assert d2 == 8 and q.tolist() == [2, 2, 0]
        d2, q = rule([7, -4, 0])         # beyond corner b
        assert d2 == 25 and q.tolist() == [4, 0, 0]
    # degenerate faces are their segments or their point, without a NaN
    p = np.array([1.0, 2, 2])
    for dtype in (np.float64, np.float32):
        d2, q = M.closest_on_face(p, a, a, a, dtype)
        assert d2 == 9 and q.tolist() == [0, 0, 0]
        d2, q = M.closest_on_face(p, a, b, b, dtype)   # a repeated vertex: the segment ab
        assert d2 == 8 and q.tolist() == [1, 0, 0]
        d2, q = M.closest_on_face(p, a, 0.5 * b, b, dtype)  # collinear corners
        assert d2 == 8 and q.tolist() == [1, 0, 0]
        d2, q = M.closest_on_face(np.array([9.0, 0, 0]), a, 0.5 * b, b, dtype)
        assert d2 == 25 and q.tolist() == [4, 0, 0]


def test_the_rule_against_a_dense_sampling_of_the_face():
    rng = np.random.default_rng(0)
    tri = rng.uniform(-1, 1, size=(3, 3))
    u = rng.uniform(size=(200000, 2))
    s = np.sqrt(u[:, 0])
    on_face = (1 - s)[:, None] * tri[0] + (s * (1 - u[:, 1]))[:, None] * tri[1] + (s * u[:, 1])[:, None] * tri[2]
    for p in rng.uniform(-2, 2, size=(20, 3)):
        d2, q = M.closest_on_face(p, *tri)
        sampled = np.sqrt(((on_face - p) ** 2).sum(1).min())
        assert np.sqrt(d2) <= sampled + 1e-12 and sampled - np.sqrt(d2) < 0.02  # no sample is closer; one is nearly as close
        assert abs(np.linalg.norm(p - q) - np.sqrt(d2)) < 1e-12
        assert M.closest_on_face(q, *tri)[0] < 1e-24  # the point lies on the face


FIXTURES = {
    "cube": (M.cube(), (f32(2.0), f32(0.3), f32(0.0625))),
    "icosphere": (M.icosphere(), (f32(4.0), f32(0.5), f32(0.11))),
    "perturbed": ((M.perturbed(M.icosphere()[0]), M.icosphere()[1]), (f32(4.0), f32(0.37))),
    "soup": (M.soup(), (f32(4.0), f32(0.25), f32(0.6))),
}


@pytest.fixture(scope="module")
def references():
    out = {}
    for name, ((v, f), sizes) in FIXTURES.items():
        q = M.queries(v, f, 40, h=sizes[-1])
        out[name] = (q, M.brute_force(q, v, f, np.float32))
    return out


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_ring_search_is_the_brute_force_for_every_cell_size(name, references):
    (v, f), sizes = FIXTURES[name]
    q, (d, face, point) = references[name]
    rings = []
    for h in sizes + (M.default_cell_size(v, f),):
        grid = M.lattice(v, f, h)
        got = M.ring_search(q, v, f, grid, M.pair_lists(v, f, grid))
        assert got[0].tobytes() == d.tobytes() and (got[1] == face).all() and got[2].tobytes() == point.tobytes(), (name, float(h))
        rings.append(int(got[3].max()))
    assert rings[0] == 0 and max(rings) >= 2  # one cell is the brute force; a fine lattice really walks


def test_the_float32_rule_stays_within_the_bound_of_the_float64_one(references):
    for name, ((v, f), _) in FIXTURES.items():
        q, (d32, face32, _) = references[name]
        d64 = np.sqrt(M.face_distances2(q, v, f))
        B = M.bound(q, v, f, d64)
        assert (np.abs(d32.astype(np.float64) - d64.min(axis=1)) <= B).all(), name
        assert (d64[np.arange(len(q)), face32] <= d64.min(axis=1) + B).all(), name
        assert B.max() < 1e-3  # (of a coordinate scale of 1 .. 20: the bound says something)


def test_max_distance_in_the_model():
    v, f = M.icosphere()
    grid = M.lattice(v, f, f32(0.2))
    lists = M.pair_lists(v, f, grid)
    q = M.queries(v, f, 30)
    free = M.ring_search(q, v, f, grid, lists)
    cut = M.ring_search(q, v, f, grid, lists, max_distance=0.05)
    near = free[0] <= f32(0.05)
    assert near.any() and (~near).any()
    assert (cut[0][near] == free[0][near]).all() and (cut[1][near] == free[1][near]).all() and np.isinf(cut[0][~near]).all() and (cut[1][~near] == -1).all()
    assert np.isnan(cut[2][~near]).all() and cut[3].max() <= free[3].max()


def test_every_face_is_registered_in_every_cell_a_point_of_it_lies_in():
    rng = np.random.default_rng(2)
    for name, ((v, f), sizes) in FIXTURES.items():
        for h in sizes:
            grid = M.lattice(v, f, h)
            begin, cell_faces = M.pair_lists(v, f, grid)
            assert begin[-1] == len(cell_faces) and (np.diff(begin) >= 0).all()
            some = rng.choice(len(f), size=min(len(f), 60), replace=False)
            b = M.barycentrics(rng.uniform(size=(len(some), 400)), rng.uniform(size=(len(some), 400)))  # [faces, samples, 3]
            b = np.concatenate([b, np.eye(3)[None].repeat(len(some), 0)], axis=1)                   # ... and the corners themselves
            on_face = (b[..., None] * v[f[some]].astype(np.float64)[:, None]).sum(axis=2).astype(f32)
            cell = M.cells_of(on_face, grid)
            key = (cell[..., 0] * grid[3][1] + cell[..., 1]) * grid[3][2] + cell[..., 2]
            for row, face in zip(key, some):
                for k in np.unique(row):
                    assert face in cell_faces[begin[k]:begin[k + 1]], (name, float(h), face, k)


def test_a_lattice_that_skips_faces_fails_the_comparison():
    v, f = M.soup()
    grid = M.lattice(v, f, f32(0.25))
    giant = v[f[2020]].astype(np.float64)  # (2 000 random and 20 degenerate faces come first)
    assert np.abs(giant[1] - giant[0]).max() == 2
    on_giant = np.array([[0.4, 0.3, 0.3], [0.2, 0.5, 0.3], [0.3, 0.2, 0.5]]) @ giant
    q = np.concatenate([M.queries(v, f, 60, h=f32(0.25)), on_giant.astype(f32)])
    d, face, _ = M.brute_force(q, v, f, np.float32)
    good = M.ring_search(q, v, f, grid, M.pair_lists(v, f, grid))
    broken = M.ring_search(q, v, f, grid, M.pair_lists(v, f, grid, whole_box=False))  # the giant triangle is only in its corners' cells
    assert good[0].tobytes() == d.tobytes() and (good[1] == face).all()
    assert (face[-3:] == 2020).all() and (broken[1][-3:] != 2020).all() and (broken[0][-3:] > d[-3:]).all() and (broken[0] >= d).all()


def test_a_stop_test_without_its_slack_fails_the_comparison():
    """a coordinate v one ulp below fl(o + K h) that the cell rule nevertheless puts into cell K: the plain plane overstates the gap
    to cell K by that ulp, and a face at a distance between the two is taken for the minimum"""
    found = None
    for h in (f32(0.3), f32(0.7), f32(0.9), f32(1.1), f32(1.3)):
        K = np.arange(1, 1000)
        plane = (K.astype(f32) * h).astype(f32)
        v = np.nextafter(plane, f32(-np.inf))
        inside = np.floor((v * (f32(1.0) / h)).astype(f32)) >= K  # (origin 0)
        if inside.any():
            found = (h, int(K[inside][-1]), v[inside][-1], plane[inside][-1])
            break
    assert found is not None
    h, K, v, plane = found
    ulp = f32(plane - v)
    p = np.array([v - 16 * ulp, 0, 0], dtype=f32)
    point_face = lambda x, y: [[x, y, 0]] * 3  # noqa: E731
    tris = np.array([point_face(0, 0), point_face(p[0], 16.5 * ulp), point_face(v, 0)], dtype=f32)  # face 1 at 16.5 ulp in p's cell, face 2 at 16 ulp in cell K
    vertices, faces = tris.reshape(-1, 3), np.arange(9).reshape(3, 3)
    grid = M.lattice(vertices, faces, h)
    assert M.cells_of(p, grid)[0] == K - 1 and M.cells_of(tris[2, 0], grid)[0] == K and grid[3][0] > K
    lists = M.pair_lists(vertices, faces, grid)
    d, face, _ = M.brute_force(p, vertices, faces, np.float32)
    assert face[0] == 2 and d[0] == 16 * ulp
    good, broken = M.ring_search(p, vertices, faces, grid, lists), M.ring_search(p, vertices, faces, grid, lists, slack=False)
    assert good[1][0] == 2 and good[0][0] == d[0] and good[3][0] >= 1
    assert broken[1][0] == 1 and broken[3][0] == 0  # stopped in its own cell, with the wrong face


def test_the_default_cell_size_respects_its_limits():
    for name, ((v, f), _) in FIXTURES.items():
        h = M.default_cell_size(v, f)
        grid = M.lattice(v, f, h)
        lo, hi = M.face_cell_ranges(v, f, grid)
        assert (grid[3] <= M.MAX_CELLS).all() and grid[3].prod() + 1 <= M.MAX_TABLE
        assert (hi - lo + 1).prod(axis=1).sum() <= 16 * len(f) + 2 ** 20
    v, f = M.icosphere()
    c = v[f].astype(np.float64)
    mean_area = (0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1)).mean()
    assert M.default_cell_size(v, f) == f32(2 * np.sqrt(2 * mean_area))  # nothing to double on a sphere
    flat = np.zeros((3, 3), dtype=f32)
    assert M.default_cell_size(flat, np.array([[0, 1, 2]])) == 1.0  # no area, no extent


def test_the_strata_rule_and_the_reductions():
    area = np.array([0.0, 3.0, 0.0, 1.0, 4.0, 0.0])
    rng = np.random.default_rng(4)
    picked = M.strata_faces(area, rng.uniform(size=1000))
    counts = np.bincount(picked, minlength=6)
    assert counts[[0, 2, 5]].sum() == 0 and (np.abs(counts - 1000 * area / area.sum()) < 2).all()
    assert (M.strata_faces(area, np.nextafter(np.ones(8), 0)) <= 4).all()
    b = M.barycentrics(rng.uniform(size=100), rng.uniform(size=100))
    assert (b >= 0).all() and np.allclose(b.sum(-1), 1)
    r = M.reductions([0.5, 0.5, 0.5, 0.5], [0.0, 1.0, 0.0, 1.0], [0.5], [2.0], thresholds=(0.5, 0.25))
    assert r["a_to_b"]["mean"] == 0.5 and r["b_to_a"]["max"] == 2.0 and r["hausdorff"] == 2.0 and r["chamfer_l1"] == 0.5 and r["chamfer_l2"] == 0.375
    assert r["thresholds"][0]["precision"] == 1.0 and r["thresholds"][0]["recall"] == 0.5 and abs(r["thresholds"][0]["fscore"] - 2 / 3) < 1e-15
    assert r["thresholds"][1]["precision"] == 0.0 and r["thresholds"][1]["fscore"] == 0.0
