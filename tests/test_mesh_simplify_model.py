"""The numpy model of mesh simplification (tests/mesh_simplify_model.py) against hand-checked cases and the properties the
contract promises.  No GPU: this file pins the model, tests/test_hip_mesh_simplify.py pins the kernels to it."""
import functools

import numpy as np
import pytest

from tests import mesh_simplify_model as mm

SHIFT = 0.0137  # the cube [-1, 1]^3 + SHIFT: no face of it lies on a cell boundary by accident of round numbers
CUBE_CELLS = (0.21, 0.37)


@functools.lru_cache(maxsize=None)
def cube():
    v, f = mm.cube_surface(24, shift=SHIFT)
    v.setflags(write=False), f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def sphere():
    v, f, n = mm.uv_sphere(24, 32, radius=0.9, centre=(0.11, -0.23, 0.05))
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


@functools.lru_cache(maxsize=None)
def simplified_cube(h, placement):
    return mm.simplify(*cube(), h, placement=placement)


def distance_to_cube_surface(points):
    x = np.abs(np.asarray(points, dtype=np.float64) - SHIFT)
    outside = np.linalg.norm(np.maximum(x - 1.0, 0.0), axis=1)
    return np.where(x.max(axis=1) <= 1.0, 1.0 - x.max(axis=1), outside)


# ------------------------------------------------------------------------------------------------------ the builders

def test_the_builders_make_closed_oriented_surfaces():
    v, f = cube()
    assert len(f) == 6 * 2 * 24 * 24 and len(v) == 6 * 24 * 24 + 2 and mm.directed_edge_balance(f)
    centroid, normal = v[f].astype(np.float64).mean(axis=1) - SHIFT, np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((centroid * normal).sum(axis=1) > 0).all()  # outward
    v, f, n = sphere()
    assert len(f) == 2 * 32 * 23 and len(v) == 2 + 23 * 32 and mm.directed_edge_balance(f)
    centre = np.asarray([0.11, -0.23, 0.05])
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (((v[f].astype(np.float64).mean(axis=1) - centre) * normal).sum(axis=1) > 0).all()
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    for k in (1, 2, 3, 17):
        v, f = mm.triangle_fan(k)
        assert len(f) == k and (f == 0).sum() == k and len(np.unique(f)) == len(v)
    v, f, nrm = mm.plane_patch(5)
    assert len(f) == 50 and np.abs(v.astype(np.float64) @ nrm - 0.21).max() < 1e-7


# ------------------------------------------------------------------------------------------------------ hand-checked cases

TETRAHEDRON = (np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32), np.asarray([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))


def test_a_tetrahedron_inside_one_cell_collapses_to_nothing():
    s = mm.simplify(*TETRAHEDRON, 1.5)
    assert s.clusters == 1 and s.collapsed_faces == 4 and s.merged_duplicates == 0
    assert s.faces.shape == (0, 3) and s.vertices.shape == (0, 3) and (s.cluster_of_vertex == -1).all()
    assert s.corner_records.tolist() == [12] and s.member_records.tolist() == [4]


def test_two_faces_on_one_oriented_triple_are_merged():
    # vertices 0 / 3 share a cell, as do 1 / 4; faces (0, 1, 2) and (4, 2, 3) both map to the oriented triple (A, B, C)
    v = np.asarray([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [0.3, 0.2, 0.1], [1.3, 0.2, 0.1]], dtype=np.float32)
    f = np.asarray([[0, 1, 2], [4, 2, 3]])
    s = mm.simplify(v, f, 1.0, origin=(0, 0, 0))
    assert s.clusters == 3 and s.collapsed_faces == 0 and s.merged_duplicates == 1 and len(s.faces) == 1
    # keys: (0,0,0) -> 0, (0,1,0) -> 1, (1,0,0) -> 2 with cells (2, 2, 1); the face (A=0, B=2, C=1) starts at its smallest index
    assert s.cluster_keys.tolist() == [0, 1, 2] and s.faces.tolist() == [[0, 2, 1]]
    assert s.cluster_of_vertex.tolist() == [0, 2, 1, 0, 2]
    # the opposite orientation is another triple: both survive
    s = mm.simplify(v, np.asarray([[0, 1, 2], [3, 2, 4]]), 1.0, origin=(0, 0, 0))
    assert s.merged_duplicates == 0 and s.faces.tolist() == [[0, 1, 2], [0, 2, 1]]


def test_a_vertex_on_a_cell_boundary_belongs_to_the_upper_cell():
    h = np.float32(0.25)
    v = np.asarray([[0.5, 0.0, 0.0], [0.49999997, 0.0, 0.0], [0.0, 0.75, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    lat = mm.lattice_of(v, h, origin=(0, 0, 0))
    assert lat.k.tolist() == [[2, 0, 0], [1, 0, 0], [0, 3, 0], [0, 0, 4]] and lat.cells.tolist() == [3, 4, 5]
    assert lat.keys.tolist() == [(2 * 4 + 0) * 5, (1 * 4) * 5, 3 * 5, 4]
    with pytest.raises(ValueError):
        mm.lattice_of(v, h, origin=(0.1, 0, 0))


def test_a_vertex_that_no_face_uses_goes_nowhere():
    v = np.concatenate([TETRAHEDRON[0], [[5.0, 5.0, 5.0]]]).astype(np.float32)
    s = mm.simplify(v, TETRAHEDRON[1], 0.6)
    assert s.clusters == 5 and len(s.vertices) == 4 and len(s.faces) == 4
    assert s.cluster_of_vertex.tolist() == [0, 3, 2, 1, -1]  # (keys ascend with x first; the stray vertex has the largest key)


def test_the_quadric_puts_a_corner_back_where_the_mean_rounds_it_off():
    # the three faces of a cube corner at (0.4, 0.4, 0.4), all inside the cell [0, 1]^3 of a lattice at the origin: the planes meet there
    v, f = mm.cube_surface(4, low=-0.4, high=0.4)
    s = mm.simplify(v, f, 1.0, origin=(-1, -1, -1), regularisation=1e-6)
    assert s.clusters == 8 and len(s.vertices) == 8 and len(s.faces) == 12  # a cube again
    assert np.abs(np.abs(s.vertices64) - 0.4).max() < 1e-5
    mean = mm.simplify(v, f, 1.0, origin=(-1, -1, -1), placement="mean")
    assert np.array_equal(mean.faces, s.faces) and np.abs(np.abs(mean.vertices64) - 0.4).min() > 0.05


# ------------------------------------------------------------------------------------------------------ properties

@pytest.mark.parametrize("h", CUBE_CELLS)
def test_quadric_vertices_lie_on_the_cube_and_mean_vertices_do_not(h):
    quadric, mean = simplified_cube(h, "quadric"), simplified_cube(h, "mean")
    off = distance_to_cube_surface(quadric.vertices64).max() / h
    print(f"h = {h}: quadric {off:.3g} h, mean {distance_to_cube_surface(mean.vertices64).max() / h:.3g} h off the surface")
    assert off < 2e-3  # lambda's bias (7.9e-4 h and 9.0e-4 h at the prototype)
    assert distance_to_cube_surface(mean.vertices64).max() > 0.1 * h
    assert np.array_equal(quadric.faces, mean.faces) and np.array_equal(quadric.cluster_of_vertex, mean.cluster_of_vertex)


def test_a_planar_patch_stays_on_its_plane():
    v, f, nrm = mm.plane_patch(20)
    input_error = np.abs(v.astype(np.float64) @ nrm - 0.21).max()  # float32 rounding of the inputs
    for h in (0.11, 0.3):
        s = mm.simplify(v, f, h)
        assert len(s.faces) > 0
        off = np.abs(s.vertices64 @ nrm - 0.21)
        # a cluster whose quadric is one plane is pulled along the plane only; the clamp moves a vertex along an axis, so it applies
        # to vertices strictly inside their cell
        k = np.floor((s.vertices64 - v.min(axis=0)) / h)
        centre = v.min(axis=0).astype(np.float64) + (k + 0.5) * h
        interior = (np.abs(s.vertices64 - centre) < 0.5 * h * (1 - 1e-9)).all(axis=1)
        assert interior.sum() > len(interior) // 2
        assert off[interior].max() <= 8 * input_error + 1e-9 * h, (off[interior].max(), input_error)


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_every_representative_lies_in_its_closed_cell(placement):
    for vertices, faces, h in ((*cube(), 0.21), (*cube(), 0.37), (*sphere()[:2], 0.3), (*sphere()[:2], 0.083)):
        s = mm.simplify(vertices, faces, h, placement=placement, regularisation=1e-6)
        lat = mm.lattice_of(vertices, h)
        key = s.vertex_keys
        k = np.stack([key // (lat.cells[1] * lat.cells[2]), key // lat.cells[2] % lat.cells[1], key % lat.cells[2]], -1)
        centre = lat.origin.astype(np.float64) + (k + 0.5) * float(lat.h)
        assert (np.abs(s.vertices64 - centre) <= 0.5 * float(lat.h) * (1 + 1e-12)).all()


def test_closed_surfaces_stay_balanced_where_nothing_was_merged():
    for vertices, faces, h in ((*cube(), 0.21), (*cube(), 0.37), (*sphere()[:2], 0.3), (*sphere()[:2], 0.17)):
        s = mm.simplify(vertices, faces, h)
        assert s.merged_duplicates == 0 and len(s.faces) > 0  # the condition under which the property is promised
        assert mm.directed_edge_balance(s.faces)
        assert len(s.faces) == s.input_faces - s.collapsed_faces


def test_the_output_is_canonical():
    v, f, n = sphere()
    s = mm.simplify(v, f, 0.3, normals=n, colours=np.abs(n))
    assert (s.faces[:, 0] < s.faces[:, 1]).all() and (s.faces[:, 0] < s.faces[:, 2]).all()
    order = np.lexsort((s.faces[:, 2], s.faces[:, 1], s.faces[:, 0]))
    assert np.array_equal(order, np.arange(len(order))) and len(np.unique(s.faces, axis=0)) == len(s.faces)
    assert (np.diff(s.vertex_keys) > 0).all() and np.array_equal(np.unique(s.faces), np.arange(len(s.vertices)))
    assert np.allclose(np.linalg.norm(s.normals64, axis=1), 1.0, atol=1e-12) and (s.colours64 >= 0).all() and (s.colours64 <= 1).all()
    # orientation survives: the normals of the simplified sphere point away from its centre
    centre = np.asarray([0.11, -0.23, 0.05])
    tri = s.vertices64[s.faces]
    assert ((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) * (tri.mean(axis=1) - centre)).sum(axis=1) > 0).all()
    # a permutation of the input faces changes nothing but the order of the sums
    again = mm.simplify(v, f[::-1], 0.3, normals=n, colours=np.abs(n))
    assert np.array_equal(again.faces, s.faces) and mm.compare(s, again.vertices, again.faces, again.colours, again.normals) == []


@pytest.mark.parametrize("target", [0, 40, 500, 1471, 100000])
def test_target_faces_is_the_stated_bisection(target):
    v, f, _ = sphere()
    s = mm.simplify(v, f, target_faces=target)
    assert len(s.faces) <= target
    # the bisection, restated
    extent = np.float32((v.max(axis=0) - v.min(axis=0)).max())
    count = lambda n: mm.face_count(v, f, np.float32(float(extent) / n))
    lo, hi = 1, 4096
    if count(hi) <= target:
        lo = hi
    else:
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if count(mid) <= target else (lo, mid)
    assert s.cell_size == float(np.float32(float(extent) / lo))
    assert len(s.faces) == count(lo)
    if target == 100000:
        assert lo == 4096 and len(s.faces) == len(f)  # fine enough for every vertex to keep a cell of its own


def test_bad_inputs_raise():
    v, f = TETRAHEDRON
    with pytest.raises(ValueError):
        mm.simplify(v, f + 1, 0.5)
    with pytest.raises(ValueError):
        mm.simplify(v * np.float32("nan"), f, 0.5)
    with pytest.raises(ValueError):
        mm.simplify(v, f, 0.5, origin=(0.5, 0, 0))
    with pytest.raises(ValueError):
        mm.simplify(v, f, 1e-7)  # more than 2^20 cells


# ------------------------------------------------------------------------------------------------------ the comparison can fail

def test_the_comparison_reports_a_moved_vertex_a_swapped_face_and_a_wrong_count():
    v, f, n = sphere()
    h = 0.3
    s = mm.simplify(v, f, h, normals=n, colours=np.abs(n))
    counts = (s.clusters, len(s.vertices), s.input_faces, s.collapsed_faces, s.merged_duplicates, len(s.faces))
    assert mm.compare(s, s.vertices, s.faces, s.colours, s.normals, s.cluster_of_vertex, counts) == []
    moved = s.vertices.copy()
    moved[7, 1] += np.float32(1e-4 * h)
    assert any(p.startswith("vertices") for p in mm.compare(s, moved, s.faces, s.colours, s.normals))
    swapped = s.faces.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert any(p.startswith("faces") for p in mm.compare(s, s.vertices, swapped, s.colours, s.normals))
    assert any(p.startswith("faces") for p in mm.compare(s, s.vertices, s.faces.astype(np.int32), s.colours, s.normals))
    tinted = s.colours.copy()
    tinted[0, 0] += np.float32(1e-6)
    assert any(p.startswith("colours") for p in mm.compare(s, s.vertices, s.faces, tinted, s.normals))
    assert any(p.startswith("normals") for p in mm.compare(s, s.vertices, s.faces, s.colours, None))
    other = s.cluster_of_vertex.copy()
    other[0] = -1 if other[0] >= 0 else 0
    assert "cluster_of_vertex differs" in mm.compare(s, s.vertices, s.faces, s.colours, s.normals, other)
    assert any(p.startswith("counts") for p in mm.compare(s, s.vertices, s.faces, s.colours, s.normals, None, counts[:5] + (counts[5] + 1,)))
    nan = s.vertices.copy()
    nan[0, 0] = np.nan
    assert mm.compare(s, nan, s.faces, s.colours, s.normals) != []
    # and the bound is tight enough to mean something: a float32 ulp or two
    assert s.vertex_bound.max() < 4 * 2.0 ** -24 * np.abs(s.vertices64).max() + 1e-12
