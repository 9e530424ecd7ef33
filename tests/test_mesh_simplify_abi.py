"""rf_mesh_cluster_keys / rf_mesh_cluster_vertices: the symbols are exported, the unit is a build input, the header declares them,
and every argument check of include/relu_field.h comes back as a code before any launch (no GPU needed), in the documented order."""
import ctypes as C
import os
import re

import pytest

from thr3ed_atom_amd import _lib

OK, NULL, SHAPE = 0, -1, -2
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_points(lib):
    for name in ("rf_mesh_cluster_keys", "rf_mesh_cluster_vertices"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "mesh_simplify_kernels.hip" in _lib.SOURCES
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    assert "int rf_mesh_cluster_keys(const float* vertices_dev, int64_t num_vertices, const float* origin, float r, const int32_t* cells, int64_t* keys_dev," in header
    assert "int rf_mesh_cluster_vertices(const float* vertices_dev, const float* colours_dev, const float* normals_dev, int64_t num_vertices," in header
    assert "enum { RF_MESH_PLACEMENT_QUADRIC = 0, RF_MESH_PLACEMENT_MEAN = 1 };" in header
    assert _lib.MESH_PLACEMENTS == {"quadric": 0, "mean": 1}
    # the constants the tests place their shapes by are the ones the unit is compiled with
    source = open(os.path.join(_lib.CSRC_DIR, "mesh_simplify_kernels.hip")).read()
    assert [int(v) for v in re.findall(r"constexpr int kClusterGroup = (\d+);", source)] == [_lib.MESH_CLUSTER_GROUP]
    assert [int(v) for v in re.findall(r"constexpr int kClusterBlock = (\d+);", source)] == [_lib.MESH_CLUSTER_GROUP * _lib.MESH_CLUSTERS_PER_BLOCK]
    assert [int(v) for v in re.findall(r"constexpr long long kLongSegment = (\d+);", source)] == [_lib.MESH_LONG_SEGMENT]
    assert [v for v in re.findall(r"constexpr int kMaxCells = (.+?);", source)] == ["1 << 20"] and _lib.MESH_MAX_CELLS == 1 << 20
    # the hot path is a gather: no atomics in the unit
    code = re.sub(r"//.*", "", source)
    assert "atomic" not in code.lower()
    assert "-ffp-contract=off" in _lib.HIPCC_FLAGS  # the float32 cell arithmetic is two rounded operations


def triple(values, ctype):
    return None if values is None else (ctype * 3)(*values)


def test_cluster_keys_validates_before_any_launch(lib):
    def call(vertices=64, count=10, origin=(0.0, 0.0, 0.0), r=2.0, cells=(4, 4, 4), keys=128, status=256):
        return lib.rf_mesh_cluster_keys(vertices, count, triple(origin, C.c_float), r, triple(cells, C.c_int32), keys, status, None)

    for missing in ("vertices", "origin", "cells", "keys", "status"):
        assert call(**{missing: None}) == NULL
    assert call(count=-1) == SHAPE and call(count=2**31) == SHAPE and call(count=2**40) == SHAPE
    for r in (0.0, -1.0, NAN, INF):
        assert call(r=r) == SHAPE
    assert call(origin=(0.0, NAN, 0.0)) == SHAPE and call(origin=(INF, 0.0, 0.0)) == SHAPE
    for cells in ((0, 4, 4), (4, -1, 4), (4, 4, (1 << 20) + 1)):
        assert call(cells=cells) == SHAPE
    assert call(count=0) == OK and call(count=0, cells=(1 << 20, 1, 1 << 20)) == OK  # nothing to do: no launch
    # the order: pointers, then the count, then r, the origin, the cells; an empty input is still checked
    assert call(keys=None, count=-1, r=0.0) == NULL
    assert call(count=0, r=0.0) == SHAPE and call(count=0, cells=(0, 1, 1)) == SHAPE


def test_cluster_vertices_validates_before_any_launch(lib):
    def call(vertices=64, colours=None, normals=None, num_vertices=10, faces=128, num_faces=5, members=192, member_begin=256, corners=320, corner_begin=384,
             keys=448, num_clusters=3, origin=(0.0, 0.0, 0.0), h=0.5, cells=(4, 4, 4), placement=0, regularisation=1e-3, out=512, colours_out=None,
             normals_out=None):
        return lib.rf_mesh_cluster_vertices(vertices, colours, normals, num_vertices, faces, num_faces, members, member_begin, corners, corner_begin, keys,
                                            num_clusters, triple(origin, C.c_float), h, triple(cells, C.c_int32), placement, regularisation, out, colours_out,
                                            normals_out, None)

    for missing in ("vertices", "faces", "members", "member_begin", "corners", "corner_begin", "keys", "origin", "cells", "out"):
        assert call(**{missing: None}) == NULL
    # an optional attribute is given on both sides or on neither
    assert call(colours=576) == NULL and call(colours_out=576) == NULL and call(normals=576) == NULL and call(normals_out=576) == NULL
    # negative counts
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE and call(num_clusters=-1) == SHAPE
    # too many
    assert call(num_vertices=2**31) == SHAPE and call(num_clusters=11) == SHAPE and call(num_faces=2**40) == SHAPE
    # h (and its reciprocal)
    for h in (0.0, -0.5, NAN, INF, 1e-45):
        assert call(h=h) == SHAPE
    assert call(origin=(NAN, 0.0, 0.0)) == SHAPE
    for cells in ((0, 4, 4), (4, 4, -3), ((1 << 20) + 1, 4, 4)):
        assert call(cells=cells) == SHAPE
    for placement in (-1, 2, 7):
        assert call(placement=placement) == SHAPE
    for regularisation in (0.0, 9e-7, 1.0001, -1e-3, NAN, INF):
        assert call(regularisation=regularisation) == SHAPE
    # nothing to do: no launch (the pointers above are not device memory -- a launch would not return 0 here without a device)
    assert call(num_clusters=0) == OK and call(num_vertices=0, num_clusters=0) == OK
    assert call(num_clusters=0, placement=1, regularisation=1.0, h=1e30, cells=(1 << 20, 1, 1)) == OK
    assert call(num_clusters=0, regularisation=1e-6) == OK
    # the order of the checks: pointers < counts < h < origin < cells < placement < regularisation < "nothing to do"
    assert call(out=None, num_faces=-1) == NULL
    assert call(colours=576, num_vertices=-1) == NULL
    assert call(num_clusters=0, regularisation=2.0) == SHAPE and call(num_vertices=0, num_clusters=0, placement=5) == SHAPE
    assert call(num_clusters=0, h=0.0) == SHAPE and call(num_clusters=0, cells=(0, 0, 0)) == SHAPE
