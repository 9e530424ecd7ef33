"""rf_mesh_raster_coverage, rf_mesh_geometry_backward_pixels, rf_mesh_geometry_backward_gather: the symbols are exported, the new unit is a
build input and takes the rasteriser's quantities from the rasteriser's own device functions, the header declares them, and every argument check of include/relu_field.h comes back as a
code before any launch (no GPU needed), in the documented order."""
import ctypes as C
import os
import re

import pytest

from tests import csrc_text
from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
NAN, INF = float("nan"), float("inf")
NEW = ("rf_mesh_raster_coverage", "rf_mesh_geometry_backward_pixels", "rf_mesh_geometry_backward_gather")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_points(lib):
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "mesh_fit_kernels.hip" in _lib.SOURCES and os.path.join(_lib.CSRC_DIR, "mesh_fit_kernels.hip") in _lib.build_inputs()
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    for name in NEW:
        assert f"int {name}(const " in header
    code = csrc_text.code("mesh_fit_kernels.hip")
    assert re.findall(r"constexpr int kLongSegment = (\d+);", code) == [str(_lib.MESH_FIT_LONG_SEGMENT)]
    # gather form: no atomics, no memset, no LDS, no inline assembly in the unit and the private headers it includes, but for the one
    # atomic of the header that is the visibility pass's own (tests/test_mesh_raster_abi.py) -- the header has none
    whole = csrc_text.unit_code("mesh_fit_kernels.hip")
    assert csrc_text.private_headers("mesh_fit_kernels.hip") == ["mesh_raster.h", "view_camera.h", "segment_sum.h"]
    assert "atomic" not in whole.lower() and "hipMemset" not in whole and "__shared__" not in whole and "asm" not in whole
    # the rasteriser's quantities are the rasteriser's: the unit includes the header of its device functions and restates neither the
    # ray's edge values nor the face set-up; no unit is included by anything, and the raster unit keeps its kernels and entry points
    assert csrc_text.includes("mesh_fit_kernels.hip") == ["mesh_raster.h", "segment_sum.h"] and "#define" not in code and "#if" not in whole
    assert "raster_edges(" in code and "raster_hit(" in code and "raster_face(" in code and "load_face(" in code
    assert "float raster_edges(" not in code and "RasterFace raster_face(" not in code and "RasterHit raster_hit(" not in code and "bool load_face(" not in code
    assert "f.c[k]" not in code and "cross_v" not in code and code.count("cross3(") == 3
    header, raster = csrc_text.code("mesh_raster.h"), csrc_text.code("mesh_raster_kernels.hip")
    assert header.count("float raster_edges(") == 1 and header.count("RasterFace raster_face(") == 1 and header.count("void cross3(") == 1
    assert "__global__" not in header and 'extern "C"' not in header and "#if" not in raster and "#define" not in raster
    assert raster.count("__global__") == 3 and 'extern "C"' in raster and "int rf_mesh_raster_taps(" in raster and "float raster_edges(" not in raster


def camera(height=8, width=12, focal=10.0):
    cam = _lib.RFCamera()
    cam.height, cam.width, cam.focal = height, width, focal
    for e in (0, 5, 10):
        cam.pose[e] = 1.0
    return cam


def bad_cameras():
    for kwargs in (dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(focal=0.0), dict(focal=-1.0), dict(focal=NAN), dict(focal=INF)):
        yield camera(**kwargs)
    for value in (NAN, INF):
        bad = camera()
        bad.pose[3] = value
        yield bad


def test_coverage_validates_before_any_launch(lib):
    def call(cam="default", vertices=64, num_vertices=10, faces=128, num_faces=6, visibility=256, flags=0, depth=512, coverage=1024, face_ids=2048):
        cam = camera() if isinstance(cam, str) else cam
        return lib.rf_mesh_raster_coverage(None if cam is None else C.byref(cam), vertices, num_vertices, faces, num_faces, visibility, flags, depth, coverage, face_ids, None)

    for missing in ("cam", "vertices", "faces", "visibility", "depth", "coverage", "face_ids"):
        assert call(**{missing: None}) == NULL, missing
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE and call(num_faces=1 << 31) == SHAPE
    for cam in bad_cameras():
        assert call(cam=cam) == SHAPE
    for flags in (_lib.FLAG_WHITE_BKGD, _lib.FLAG_RENDER_DIFFUSE, _lib.TEXTURE_VIEWS_TWO_SIDED, 1 << 9, _lib.RASTER_CULL_BACKFACES | 4):
        assert call(flags=flags) == UNSUPPORTED
    # the order: pointers < shapes < unsupported
    assert call(coverage=None, num_faces=-1, flags=2) == NULL and call(cam=camera(height=0), flags=2) == SHAPE and call(num_vertices=-1, flags=2) == SHAPE
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0, flags=2) == UNSUPPORTED


def test_backward_pixels_validates_before_any_launch(lib):
    def call(cam="default", vertices=64, num_vertices=10, faces=128, num_faces=6, face_ids=256, coverage=512, grad_depth=1024, grad_coverage=2048, flags=0,
             records=4096, status=8192):
        cam = camera() if isinstance(cam, str) else cam
        return lib.rf_mesh_geometry_backward_pixels(None if cam is None else C.byref(cam), vertices, num_vertices, faces, num_faces, face_ids, coverage, grad_depth,
                                                    grad_coverage, flags, records, status, None)

    for missing in ("cam", "vertices", "faces", "face_ids", "coverage", "grad_depth", "grad_coverage", "records", "status"):
        assert call(**{missing: None}) == NULL, missing
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE and call(num_faces=1 << 31) == SHAPE
    for cam in bad_cameras():
        assert call(cam=cam) == SHAPE
    for flags in (1, 2, 64, 1 << 9, _lib.RASTER_CULL_BACKFACES | 4):
        assert call(flags=flags) == UNSUPPORTED
    assert call(records=None, num_faces=-1, flags=2) == NULL and call(num_faces=-1, flags=2) == SHAPE
    # no faces: every pixel is a miss, RF_OK without a launch (the pointers are not device memory)
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0) == OK and call(vertices=None, num_vertices=0, faces=None, num_faces=0, flags=2) == UNSUPPORTED
    assert call(num_faces=0, flags=_lib.RASTER_CULL_BACKFACES) == OK


def test_backward_gather_validates_before_any_launch(lib):
    def call(records=64, num_pixels=100, hit_pixels=128, num_hits=40, face_offsets=256, num_faces=6, corner_slots=512, vertex_offsets=1024, num_vertices=10,
             long_segment=0, flags=0, face_grads=2048, grad_vertices=4096, status=8192):
        return lib.rf_mesh_geometry_backward_gather(records, num_pixels, hit_pixels, num_hits, face_offsets, num_faces, corner_slots, vertex_offsets, num_vertices,
                                                    long_segment, flags, face_grads, grad_vertices, status, None)

    for missing in ("records", "hit_pixels", "face_offsets", "corner_slots", "vertex_offsets", "face_grads", "grad_vertices", "status"):
        assert call(**{missing: None}) == NULL, missing
    for kwargs in (dict(num_pixels=-1), dict(num_pixels=1 << 31), dict(num_hits=-1), dict(num_hits=101), dict(num_faces=-1), dict(num_faces=(1 << 31) // 3 + 1),
                   dict(num_vertices=-1), dict(num_vertices=1 << 31), dict(long_segment=-1)):
        assert call(**kwargs) == SHAPE, kwargs
    for flags in (1, 2, 32, 64, 1 << 20):
        assert call(flags=flags) == UNSUPPORTED
    assert call(status=None, num_hits=-1, flags=1) == NULL and call(long_segment=-5, flags=1) == SHAPE
    # arrays that a zero count does not need are no errors: these fail only at what comes after
    assert call(records=None, hit_pixels=None, num_hits=0, corner_slots=None, face_grads=None, num_faces=0, grad_vertices=None, num_vertices=0, flags=1) == UNSUPPORTED
    assert call(records=None, hit_pixels=None, num_hits=0, corner_slots=None, face_grads=None, num_faces=0, grad_vertices=None, num_vertices=0, long_segment=-1) == SHAPE
    assert call(records=None, hit_pixels=None, num_hits=0, corner_slots=None, face_grads=None, num_faces=0, grad_vertices=None, num_vertices=0) == OK
