"""rf_mesh_raster_visibility / rf_mesh_raster_shade: the symbols are exported, the unit is a build input, the header declares them, and
every argument check of include/relu_field.h comes back as a code before any launch (no GPU needed), in the documented order."""
import ctypes as C
import os
import re

import pytest

from tests import csrc_text
from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_points(lib):
    for name in ("rf_mesh_raster_visibility", "rf_mesh_raster_shade"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "mesh_raster_kernels.hip" in _lib.SOURCES
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    assert "int rf_mesh_raster_visibility(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces," in header
    assert "int rf_mesh_raster_shade(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces," in header
    assert f"enum {{ RF_RASTER_CULL_BACKFACES = {_lib.RASTER_CULL_BACKFACES} }};" in header
    assert _lib.RASTER_CULL_BACKFACES not in (_lib.FLAG_WHITE_BKGD, _lib.FLAG_RENDER_DIFFUSE, _lib.FLAG_AABB_SAMPLING, _lib.FLAG_OCCUPANCY_SKIP, _lib.FLAG_JITTER_KEYED)
    # the limits the binding checks are the ones the unit is compiled with (they live in the private headers the unit includes)
    assert csrc_text.private_headers("mesh_raster_kernels.hip") == ["mesh_raster.h", "view_camera.h"]
    assert os.path.join(_lib.CSRC_DIR, "mesh_raster.h") in _lib.build_inputs() and os.path.join(_lib.CSRC_DIR, "view_camera.h") in _lib.build_inputs()
    assert re.findall(r"constexpr int kMaxImageEdge = (\d+);", csrc_text.code("view_camera.h")) == [str(_lib.RASTER_MAX_EDGE)]
    assert re.findall(r"constexpr int kLaneBox = (\d+);", csrc_text.code("mesh_raster.h")) == [str(_lib.RASTER_LANE_BOX)]
    code = csrc_text.unit_code("mesh_raster_kernels.hip")  # the unit together with its private headers
    assert len(re.findall(r"constexpr int kMaxImageEdge = ", code)) == len(re.findall(r"constexpr int kLaneBox = ", code)) == 1
    # the ray is cast_rays' own, the only atomic is the 64-bit minimum of the visibility pass, and nothing needs LDS or a barrier
    assert "pixel_ray(" in code and "-ffp-contract=off" in _lib.HIPCC_FLAGS
    assert re.findall(r"__hip_atomic_fetch_\w+|atomic[A-Z]\w+", code) == ["__hip_atomic_fetch_min"]
    # the shade kernel has no atomic and takes its hit from raster_hit and raster_face, through winning_hit of the header
    unit = csrc_text.code("mesh_raster_kernels.hip")
    shade = unit[unit.index("void mesh_raster_shade_kernel"):unit.index("void mesh_raster_taps_kernel")]
    assert "atomic" not in shade.lower() and "winning_hit(" in shade and "texel_taps(" in shade and "bilinear_blend(" in shade
    header = csrc_text.code("mesh_raster.h")
    winning_hit = header[header.index("bool winning_hit("):header.index("BilinearTaps texel_taps(")]
    assert "raster_hit(" in winning_hit and "raster_face(" in winning_hit and "load_face(" in winning_hit and "winning_key(" in winning_hit and "atomic" not in header.lower()
    assert "int check_raster(" in header and "check_raster(" in unit and "int check_raster(" not in unit
    assert "__shared__" not in code and "__syncthreads" not in code and "hipMemset" not in code


def make_camera(height=24, width=40, focal=30.0, pose=None):
    cam = _lib.RFCamera()
    cam.height, cam.width, cam.focal = height, width, focal
    for k, x in enumerate(pose or (1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3)):
        cam.pose[k] = x
    return cam


def test_visibility_validates_before_any_launch(lib):
    def call(camera="default", vertices=64, num_vertices=10, faces=128, num_faces=6, near=0.0, flags=0, visibility=256, status=1024):
        cam = make_camera() if camera == "default" else camera
        return lib.rf_mesh_raster_visibility(None if cam is None else C.byref(cam), vertices, num_vertices, faces, num_faces, near, flags, visibility, status, None)

    # null pointers
    for missing in ("camera", "vertices", "faces", "visibility", "status"):
        assert call(**{missing: None}) == NULL
    # shapes
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE and call(num_faces=2**31) == SHAPE and call(num_faces=2**40) == SHAPE
    for edge in (0, -1, 16385):
        assert call(camera=make_camera(height=edge)) == SHAPE and call(camera=make_camera(width=edge)) == SHAPE
    for focal in (0.0, -30.0, NAN, INF, -INF):
        assert call(camera=make_camera(focal=focal)) == SHAPE
    for bad in (NAN, INF):
        for k in (0, 5, 11):
            pose = [1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3]
            pose[k] = bad
            assert call(camera=make_camera(pose=pose)) == SHAPE
    for near in (-0.5, NAN, INF, -INF):
        assert call(near=near) == SHAPE
    # unsupported: flag bits other than WHITE_BKGD (ignored here) and CULL_BACKFACES
    for flags in (_lib.FLAG_RENDER_DIFFUSE, _lib.FLAG_AABB_SAMPLING, _lib.FLAG_OCCUPANCY_SKIP, _lib.FLAG_JITTER_KEYED, 1 << 6, 1 << 31,
                  _lib.RASTER_CULL_BACKFACES | _lib.FLAG_RENDER_DIFFUSE):
        assert call(flags=flags) == UNSUPPORTED
    # the order: pointers < shapes < unsupported
    assert call(visibility=None, num_faces=-1, flags=2) == NULL and call(status=None, near=NAN) == NULL
    assert call(faces=None, camera=make_camera(height=0)) == NULL
    assert call(num_faces=-1, flags=2) == SHAPE and call(near=-1.0, flags=4) == SHAPE and call(camera=make_camera(focal=0.0), flags=64) == SHAPE
    # arrays that a zero count does not need are no errors, and an empty mesh is done without a launch
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0, flags=2) == UNSUPPORTED
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0) == OK and call(num_faces=0, faces=None) == OK
    for flags in (_lib.FLAG_WHITE_BKGD, _lib.RASTER_CULL_BACKFACES, _lib.FLAG_WHITE_BKGD | _lib.RASTER_CULL_BACKFACES):
        assert call(num_faces=0, flags=flags) == OK
    assert call(num_faces=0, camera=make_camera(height=16384, width=1)) == OK and call(num_faces=0, camera=make_camera(height=1, width=16384), near=3.0) == OK


def test_shade_validates_before_any_launch(lib):
    def call(camera="default", vertices=64, num_vertices=10, faces=128, num_faces=6, visibility=256, uvs=512, texture=1024, texture_height=12, texture_width=18,
             colours=2048, flags=0, colour=4096, depth=8192, face_ids=16384, barycentrics=32768):
        cam = make_camera() if camera == "default" else camera
        return lib.rf_mesh_raster_shade(None if cam is None else C.byref(cam), vertices, num_vertices, faces, num_faces, visibility, uvs, texture, texture_height,
                                        texture_width, colours, flags, colour, depth, face_ids, barycentrics, None)

    # null pointers (every check below fails at a later one, here the unknown flag bit: nothing is launched on this machine)
    for missing in ("camera", "vertices", "faces", "visibility", "depth", "face_ids"):
        assert call(**{missing: None}, flags=2) == NULL
    assert call(uvs=None, flags=2) == NULL and call(texture=None, flags=2) == NULL                # the bake comes by halves
    assert call(uvs=None, texture=None, colours=None, flags=2) == NULL                          # a colour image without a source
    # optional arrays
    assert call(uvs=None, texture=None, flags=2) == UNSUPPORTED and call(colours=None, flags=2) == UNSUPPORTED
    assert call(uvs=None, texture=None, colours=None, colour=None, flags=2) == UNSUPPORTED and call(barycentrics=None, flags=2) == UNSUPPORTED
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0, flags=2) == UNSUPPORTED
    # shapes
    assert call(num_vertices=-1, flags=2) == SHAPE and call(num_faces=-1, flags=2) == SHAPE and call(num_faces=2**31, flags=2) == SHAPE
    for edge in (0, -1, 16385):
        assert call(camera=make_camera(height=edge)) == SHAPE and call(camera=make_camera(width=edge)) == SHAPE
        assert call(texture_height=edge) == SHAPE and call(texture_width=edge) == SHAPE
        assert call(uvs=None, texture=None, texture_height=edge, flags=2) == UNSUPPORTED  # (no texture: its size is not looked at)
    for focal in (0.0, -30.0, NAN, INF):
        assert call(camera=make_camera(focal=focal)) == SHAPE
    pose = [1, 0, 0, 0.1, 0, 1, 0, NAN, 0, 0, 1, 0.3]
    assert call(camera=make_camera(pose=pose)) == SHAPE
    # unsupported
    for flags in (_lib.FLAG_RENDER_DIFFUSE, _lib.FLAG_AABB_SAMPLING, _lib.FLAG_OCCUPANCY_SKIP, _lib.FLAG_JITTER_KEYED, 1 << 6, _lib.FLAG_WHITE_BKGD | 2):
        assert call(flags=flags) == UNSUPPORTED
    # the order
    assert call(depth=None, num_faces=-1, flags=2) == NULL and call(texture=None, texture_height=0) == NULL
    assert call(texture_width=0, flags=2) == SHAPE and call(camera=make_camera(width=0), flags=2) == SHAPE
