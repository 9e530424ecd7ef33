"""rf_texture_project_views: the symbol is exported, the unit and the shared atlas header are build inputs, the header declares it, and
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


def test_entry_point(lib):
    assert "rf_texture_project_views" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "rf_texture_project_views")
    assert "texture_views_kernels.hip" in _lib.SOURCES
    assert os.path.join(_lib.CSRC_DIR, "texture_atlas.h") in _lib.build_inputs()
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    assert "int rf_texture_project_views(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, int32_t patch, int32_t cols," in header
    assert re.findall(r"enum \{ RF_TEXTURE_VIEWS_TWO_SIDED = (\d+) \};", header) == [str(_lib.TEXTURE_VIEWS_TWO_SIDED)]
    assert _lib.TEXTURE_VIEWS_TWO_SIDED not in (_lib.FLAG_WHITE_BKGD, _lib.FLAG_RENDER_DIFFUSE, _lib.FLAG_AABB_SAMPLING, _lib.FLAG_OCCUPANCY_SKIP,
                                                _lib.FLAG_JITTER_KEYED, _lib.RASTER_CULL_BACKFACES)
    # the limits the binding checks are the ones the unit is compiled with
    source = csrc_text.unit_code("texture_views_kernels.hip")  # the unit together with its private headers
    assert csrc_text.private_headers("texture_views_kernels.hip") == ["texture_atlas.h", "view_camera.h"]
    assert os.path.join(_lib.CSRC_DIR, "view_camera.h") in _lib.build_inputs()
    assert re.findall(r"constexpr int kMaxViews = (\d+);", source) == [str(_lib.TEXTURE_VIEWS_MAX_VIEWS)]
    assert re.findall(r"constexpr int kMaxViews = (\d+);", csrc_text.code("view_camera.h")) == [str(_lib.TEXTURE_VIEWS_MAX_VIEWS)]
    assert re.findall(r"constexpr int kMaxCosPower = (\d+);", source) == [str(_lib.TEXTURE_VIEWS_MAX_COS_POWER)]
    assert re.findall(r"constexpr int kMinPatch = (\d+), kMaxPatch = (\d+);", source) == [(str(_lib.TEXTURE_MIN_PATCH), str(_lib.TEXTURE_MAX_PATCH))]
    assert re.findall(r"constexpr int kMaxImageEdge = (\d+);", source) == [str(_lib.TEXTURE_MAX_EDGE)]
    assert C.sizeof(_lib.RFCamera) == 60  # 16 of them travel in the kernel's argument struct
    # one lane per texel, load-add-store: no atomics and no memset in the unit; the atlas map is the shared one in both units
    code = source
    assert "atomic" not in code.lower() and "hipMemset" not in code
    own = csrc_text.code("texture_views_kernels.hip")
    assert "bilinear_taps(" in own and "bilinear_blend(" in own and "floorf" not in own and "fill_view_cameras(" in own and "view_cameras_ok(" in own
    bake = csrc_text.code("texture_kernels.hip")
    for unit in (own, bake):
        assert '#include "texture_atlas.h"' in unit
        for helper in ("atlas_texel(", "atlas_face(", "atlas_point("):
            assert helper in unit


def cameras(n=2, height=8, width=12, focal=10.0):
    cams = (_lib.RFCamera * max(n, 1))()
    for k in range(n):
        cams[k].height, cams[k].width, cams[k].focal = height, width, focal
        for e in (0, 5, 10):
            cams[k].pose[e] = 1.0
    return cams


def test_validates_before_any_launch(lib):
    def call(vertices=64, num_vertices=10, faces=128, num_faces=6, patch=8, cols=2, rows=2, num_views=2, cams="default", images=256, visibility=512, alphas=768,
             near=0.0, depth_bias=0.1, min_cos=0.1, cos_power=2, background=0.0, flags=0, accum=1024, count=2048, status=4096):
        cams = cameras(max(num_views, 0)) if isinstance(cams, str) else cams
        return lib.rf_texture_project_views(vertices, num_vertices, faces, num_faces, patch, cols, rows, num_views, cams, images, visibility, alphas, near, depth_bias,
                                            min_cos, cos_power, background, flags, accum, count, status, None)

    two = _lib.TEXTURE_VIEWS_TWO_SIDED
    # null pointers
    for missing in ("vertices", "faces", "cams", "images", "visibility", "accum", "status"):
        assert call(**{missing: None}) == NULL, missing
    # shapes
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE
    assert call(num_views=-1) == SHAPE and call(num_views=17, cams=cameras(17)) == SHAPE
    for patch in (1, 0, -8, 65):
        assert call(patch=patch) == SHAPE
    assert call(cols=0) == SHAPE and call(rows=0) == SHAPE and call(cols=-2) == SHAPE
    assert call(cols=1366, rows=1) == SHAPE and call(cols=1, rows=1366, num_faces=2) == SHAPE  # 1366 * 12 = 16392 texels
    assert call(patch=64, cols=241, rows=1) == SHAPE                                          # 241 * 68 = 16388
    assert call(num_faces=9) == SHAPE                                                         # 2 * 2 * 2 = 8 places
    for kwargs in (dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(focal=0.0), dict(focal=-1.0), dict(focal=NAN), dict(focal=INF)):
        assert call(cams=cameras(2, **kwargs)) == SHAPE, kwargs
    unequal = cameras(2)
    unequal[1].width = 13
    assert call(cams=unequal) == SHAPE
    for entry in (0, 3, 11):
        for value in (NAN, INF):
            bad_pose = cameras(2)
            bad_pose[1].pose[entry] = value
            assert call(cams=bad_pose) == SHAPE
    for name in ("near", "depth_bias", "background"):
        for value in (-0.5, NAN, INF, -INF):
            assert call(**{name: value}) == SHAPE, (name, value)
    for min_cos in (-0.1, 1.0, 1.5, NAN, INF):
        assert call(min_cos=min_cos) == SHAPE
    for cos_power in (-1, 9):
        assert call(cos_power=cos_power) == SHAPE
    # unsupported: every flag bit but RF_TEXTURE_VIEWS_TWO_SIDED
    for flags in (_lib.FLAG_WHITE_BKGD, _lib.FLAG_RENDER_DIFFUSE, _lib.RASTER_CULL_BACKFACES, 1 << 9, two | _lib.FLAG_WHITE_BKGD):
        assert call(flags=flags) == UNSUPPORTED
    # the order: pointers < shapes < unsupported
    assert call(accum=None, patch=1, flags=1) == NULL and call(status=None, num_faces=-1) == NULL and call(images=None, min_cos=2.0) == NULL
    assert call(patch=1, flags=1) == SHAPE and call(near=NAN, flags=4) == SHAPE and call(num_faces=9, flags=1) == SHAPE and call(cams=unequal, flags=1) == SHAPE
    # optional arrays, and arrays that a zero count does not need, are no errors: these fail only at what comes after, or not at all
    assert call(alphas=None, count=None, patch=1) == SHAPE and call(alphas=None, count=None, flags=1) == UNSUPPORTED
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0, flags=1) == UNSUPPORTED
    assert call(num_views=0, cams=None, images=None, visibility=None, flags=1) == UNSUPPORTED
    # nothing to do: RF_OK without a launch (the pointers are not device memory)
    assert call(num_views=0, cams=None, images=None, visibility=None) == OK and call(num_views=0, flags=two) == OK
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0) == OK and call(num_faces=0, flags=two, min_cos=0.0, cos_power=0) == OK
