"""rf_mesh_raster_taps, rf_texture_sample, rf_texture_sample_backward: the symbols are exported, the new unit is a build input, the
header declares them, and every argument check of include/relu_field.h comes back as a code before any launch (no GPU needed), in
the documented order."""
import ctypes as C
import os
import re

import pytest

from tests import csrc_text
from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
NAN, INF = float("nan"), float("inf")
NEW = ("rf_mesh_raster_taps", "rf_texture_sample", "rf_texture_sample_backward")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_points(lib):
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "texture_fit_kernels.hip" in _lib.SOURCES and os.path.join(_lib.CSRC_DIR, "texture_fit_kernels.hip") in _lib.build_inputs()
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    for prototype in ("int rf_mesh_raster_taps(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,",
                      "int rf_texture_sample(const void* taps_dev, int64_t num_pixels, const float* texture_dev, int32_t texture_height, int32_t texture_width,",
                      "int rf_texture_sample_backward(const float* grad_colour_dev, int64_t num_pixels, const int64_t* offsets_dev, const void* entries_dev,"):
        assert prototype in header
    assert "uint16_t x0, x1, y0, y1;" in header and "} RFTextureTap; /* 16 bytes */" in header and "} RFTextureTapEntry; /* 8 bytes */" in header
    # the limits the binding names are the ones the unit is compiled with
    source = csrc_text.code("texture_fit_kernels.hip")
    assert re.findall(r"constexpr int kLongSegment = (\d+);", source) == [str(_lib.TEXTURE_FIT_LONG_SEGMENT)]
    assert re.findall(r"constexpr unsigned int kNoTap = 0x([0-9a-f]+)u;", source) == [format(_lib.TEXTURE_NO_TAP, "x")]
    code = csrc_text.unit_code("texture_fit_kernels.hip")  # the unit together with its private headers
    assert csrc_text.private_headers("texture_fit_kernels.hip") == ["segment_sum.h", "view_camera.h"]
    assert re.findall(r"constexpr int kMaxImageEdge = (\d+);", code) == [str(_lib.RASTER_MAX_EDGE)] and _lib.TEXTURE_NO_TAP > _lib.RASTER_MAX_EDGE
    # gather form: no atomics, no memset, no LDS in the unit and its headers; both raster kernels go through the two shared device
    # functions, and the fetch of texture_sample_kernel is the shade kernel's: one bilinear_blend
    assert "atomic" not in code.lower() and "hipMemset" not in code and "__shared__" not in code
    raster, header = csrc_text.code("mesh_raster_kernels.hip"), csrc_text.code("mesh_raster.h")
    assert raster.count("winning_hit(") == 2 and raster.count("texel_taps(") == 2  # two callers each ...
    assert header.count("winning_hit(") == 1 and header.count("texel_taps(") == 1  # ... of one definition, with no separate declaration
    assert header.index("bool winning_hit(") < header.index("BilinearTaps texel_taps(") and "bilinear_taps(" in header[header.index("BilinearTaps texel_taps("):]
    assert source.count("bilinear_blend(") == 1 and raster.count("bilinear_blend(") == 1 and csrc_text.code("view_camera.h").count("float bilinear_blend(") == 1
    for text in (source, raster):
        assert "top" not in text and "bot" not in text  # (neither restates the blend)


def camera(height=8, width=12, focal=10.0):
    cam = _lib.RFCamera()
    cam.height, cam.width, cam.focal = height, width, focal
    for e in (0, 5, 10):
        cam.pose[e] = 1.0
    return cam


def test_taps_validates_before_any_launch(lib):
    def call(cam="default", vertices=64, num_vertices=10, faces=128, num_faces=6, visibility=256, uvs=512, height=6, width=6, flags=0, taps=1024):
        cam = camera() if isinstance(cam, str) else cam
        return lib.rf_mesh_raster_taps(None if cam is None else C.byref(cam), vertices, num_vertices, faces, num_faces, visibility, uvs, height, width, flags, taps, None)

    for missing in ("cam", "vertices", "faces", "visibility", "uvs", "taps"):
        assert call(**{missing: None}) == NULL, missing
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE and call(num_faces=1 << 31) == SHAPE
    for kwargs in (dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(focal=0.0), dict(focal=-1.0), dict(focal=NAN), dict(focal=INF)):
        assert call(cam=camera(**kwargs)) == SHAPE, kwargs
    for value in (NAN, INF):
        bad = camera()
        bad.pose[3] = value
        assert call(cam=bad) == SHAPE
    for kwargs in (dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(height=-1)):
        assert call(**kwargs) == SHAPE, kwargs
    for flags in (_lib.FLAG_RENDER_DIFFUSE, _lib.TEXTURE_VIEWS_TWO_SIDED, 1 << 9, _lib.RASTER_CULL_BACKFACES | 4):
        assert call(flags=flags) == UNSUPPORTED
    # the order: pointers < shapes < unsupported
    assert call(taps=None, height=0, flags=2) == NULL and call(visibility=None, num_faces=-1) == NULL
    assert call(height=0, flags=2) == SHAPE and call(num_vertices=-1, flags=2) == SHAPE
    # arrays that a zero count does not need are no errors: these fail only at what comes after
    assert call(vertices=None, num_vertices=0, faces=None, uvs=None, num_faces=0, flags=2) == UNSUPPORTED
    assert call(vertices=None, num_vertices=0, faces=None, uvs=None, num_faces=0, width=0) == SHAPE


def test_sample_validates_before_any_launch(lib):
    def call(taps=64, num_pixels=100, texture=128, height=6, width=6, background=0.0, flags=0, colour=256, status=512):
        return lib.rf_texture_sample(taps, num_pixels, texture, height, width, background, flags, colour, status, None)

    for missing in ("taps", "texture", "colour", "status"):
        assert call(**{missing: None}) == NULL, missing
    assert call(num_pixels=-1) == SHAPE and call(num_pixels=1 << 31) == SHAPE
    for kwargs in (dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(background=-0.5), dict(background=NAN), dict(background=INF)):
        assert call(**kwargs) == SHAPE, kwargs
    for flags in (1, 2, 32, 64, 1 << 20):
        assert call(flags=flags) == UNSUPPORTED
    assert call(status=None, height=0, flags=1) == NULL and call(texture=None, num_pixels=-1) == NULL
    assert call(height=0, flags=1) == SHAPE and call(background=NAN, flags=1) == SHAPE
    # no pixels: the pixel arrays are not needed, and RF_OK comes back without a launch (the pointers are not device memory)
    assert call(taps=None, colour=None, num_pixels=0, flags=1) == UNSUPPORTED and call(taps=None, colour=None, num_pixels=0, width=0) == SHAPE
    assert call(taps=None, colour=None, num_pixels=0) == OK and call(num_pixels=0, background=0.25) == OK


def test_sample_backward_validates_before_any_launch(lib):
    def call(grad_colour=64, num_pixels=100, offsets=128, entries=256, num_entries=40, height=6, width=6, long_segment=0, flags=0, grad_texture=512, status=1024):
        return lib.rf_texture_sample_backward(grad_colour, num_pixels, offsets, entries, num_entries, height, width, long_segment, flags, grad_texture, status, None)

    for missing in ("grad_colour", "offsets", "entries", "grad_texture", "status"):
        assert call(**{missing: None}) == NULL, missing
    assert call(num_pixels=-1) == SHAPE and call(num_pixels=1 << 31) == SHAPE and call(num_entries=-1) == SHAPE and call(num_entries=1 << 33) == SHAPE
    for kwargs in (dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(long_segment=-1)):
        assert call(**kwargs) == SHAPE, kwargs
    for flags in (1, 2, 32, 64, 1 << 20):
        assert call(flags=flags) == UNSUPPORTED
    assert call(grad_texture=None, height=0, flags=1) == NULL and call(offsets=None, num_entries=-1) == NULL
    assert call(height=0, flags=1) == SHAPE and call(long_segment=-5, flags=1) == SHAPE
    # arrays that a zero count does not need are no errors: these fail only at what comes after
    assert call(grad_colour=None, num_pixels=0, entries=None, num_entries=0, flags=1) == UNSUPPORTED
    assert call(grad_colour=None, num_pixels=0, entries=None, num_entries=0, long_segment=-1) == SHAPE
