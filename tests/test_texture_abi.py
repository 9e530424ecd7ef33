"""rf_texture_bake: the symbol is exported, the unit is a build input, the header declares it, and every argument check of
include/relu_field.h comes back as a code before any launch (no GPU needed), in the documented order."""
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
    assert "rf_texture_bake" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "rf_texture_bake")
    assert "texture_kernels.hip" in _lib.SOURCES
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    assert "int rf_texture_bake(const RFGrid* grid, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, int32_t patch," in header
    # the limits the binding checks are the ones the unit is compiled with
    source = open(os.path.join(_lib.CSRC_DIR, "texture_kernels.hip")).read()
    assert re.findall(r"constexpr int kMinPatch = (\d+), kMaxPatch = (\d+);", source) == [(str(_lib.TEXTURE_MIN_PATCH), str(_lib.TEXTURE_MAX_PATCH))]
    assert re.findall(r"constexpr int kMaxSamples = (\d+);", source) == [str(_lib.TEXTURE_MAX_SAMPLES)]
    assert re.findall(r"constexpr int kMaxImageEdge = (\d+);", csrc_text.unit_code("texture_kernels.hip")) == [str(_lib.TEXTURE_MAX_EDGE)]  # (view_camera.h's)
    assert "const int block = patch + 4;" in source and _lib.TEXTURE_GUTTER == 4
    # one lane per texel, every texel written once: no atomics in the unit, and the addressing comes from the shared header
    code = re.sub(r"//.*", "", source)
    assert "atomic" not in code.lower()
    for helper in ("query_cell(", "query_corner(", "query_offset(", "density_post(", "sh_basis<", "sigmoidf_("):
        assert helper in code
    assert "node_lin" not in code and "hipMemset" not in code


def make_grid(F=27, layout="split", dims=(8, 8, 8)):
    g = _lib.RFGrid()
    g.densities_dev, g.features_dev = 1 << 20, 1 << 21
    for a in range(3):
        g.dims[a] = dims[a]
        g.aabb_min[a], g.aabb_max[a] = -1.0, 1.0
        g.norm_scale[a], g.norm_bias[a] = 1.0, 0.0
    g.num_features = F
    g.density_stride, g.feature_stride = (1, F) if layout == "reference" else (4, F - 3)
    g.layout = _lib.LAYOUTS[layout]
    g.density_scale, g.density_mode = 1.0, 0
    return g


def test_validates_before_any_launch(lib):
    def call(grid="default", vertices=64, num_vertices=10, faces=128, num_faces=6, patch=8, cols=2, rows=2, reach=0.5, samples=16, flags=0, texture=256,
             opacity=512, status=1024):
        g = make_grid() if grid == "default" else grid
        return lib.rf_texture_bake(None if g is None else C.byref(g), vertices, num_vertices, faces, num_faces, patch, cols, rows, reach, samples, flags,
                                   texture, opacity, status, None)

    # null pointers
    assert call(grid=None) == NULL
    no_tensor = make_grid()
    no_tensor.densities_dev = None
    assert call(grid=no_tensor) == NULL
    for missing in ("vertices", "faces", "texture", "status"):
        assert call(**{missing: None}) == NULL
    # shapes
    assert call(num_vertices=-1) == SHAPE and call(num_faces=-1) == SHAPE
    for patch in (1, 0, -8, 65):
        assert call(patch=patch) == SHAPE
    for samples in (0, -1, 257):
        assert call(samples=samples) == SHAPE
    for reach in (-0.5, NAN, INF, -INF):
        assert call(reach=reach) == SHAPE
    assert call(cols=0) == SHAPE and call(rows=0) == SHAPE and call(cols=-2) == SHAPE
    assert call(cols=1366, rows=1) == SHAPE and call(cols=1, rows=1366, num_faces=2) == SHAPE  # 1366 * 12 = 16392 texels
    assert call(patch=64, cols=241, rows=1) == SHAPE                                          # 241 * 68 = 16388
    assert call(num_faces=9) == SHAPE                                                         # 2 * 2 * 2 = 8 places
    bad_dims = make_grid(dims=(0, 8, 8))
    assert call(grid=bad_dims) == SHAPE
    # unsupported: flag bits other than RENDER_DIFFUSE, a feature count that is no SH degree
    for flags in (_lib.FLAG_WHITE_BKGD, _lib.FLAG_AABB_SAMPLING, _lib.FLAG_OCCUPANCY_SKIP, _lib.FLAG_JITTER_KEYED, 1 << 9,
                  _lib.FLAG_RENDER_DIFFUSE | _lib.FLAG_WHITE_BKGD):
        assert call(flags=flags) == UNSUPPORTED
    assert call(grid=make_grid(F=5, layout="reference")) == UNSUPPORTED
    # the order: pointers < shapes < unsupported
    assert call(texture=None, patch=1, flags=1) == NULL
    assert call(status=None, num_faces=-1) == NULL
    assert call(patch=1, flags=1) == SHAPE and call(reach=NAN, flags=4) == SHAPE and call(num_faces=9, flags=1) == SHAPE
    assert call(grid=bad_dims, faces=None) == NULL and call(grid=bad_dims, flags=1) == SHAPE
    # an optional opacity image and arrays that a zero count does not need are no errors: these fail only at what comes after
    assert call(opacity=None, patch=1) == SHAPE and call(opacity=None, flags=1) == UNSUPPORTED
    assert call(vertices=None, num_vertices=0, faces=None, num_faces=0, flags=1) == UNSUPPORTED
