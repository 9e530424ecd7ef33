"""rf_label_components: the symbol is exported, the argument checks of include/relu_field.h come back as codes before any launch
(no GPU needed), and the tile edge the binding publishes is the one the kernel unit is compiled with."""
import ctypes as C
import os
import re

import pytest

from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def rf_grid(dims=(4, 4, 4), F=3, layout="split", mode="relu", dens=64, feat=128):
    g = _lib.RFGrid()
    g.densities_dev, g.features_dev = dens, feat
    for a in range(3):
        g.dims[a] = dims[a]
    g.num_features = F
    g.density_stride, g.feature_stride = (1, F) if layout == "reference" else (4, max(F - 3, 0))
    g.density_scale, g.density_mode, g.layout = 1.0, _lib.DENSITY_MODES[mode], _lib.LAYOUTS[layout]
    return g


def test_entry_point(lib):
    assert "rf_label_components" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "rf_label_components")
    assert "component_kernels.hip" in _lib.SOURCES
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert _lib.CONNECTIVITIES == (6, 18, 26)
    source = open(os.path.join(_lib.CSRC_DIR, "component_kernels.hip")).read()
    assert [int(v) for v in re.findall(r"constexpr int kComponentTile = (\d+);", source)] == [_lib.COMPONENT_TILE]
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "int rf_label_components(const RFGrid* grid, float threshold, int32_t connectivity, int32_t* labels_dev, int32_t* sizes_dev, void* stream);" in header
    assert "#define RF_ABI_VERSION 4" in header


def test_validates_before_any_launch(lib):
    def call(grid=None, threshold=0.0, connectivity=26, labels=256, sizes=512, **grid_args):
        g = rf_grid(**grid_args) if grid is None else grid
        return lib.rf_label_components(C.byref(g), threshold, connectivity, labels, sizes, None)

    # check_grid
    assert lib.rf_label_components(None, 0.0, 26, 256, 512, None) == NULL
    assert call(dens=None) == NULL and call(F=12, feat=None) == NULL
    assert call(dims=(0, 4, 4)) == SHAPE and call(dims=(4, 4, 2047)) == SHAPE
    assert call(F=5) == UNSUPPORTED
    bad_mode = rf_grid()
    bad_mode.density_mode = 7
    assert call(grid=bad_mode) == UNSUPPORTED
    # the outputs
    assert call(labels=None) == NULL and call(labels=None, sizes=None) == NULL
    assert call(labels=256, sizes=256) == SHAPE
    # threshold
    assert call(threshold=-1e-6) == SHAPE and call(threshold=float("nan")) == SHAPE and call(threshold=-float("inf")) == SHAPE
    # connectivity
    for connectivity in (0, 4, 7, 8, 27, -26, 124):
        assert call(connectivity=connectivity) == SHAPE
    # more than 2^31 - 1 nodes: 2046 * 2046 * 520 = 2 176 780 320 passes check_grid (< 2^32) and is refused here, on every storage
    for layout in ("reference", "split", "bricked"):
        assert call(dims=(2046, 2046, 520), layout=layout) == SHAPE
        assert call(dims=(520, 2046, 2046), layout=layout, sizes=None) == SHAPE
    # the order of the checks: the grid first, then the pointer, then the numbers
    assert call(dims=(0, 4, 4), labels=None, threshold=-1.0) == SHAPE
    assert call(dens=None, labels=None, connectivity=5) == NULL
    assert call(labels=None, threshold=-1.0, connectivity=5) == NULL
