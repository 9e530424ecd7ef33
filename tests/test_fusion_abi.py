"""rf_fuse_depth_views: the symbol is exported and declared, its unit is a build input free of atomics, LDS and inline assembly, and
the argument checks of include/relu_field.h come back as codes, in the documented order, before any launch (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

from tests import csrc_text
from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
UNIT = "fusion_kernels.hip"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_point(lib):
    assert "rf_fuse_depth_views" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "rf_fuse_depth_views")
    assert UNIT in _lib.SOURCES and os.path.join(_lib.CSRC_DIR, UNIT) in _lib.build_inputs()
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    assert "enum { RF_FUSE_CARVE = 128 };" in header and _lib.FUSE_CARVE == 128
    assert ("int rf_fuse_depth_views(const float* aabb_min, const float* aabb_max, const int32_t* dims, int32_t num_views, const RFCamera* cameras,\n"
            "                        const float* depths_dev, const float* alphas_dev, const float* images_dev, float near, float truncation, float min_alpha,\n"
            "                        uint32_t flags, float* tsdf_sum_dev, int32_t* counts_dev, float* colour_sum_dev, void* stream);") in header
    assert len(lib.rf_fuse_depth_views.argtypes) == 16
    source = csrc_text.unit_code(UNIT)  # the unit together with its private header
    assert [int(v) for v in re.findall(r"constexpr int kMaxViews = (\d+);", source)] == [_lib.FUSE_MAX_VIEWS]
    assert [int(v) for v in re.findall(r"constexpr int kMaxViews = (\d+);", csrc_text.code("view_camera.h"))] == [_lib.FUSE_MAX_VIEWS]
    assert [int(v) for v in re.findall(r"constexpr int kMaxDim = (\d+);", csrc_text.code(UNIT))] == [_lib.FUSE_MAX_DIM]


def test_the_unit_has_no_atomics_no_lds_and_no_assembly():
    code = csrc_text.unit_code(UNIT)  # the unit together with its private header
    assert "__global__" in code
    for word in ("atomic", "__shared__", "asm", "__syncthreads", "__builtin_amdgcn"):
        assert word not in code, word
    assert csrc_text.includes(UNIT) == ["view_camera.h"] and csrc_text.includes("view_camera.h") == ["rf_device.h"]
    assert os.path.join(_lib.CSRC_DIR, "view_camera.h") in _lib.build_inputs()


def camera(height=8, width=8, focal=10.0, pose=(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4)):
    cam = _lib.RFCamera()
    cam.height, cam.width, cam.focal = height, width, focal
    for i, v in enumerate(pose):
        cam.pose[i] = float(v)
    return cam


def test_validates_in_the_documented_order_before_any_launch(lib):
    """every pointer below is a made-up address: a launch, or any device access, would fault"""
    f3 = _lib.float3

    def call(lo=(-1, -1, -1), hi=(1, 1, 1), dims=(4, 4, 4), views=1, cams="default", depths=4096, alphas=None, images=None, near=0.0, truncation=0.5,
             min_alpha=0.5, flags=_lib.FUSE_CARVE, tsdf=8192, counts=16384, colour=None):
        if cams == "default":
            cams = [camera()] * max(views, 1)
        cam_array = None if cams is None else (_lib.RFCamera * len(cams))(*cams)
        return lib.rf_fuse_depth_views(None if lo is None else f3(lo), None if hi is None else f3(hi), None if dims is None else (C.c_int32 * 3)(*dims), views, cam_array,
                                       depths, alphas, images, near, truncation, min_alpha, flags, tsdf, counts, colour, None)

    nan, inf = float("nan"), float("inf")
    # 1. pointers
    assert call(lo=None) == NULL and call(hi=None) == NULL and call(dims=None) == NULL and call(tsdf=None) == NULL and call(counts=None) == NULL
    assert call(cams=None) == NULL and call(depths=None) == NULL
    assert call(images=32768) == NULL and call(images=32768, colour=65536, views=0) == OK
    # 2. shapes, in the header's order
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 4097), (2048, 2048, 512)):
        assert call(dims=dims) == SHAPE
    assert call(dims=(2048, 2048, 511), views=0) == OK  # 2^31 - 2^22 nodes
    assert call(lo=(nan, -1, -1)) == SHAPE and call(hi=(1, inf, 1)) == SHAPE and call(lo=(-1, 1, -1)) == SHAPE and call(lo=(-1, -1, 2)) == SHAPE
    assert call(lo=(-3e38, -1, -1), hi=(3e38, 1, 1)) == SHAPE  # an extent that overflows
    assert call(views=-1) == SHAPE and call(views=17, cams=[camera()] * 17) == SHAPE
    assert call(cams=[camera(height=0)]) == SHAPE and call(cams=[camera(width=16385)]) == SHAPE
    assert call(views=2, cams=[camera(), camera(height=9)]) == SHAPE
    assert call(cams=[camera(focal=0.0)]) == SHAPE and call(cams=[camera(focal=nan)]) == SHAPE and call(cams=[camera(focal=inf)]) == SHAPE
    assert call(cams=[camera(pose=(1, 0, 0, 0, 0, 1, 0, nan, 0, 0, 1, 4))]) == SHAPE
    assert call(near=-1e-6) == SHAPE and call(near=nan) == SHAPE and call(near=inf) == SHAPE
    assert call(truncation=0.0) == SHAPE and call(truncation=-0.5) == SHAPE and call(truncation=nan) == SHAPE and call(truncation=inf) == SHAPE
    assert call(min_alpha=-0.01) == SHAPE and call(min_alpha=1.01) == SHAPE and call(min_alpha=nan) == SHAPE
    assert call(counts=16388) == SHAPE and call(images=32768, colour=65544) == SHAPE  # accumulators read as 8 and 16 bytes
    # 3. flags
    for flags in (1, 64, 256, _lib.FUSE_CARVE | 2, 1 << 31):
        assert call(flags=flags, views=0) == UNSUPPORTED
    # the order: pointers before shapes before flags
    assert call(tsdf=None, dims=(0, 4, 4), flags=1) == NULL
    assert call(depths=None, truncation=-1.0) == NULL
    assert call(images=32768, views=17, flags=1) == NULL
    assert call(dims=(0, 4, 4), flags=1) == SHAPE and call(truncation=nan, flags=3) == SHAPE and call(min_alpha=2.0, flags=1) == SHAPE
    assert call(dims=(0, 4, 4), lo=(nan, 0, 0), views=99) == SHAPE
    # no views: RF_OK without a launch, with or without the optional arrays, cameras and depths
    assert call(views=0) == OK and call(views=0, cams=None, depths=None) == OK and call(views=0, flags=0) == OK
    assert call(views=0, min_alpha=0.0) == OK and call(views=0, min_alpha=1.0) == OK and call(views=0, near=0.0) == OK
