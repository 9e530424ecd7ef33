"""rf_ssim_tiles / rf_ssim_forward / rf_ssim_backward: the argument checks of include/relu_field.h come back as codes before any device
access (no GPU needed), and the binding mirrors RFImage."""
import ctypes as C
import os

import pytest

from thr3ed_atom_amd import _lib

NULL, SHAPE, UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _image(ptr=64, strides=(90, 3, 1)):
    im = _lib.RFImage()
    im.data_dev = ptr
    im.stride_h, im.stride_w, im.stride_c = strides
    return im


def test_entry_points_and_struct(lib):
    for name in ("rf_ssim_tiles", "rf_ssim_forward", "rf_ssim_backward"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.rf_abi_version() == 4
    assert _lib.ABI_STRUCTS.index(_lib.RFImage) == 11 and lib.rf_abi_struct_size(11) == C.sizeof(_lib.RFImage) == 32
    assert lib.rf_abi_struct_size(12) == -1


def test_tile_counts(lib):
    th, tw = _lib.SSIM_TILE
    assert lib.rf_ssim_tiles(11, 11, 1, 0) == 1 and lib.rf_ssim_tiles(1, 1, 3, 1) == 3
    assert lib.rf_ssim_tiles(th + 10, tw + 10, 3, 0) == 3 and lib.rf_ssim_tiles(th + 11, tw + 10, 3, 0) == 6 and lib.rf_ssim_tiles(th + 10, tw + 11, 3, 0) == 6
    assert lib.rf_ssim_tiles(th, tw, 1, 1) == 1 and lib.rf_ssim_tiles(th + 1, tw + 1, 1, 1) == 4
    assert lib.rf_ssim_tiles(800, 800, 3, 0) == 3 * 50 * 25
    assert lib.rf_ssim_tiles(10, 30, 3, 0) == SHAPE and lib.rf_ssim_tiles(30, 10, 3, 0) == SHAPE and lib.rf_ssim_tiles(10, 30, 3, 1) == 3
    assert lib.rf_ssim_tiles(0, 30, 3, 1) == SHAPE and lib.rf_ssim_tiles(30, 30, 0, 1) == SHAPE
    assert lib.rf_ssim_tiles(30, 30, 3, 2) == UNSUPPORTED and lib.rf_ssim_tiles(30, 30, 3, -1) == UNSUPPORTED


def test_forward_validates_before_any_launch(lib):
    x, y = _image(), _image()
    ok = (64, 64, 64, 64)  # map, derivative maps, partials, mean

    def fwd(a, b, H=30, W=30, Cn=3, padding=0, outs=ok):
        return lib.rf_ssim_forward(None if a is None else C.byref(a), None if b is None else C.byref(b), H, W, Cn, padding, *outs, None)

    assert fwd(None, y) == NULL and fwd(x, None) == NULL
    assert fwd(_image(ptr=None), y) == NULL and fwd(x, _image(ptr=None)) == NULL
    assert fwd(x, y, outs=(64, 64, None, 64)) == NULL and fwd(x, y, outs=(64, 64, 64, None)) == NULL  # partials, mean
    for H, W, Cn in ((0, 30, 3), (30, 0, 3), (30, 30, 0), (-1, 30, 3)):
        assert fwd(x, y, H, W, Cn) == SHAPE
    assert fwd(x, y, 10, 30) == SHAPE and fwd(x, y, 30, 10) == SHAPE  # "valid" below 11
    for strides in ((0, 3, 1), (90, 0, 1), (90, 3, 0)):
        assert fwd(_image(strides=strides), y) == SHAPE and fwd(x, _image(strides=strides)) == SHAPE
    assert fwd(x, y, padding=2) == UNSUPPORTED and fwd(x, y, padding=-1) == UNSUPPORTED
    assert fwd(None, _image(strides=(0, 3, 1))) == NULL  # a null pointer comes before a bad stride


def test_backward_validates_before_any_launch(lib):
    x, y, g = _image(), _image(), _image(ptr=128)

    def bwd(a, b, c, H=30, W=30, Cn=3, padding=1, dmaps=64, gout=64):
        ref = lambda im: None if im is None else C.byref(im)  # noqa: E731
        return lib.rf_ssim_backward(ref(a), ref(b), H, W, Cn, padding, dmaps, gout, ref(c), None)

    assert bwd(None, y, g) == NULL and bwd(x, None, g) == NULL and bwd(x, y, None) == NULL and bwd(x, y, _image(ptr=None)) == NULL
    assert bwd(x, y, g, dmaps=None) == NULL and bwd(x, y, g, gout=None) == NULL
    assert bwd(x, y, g, H=0) == SHAPE and bwd(x, y, g, Cn=0) == SHAPE
    assert bwd(x, y, g, H=10, padding=0) == SHAPE
    assert bwd(x, y, _image(ptr=128, strides=(90, 3, 0))) == SHAPE
    assert bwd(x, y, g, padding=7) == UNSUPPORTED
