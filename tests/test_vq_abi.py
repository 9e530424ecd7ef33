"""rf_vq_assign / rf_vq_centroids: both symbols are exported and the argument checks of include/relu_field.h come back as codes
before any launch (no GPU needed)."""
import os

import pytest

from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_points(lib):
    for name in ("rf_vq_assign", "rf_vq_centroids"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "vq_kernels.hip" in _lib.SOURCES
    assert lib.rf_abi_version() == 4
    assert (_lib.VQ_MAX_DIM, _lib.VQ_MAX_CODES) == (64, 65536)


def test_assign_validates_before_any_launch(lib):
    def assign(x=64, M=100, D=27, stride=27, cb=128, Cn=512, index=256, dist=512):
        return lib.rf_vq_assign(x, M, D, stride, cb, Cn, index, dist, None)

    assert assign(x=None) == NULL and assign(cb=None) == NULL and assign(index=None) == NULL and assign(dist=None) == NULL
    for D in (0, -1, 65):
        assert assign(D=D, stride=80) == UNSUPPORTED
    for Cn in (0, -5, 65537):
        assert assign(Cn=Cn) == UNSUPPORTED
    assert assign(M=-1) == SHAPE and assign(stride=26) == SHAPE and assign(stride=0) == SHAPE
    assert assign(index=512) == SHAPE and assign(index=64) == SHAPE and assign(dist=128) == SHAPE  # an output that is another array
    assert assign(x=None, D=65) == NULL  # a null pointer comes first
    assert assign(D=65, stride=10) == UNSUPPORTED  # ... then the sizes
    # no vectors: a no-op, whatever the vector and output pointers are -- but still validated
    assert assign(M=0) == OK and assign(M=0, x=None, index=None, dist=None) == OK
    assert assign(M=0, cb=None) == NULL and assign(M=0, D=0) == UNSUPPORTED and assign(M=0, stride=3) == SHAPE


def test_centroids_validate_before_any_launch(lib):
    def centroids(x=64, stride=27, D=27, w=128, order=256, offsets=512, Cn=512, cb=1024, sums=2048):
        return lib.rf_vq_centroids(x, stride, D, w, order, offsets, Cn, cb, sums, None)

    for name in ("x", "w", "order", "offsets", "cb"):
        assert centroids(**{name: None}) == NULL
    for D in (0, 65):
        assert centroids(D=D, stride=80) == UNSUPPORTED
    for Cn in (0, 65537):
        assert centroids(Cn=Cn) == UNSUPPORTED
    assert centroids(stride=26) == SHAPE
    assert centroids(cb=64) == SHAPE and centroids(sums=1024) == SHAPE and centroids(sums=128) == SHAPE and centroids(cb=512) == SHAPE
    assert centroids(x=None, D=65) == NULL
