"""rf_mesh_closest_gradients: the symbol is exported and declared, its unit and private header are build inputs that sit over the one
distance rule of mesh_distance.h, free of atomics, LDS, barriers, inline assembly, builtins and macros, and the argument checks of
include/relu_field.h come back as codes, in the documented order, before any launch (no GPU needed)."""
import os
import re

import pytest

from tests import csrc_text
from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
UNIT, HEADER, RULE = "mesh_distance_grad_kernels.hip", "mesh_distance_grad.h", "mesh_distance.h"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entry_point(lib):
    assert "rf_mesh_closest_gradients" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "rf_mesh_closest_gradients")
    assert len(_lib.EXPORTED_SYMBOLS) == 69 and len(set(_lib.EXPORTED_SYMBOLS)) == 69
    inputs = _lib.build_inputs()
    assert UNIT in _lib.SOURCES and os.path.join(_lib.CSRC_DIR, UNIT) in inputs and os.path.join(_lib.CSRC_DIR, HEADER) in inputs
    assert lib.rf_abi_version() == 4 and _lib.ABI_VERSION == 4
    header = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    assert "#define RF_ABI_VERSION 4" in header
    assert ("int rf_mesh_closest_gradients(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,\n"
            "                              const float* points_dev, const int64_t* face_dev, const float* grad_distance_dev, int64_t num_points,\n"
            "                              uint32_t flags, float* grad_points_dev, float* records_dev, float* barycentrics_dev,\n"
            "                              int32_t* region_dev, int32_t* status_dev, void* stream);") in header
    for phrase in ("dL/dp = G u", "dL/d(corner k) = -beta_k G u", "S = (E_ab + E_bc) + E_ca, beta_c = E_ab / S, beta_a = E_bc / S, beta_b = E_ca / S"):
        assert phrase in header, phrase
    assert len(lib.rf_mesh_closest_gradients.argtypes) == 15
    assert [int(v) for v in re.findall(r"constexpr int kGradBlock = (\d+);", csrc_text.code(UNIT))] == [256]


def test_the_unit_sits_over_the_one_rule_and_has_no_atomics_no_lds_and_no_assembly():
    assert csrc_text.includes(UNIT) == [HEADER] and csrc_text.includes(HEADER) == [RULE]
    for name in ("closest_on_face", "dist_segment", "dist_candidate"):
        assert csrc_text.definitions(r"FaceClosest " + name + r"\(") == [(RULE, "FaceClosest " + name + "(")], name
    assert csrc_text.definitions(r"float dist_edge\(") == [(RULE, "float dist_edge(")]
    assert csrc_text.definitions(r"float dist_dot\(") == [(RULE, "float dist_dot(")]
    own = csrc_text.code(UNIT) + csrc_text.code(HEADER)
    for word in ("atomic", "__shared__", "asm", "__syncthreads", "__builtin_amdgcn", "#define", "__shfl", "__ballot"):
        assert word not in own, word
    for word in ("atomic", "__shared__", "asm", "__syncthreads", "__builtin_amdgcn", "#define"):
        assert word not in csrc_text.unit_code(UNIT), word  # (with the rule's header)
    assert "__global__" in own and own.count("closest_gradient_on_face(") == 2  # the definition and the one call
    for helper in ("dist_segment(", "dist_candidate(", "dist_edge(", "dist_dot("):
        assert helper in csrc_text.code(HEADER), helper
    # the forward's files are not part of this change's claims beyond being included: their text is pinned by their own ABI test
    assert "closest_on_face(" not in own


def test_validates_in_the_documented_order_before_any_launch(lib):
    """every device pointer below is a made-up address: a launch, or any device access, would fault"""

    def grads(vertices=4096, V=8, faces=8192, T=4, points=12288, face=16384, grad=20480, N=4, flags=0, grad_points=24576, records=28672, bary=32768, region=36864,
              status=40960):
        return lib.rf_mesh_closest_gradients(vertices, V, faces, T, points, face, grad, N, flags, grad_points, records, bary, region, status, None)

    none = dict(grad_points=None, records=None, bary=None, region=None)
    # 1. pointers
    assert grads(status=None) == NULL
    for name in ("vertices", "faces", "points", "face", "grad"):
        assert grads(**{name: None}) == NULL, name
    assert grads(**none) == NULL
    # 2. shapes
    for name in ("V", "T", "N"):
        assert grads(**{name: -1}) == SHAPE and grads(**{name: 1 << 31}) == SHAPE, name
    # 3. flags
    for flags in (1, 2, 128, 1 << 31):
        assert grads(flags=flags, T=0) == UNSUPPORTED and grads(flags=flags, N=0) == UNSUPPORTED
    # the order: pointers before shapes before flags
    assert grads(status=None, N=-1) == NULL and grads(points=None, V=1 << 31, flags=1) == NULL and grads(T=-1, **none) == NULL
    assert grads(N=-1, flags=1) == SHAPE and grads(V=-1, flags=3) == SHAPE
    # zero queries / zero faces: RF_OK without a launch, with or without the arrays they would need
    assert grads(N=0) == OK and grads(N=0, points=None, face=None, grad=None, **none) == OK
    assert grads(T=0) == OK and grads(T=0, vertices=None, faces=None) == OK and grads(T=0, V=0, vertices=None, faces=None) == OK
    # every single output is enough
    for name in none:
        assert grads(N=0, **{k: None for k in none if k != name}) == OK
