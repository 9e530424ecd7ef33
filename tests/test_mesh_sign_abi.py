"""rf_mesh_face_pseudonormals and rf_mesh_signed_distance: the symbols are exported and declared in include/relu_field_ext.h -- the
list of include/relu_field.h stays closed at 69 --, the prototypes agree with the binding's argtypes, the unit and its private header
are build inputs that sit over the gradient rule alone, free of atomics, LDS, barriers, inline assembly, builtins and macros, and the
argument checks come back as codes, in the documented order, before any launch (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

from tests import csrc_text
from tests.test_abi_symbols import _matches, _same_scalar
from thr3ed_atom_amd import _lib

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
UNIT, HEADER, RULE = "mesh_sign_kernels.hip", "mesh_sign.h", "mesh_distance_grad.h"
EXT = os.path.join(_lib.INCLUDE_DIR, "relu_field_ext.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def prototypes():
    """{name: (return type, [parameter types])} of include/relu_field_ext.h, comments removed"""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(EXT).read(), flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"(?m)^((?:const )?\w+\*?) (rf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        out[name] = (ret.strip(), [] if params == ["void"] else [re.sub(r"\s*\b\w+$", "", p) for p in params])
    return out


def test_the_extension_header_declares_the_extension_symbols_and_the_first_list_stays_closed(lib):
    assert len(_lib.EXPORTED_SYMBOLS) == 69 and len(set(_lib.EXPORTED_SYMBOLS)) == 69
    assert _lib.EXTENSION_SYMBOLS == ["rf_ext_abi_version", "rf_mesh_face_pseudonormals", "rf_mesh_signed_distance"]
    assert not set(_lib.EXTENSION_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    declared = prototypes()
    assert sorted(declared) == sorted(_lib.EXTENSION_SYMBOLS)
    first = open(os.path.join(_lib.INCLUDE_DIR, "relu_field.h")).read()
    for name in _lib.EXTENSION_SYMBOLS:
        assert hasattr(lib, name) and name not in first, name
    text = open(EXT).read()
    assert "#define RF_EXT_ABI_VERSION 1" in text and '#include "relu_field.h"' in text
    assert lib.rf_ext_abi_version() == _lib.EXT_ABI_VERSION == 1 and lib.rf_abi_version() == _lib.ABI_VERSION == 4
    assert EXT in _lib.build_inputs() and UNIT in _lib.SOURCES
    assert os.path.join(_lib.CSRC_DIR, UNIT) in _lib.build_inputs() and os.path.join(_lib.CSRC_DIR, HEADER) in _lib.build_inputs()
    for phrase in ("sign = s < 0 ? -1 : +1", "alpha_k = atan2f(len, dot(e1_k, e2_k))", "n^_f + n^_h when h >= 0, else n^_f", "beta_x == 1"):
        assert phrase in text, phrase


def test_prototypes_agree_with_the_argtypes(lib):
    for name, (ret, params) in sorted(prototypes().items()):
        fn = getattr(lib, name)
        argtypes = fn.argtypes or []
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes, {len(params)} parameters in the header"
        for k, (ctype, c_type) in enumerate(zip(argtypes, params)):
            assert _matches(ctype, c_type), f"{name}: argument {k} is {ctype!r}, the header has `{c_type}`"
        assert _same_scalar(fn.restype, ret), name
    assert len(lib.rf_mesh_face_pseudonormals.argtypes) == 9 and len(lib.rf_mesh_signed_distance.argtypes) == 15
    assert not _matches(C.c_int32, "int64_t")  # (the comparison notices a wrong entry)


def test_each_extension_symbol_is_defined_once_in_its_unit():
    definition = re.compile(r"^(?:int|int32_t|int64_t|const char\*) (rf_[a-z_0-9]+)\(", re.M)
    found = {unit: definition.findall(open(os.path.join(_lib.CSRC_DIR, unit)).read()) for unit in _lib.SOURCES}
    for name in _lib.EXTENSION_SYMBOLS:
        assert [unit for unit, names in found.items() for n in names if n == name] == [UNIT], name
    assert sorted(found[UNIT]) == sorted(_lib.EXTENSION_SYMBOLS)


def test_the_unit_sits_over_the_gradient_rule_and_has_no_atomics_no_lds_and_no_assembly():
    assert csrc_text.includes(UNIT) == [HEADER] and csrc_text.includes(HEADER) == [RULE]
    assert csrc_text.private_headers(UNIT) == [HEADER, RULE, "mesh_distance.h"]
    own = csrc_text.code(UNIT) + csrc_text.code(HEADER)
    for word in ("atomic", "__shared__", "asm", "__syncthreads", "__builtin_amdgcn", "#define", "__shfl", "__ballot"):
        assert word not in own, word
    for word in ("atomic", "__shared__", "asm", "__syncthreads", "__builtin_amdgcn", "#define"):
        assert word not in csrc_text.unit_code(UNIT), word  # (with the rules' headers)
    assert own.count("__global__") == 2 and own.count("closest_gradient_on_face(") == 1  # the one call
    assert csrc_text.definitions(r"SignNormal unit_normal\(") == [(HEADER, "SignNormal unit_normal(")]
    assert csrc_text.definitions(r"float signed_distance\(") == [(HEADER, "float signed_distance(")]
    assert "closest_on_face(" not in own and "dist_segment(" not in own  # the distance rule is reached through the gradient rule only
    assert [int(v) for v in re.findall(r"constexpr int kSignBlock = (\d+);", csrc_text.code(UNIT))] == [256]
    # no array is indexed by a register in the rule (the compiler would move it to LDS or scratch)
    assert not re.search(r"beta\[[a-z]", csrc_text.code(HEADER))


def test_validates_in_the_documented_order_before_any_launch(lib):
    """every device pointer below is a made-up address: a launch, or any device access, would fault"""

    def normals(vertices=4096, V=8, faces=8192, T=4, flags=0, out=12288, records=16384, status=20480):
        return lib.rf_mesh_face_pseudonormals(vertices, V, faces, T, flags, out, records, status, None)

    def signed(vertices=4096, V=8, faces=8192, T=4, partners=12288, table=16384, points=20480, face=24576, N=4, flags=0, out=28672, feature=32768, normal=36864,
               status=40960):
        return lib.rf_mesh_signed_distance(vertices, V, faces, T, partners, table, points, face, N, flags, out, feature, normal, status, None)

    # 1. pointers
    assert normals(status=None) == NULL and signed(status=None) == NULL
    for name in ("vertices", "faces", "out", "records"):
        assert normals(**{name: None}) == NULL, name
    for name in ("vertices", "faces", "partners", "table", "points", "face", "out"):
        assert signed(**{name: None}) == NULL, name
    # 2. shapes
    for name in ("V", "T"):
        assert normals(**{name: -1}) == SHAPE and normals(**{name: 1 << 31}) == SHAPE, name
    for name in ("V", "T", "N"):
        assert signed(**{name: -1}) == SHAPE and signed(**{name: 1 << 31}) == SHAPE, name
    assert normals(T=(1 << 31) // 3) == SHAPE and signed(T=(1 << 31) // 3) == SHAPE  # an edge is 3 face + k in int32
    # 3. flags
    for flags in (1, 2, 128, 1 << 31):
        assert normals(flags=flags, T=0) == UNSUPPORTED
        assert signed(flags=flags, T=0) == UNSUPPORTED and signed(flags=flags, N=0) == UNSUPPORTED
    # the order: pointers before shapes before flags
    assert normals(status=None, T=-1) == NULL and normals(out=None, V=1 << 31, flags=1) == NULL and normals(V=-1, flags=1) == SHAPE
    assert signed(status=None, N=-1) == NULL and signed(points=None, V=1 << 31, flags=1) == NULL and signed(N=-1, flags=1) == SHAPE and signed(V=-1, flags=3) == SHAPE
    # zero faces / zero queries: RF_OK without a launch, with or without the arrays they would need
    assert normals(T=0) == OK and normals(T=0, vertices=None, faces=None, out=None, records=None) == OK
    assert signed(N=0) == OK and signed(N=0, points=None, face=None, out=None, feature=None, normal=None) == OK
    assert signed(T=0) == OK and signed(T=0, V=0, vertices=None, faces=None, partners=None, table=None) == OK
    # the two optional outputs
    assert signed(N=0, feature=None) == OK and signed(N=0, normal=None) == OK
