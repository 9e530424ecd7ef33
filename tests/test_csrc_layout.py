"""The layout of thr3ed_atom_amd/csrc: what several units must compute with the same bits is defined ONCE, in a private header they
include; no unit is included by another.  Source text only, no GPU needed."""
import os
import re

import pytest

from tests import csrc_text
from thr3ed_atom_amd import _lib

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a definition looks like (a call has no return type in front of the name)
ONCE = {
    "raster_edges": r"float raster_edges\(",
    "raster_face": r"RasterFace raster_face\(",
    "raster_hit": r"RasterHit raster_hit\(",
    "load_face": r"bool load_face\(",
    "winning_key": r"bool winning_key\(",
    "winning_hit": r"bool winning_hit\(",
    "texel_taps": r"BilinearTaps texel_taps\(",
    "bilinear_taps": r"BilinearTaps bilinear_taps\(",
    "bilinear_blend": r"float bilinear_blend\(",
    "the segmented-sum body": r"acc\[c\] \+ __shfl_down\(acc\[c\], step, 64\)",  # (the float tree after its __ballot(is_long) hand-off)
    "camera_ok": r"bool camera_ok\(",
    "view_cameras_ok": r"bool view_cameras_ok\(",
    "image_shape_ok": r"bool image_shape_ok\(",
    "check_raster": r"int check_raster\(",
    "kMaxImageEdge": r"constexpr int kMaxImageEdge\b",
    "kMaxViews": r"constexpr int kMaxViews\b",
    "kNoHit": r"constexpr unsigned long long kNoHit\b",
    "kLaneBox": r"constexpr int kLaneBox\b",
}
HOME = {"raster_edges": "mesh_raster.h", "raster_face": "mesh_raster.h", "raster_hit": "mesh_raster.h", "load_face": "mesh_raster.h", "winning_key": "mesh_raster.h",
        "winning_hit": "mesh_raster.h", "texel_taps": "mesh_raster.h", "check_raster": "mesh_raster.h", "kLaneBox": "mesh_raster.h",
        "the segmented-sum body": "segment_sum.h"}


@pytest.mark.parametrize("what", sorted(ONCE))
def test_defined_exactly_once_in_all_of_csrc(what):
    found = csrc_text.definitions(ONCE[what])
    assert len(found) == 1, (what, [f for f, _ in found])
    assert found[0][0] == HOME.get(what, "view_camera.h")
    # and nothing declares it a second time: every other occurrence of the name is a call
    name = re.search(r"(\w+)\\[(b]", ONCE[what])
    if name and ONCE[what].endswith(r"\("):
        declared = csrc_text.definitions(r"__forceinline__[^;{]*\b%s\(" % name.group(1)) + csrc_text.definitions(r"^(?:inline )?(?:bool|int) %s\(" % name.group(1))
        assert len(declared) <= 1, (what, declared)


def test_the_wavefront_hand_off_of_a_long_segment_exists_where_it_should():
    # segment_sum.h's, and the grouped double-precision one of the simplifier, which is another reduction
    assert sorted(f for f, _ in csrc_text.definitions(r"__ballot\(is_long\)")) == ["mesh_simplify_kernels.hip", "segment_sum.h"]


def test_the_shared_limits_have_the_bindings_values():
    edge = csrc_text.definitions(r"constexpr int kMaxImageEdge = (\d+);")
    views = csrc_text.definitions(r"constexpr int kMaxViews = (\d+);")
    assert edge == [("view_camera.h", str(_lib.RASTER_MAX_EDGE))] and _lib.TEXTURE_MAX_EDGE == _lib.RASTER_MAX_EDGE
    assert views == [("view_camera.h", str(_lib.TEXTURE_VIEWS_MAX_VIEWS))] and _lib.FUSE_MAX_VIEWS == _lib.TEXTURE_VIEWS_MAX_VIEWS


def test_no_unit_is_included_and_headers_are_build_inputs():
    for name in csrc_text.files():
        for header in csrc_text.includes(name):
            assert header.endswith(".h") and (header in csrc_text.files() or header == "relu_field.h"), (name, header)
        if name.endswith(".h"):
            assert "#pragma once" in csrc_text.code(name) and os.path.join(_lib.CSRC_DIR, name) in _lib.build_inputs(), name
            assert "__global__" not in csrc_text.code(name) and 'extern "C"' not in csrc_text.code(name), name  # kernels and entry points stay in units
        else:
            assert name in _lib.SOURCES, name
    assert csrc_text.private_headers("mesh_fit_kernels.hip") == ["mesh_raster.h", "view_camera.h", "segment_sum.h"]
    assert csrc_text.private_headers("mesh_raster_kernels.hip") == ["mesh_raster.h", "view_camera.h"]
    assert csrc_text.private_headers("texture_fit_kernels.hip") == ["segment_sum.h", "view_camera.h"]
    assert csrc_text.private_headers("texture_views_kernels.hip") == ["texture_atlas.h", "view_camera.h"]
    assert csrc_text.private_headers("fusion_kernels.hip") == ["view_camera.h"]
    # the preprocessor switch that once cut the raster unit into a header is gone from the whole tree
    switch = "RF_MESH_RASTER_DEVICE" + "_ONLY"
    for folder in ("thr3ed_atom_amd", "include", "tests", "docs", "tools"):
        for root, _, names in os.walk(os.path.join(REPO_ROOT, folder)):
            for n in names:
                if n.endswith((".py", ".hip", ".h", ".md")):
                    assert switch not in open(os.path.join(root, n), errors="replace").read(), os.path.join(root, n)
    for n in ("README.md", "DESIGN.md"):
        assert switch not in open(os.path.join(REPO_ROOT, n)).read(), n


def test_the_segmented_sum_kernels_are_one_call_of_the_shared_body():
    fit, mesh = csrc_text.code("texture_fit_kernels.hip"), csrc_text.code("mesh_fit_kernels.hip")
    for unit, kernel in ((fit, "void texture_sample_backward_kernel("), (mesh, "void segment_sum_kernel(")):
        body = unit[unit.index(kernel):]
        body = body[body.index("{") + 1:body.index("\n}")]
        assert body.count(";") == 1 and "segment_sum<" in body, kernel
        assert "__shfl" not in unit and "__ballot" not in unit
    assert "void add_entry(" in fit and "void add_row(" in mesh
    # the unit weight of the mesh sums is no multiplication by one
    add_row = mesh[mesh.index("void add_row("):mesh.index("struct AddRow")]
    assert "acc[c] = acc[c] + g[c];" in add_row and "weight" not in add_row
