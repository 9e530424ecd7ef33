"""The float64 model of the mesh rasteriser (tests/mesh_raster_model.py) on the inputs the GPU test runs: few pixels are ambiguous, the
crafted cases are exact in float32 and watertight, and the comparison the GPU test applies rejects wrong models.  No GPU needed."""
import numpy as np
import pytest

from tests import mesh_raster_model as rm


@pytest.mark.parametrize("name", rm.CASES)
def test_few_pixels_are_ambiguous_and_the_model_passes_its_own_comparison(name):
    case, ref = rm.make_case(name), rm.reference(name)
    share = ref["ambiguous"].mean()
    print(f"{name}: {ref['mask'].sum()} of {ref['mask'].size} pixels covered, {ref['ambiguous'].sum()} ambiguous")
    if case["exact"]:
        rm.assert_exact_in_float32(case)
    else:
        assert share <= rm.MAX_AMBIGUOUS, share
    assert rm.compare(ref, rm.as_result(ref), exact=case["exact"]) == 0.0
    assert np.isfinite(ref["depth"]).all() and (ref["depth"][~ref["mask"]] == 0).all() and (ref["face_ids"][~ref["mask"]] == -1).all()
    if ref["colour"] is not None:
        assert (ref["colour"][~ref["mask"]] == (1.0 if case["white"] else 0.0)).all()
    take = np.ones_like(ref["mask"]) if case["exact"] else ~ref["ambiguous"]
    print(f"{name}: worst bounds: depth {ref['depth_bound'][take].max():.2e}, w {ref['bary_bound'][take].max():.2e}, colour {0.0 if ref['colour'] is None else ref['colour_bound'][take].max():.2e}")
    # the bounds say something: on the typical compared pixel of a case, less than 1e-4 of the depth and half an 8-bit step of colour
    # (a sub-pixel triangle's edge values are small differences of large products: its own bound is honest and wide)
    take &= ref["mask"]
    if take.any() and not name.startswith("slivers"):
        assert np.median(ref["depth_bound"][take] / ref["depth"][take]) < 1e-4
        if ref["colour"] is not None:
            assert np.median(ref["colour_bound"][take]) < 1.0 / 510.0


def test_the_cases_cover_what_they_are_named_for():
    covered = {name: rm.reference(name)["mask"].sum() for name in rm.CASES}
    assert covered["fullscreen"] == 24 * 40 and covered["one_pixel"] == 1
    ids = rm.reference("one_pixel")["face_ids"]
    assert ids[0, 0] == 0
    for T in (63, 64, 65, 2000):  # several sub-pixel triangles cover no pixel centre, several do
        drawn = np.unique(rm.reference(f"slivers{T}")["face_ids"])
        drawn = drawn[drawn >= 0]
        assert 0 < len(drawn) < T, (T, len(drawn))
    assert set(np.unique(rm.reference("behind_and_near")["face_ids"])) <= {-1, 4, 5} and covered["behind_and_near"] > 0
    assert set(np.unique(rm.reference("zero_area")["face_ids"])) <= {-1, 0, 4}
    both, culled = rm.reference("windings-cull0"), rm.reference("windings-cull1")
    assert culled["mask"].sum() < both["mask"].sum() and (both["mask"] | ~culled["mask"]).all()
    s = rm.edge_values(*(rm.make_case("windings-cull1")[k] for k in ("vertices", "faces", "H", "W", "focal", "R", "t")))[0].sum(-1)
    drawn = culled["face_ids"].reshape(-1)
    assert all(s[drawn[p], p] < 0 for p in np.flatnonzero(drawn >= 0))  # only the faces whose normal looks at the camera
    dup = rm.reference("duplicate")["face_ids"]
    assert dup.max() <= 3 and not rm.reference("duplicate")["ambiguous"][dup >= 0].all()
    overhang = rm.reference("overhang")["mask"]
    assert overhang[0].any() and overhang[-1].any() and overhang[:, 0].any() and overhang[:, -1].any()
    assert overhang[0, 0] and overhang[0, -1] and overhang[-1, 0] and overhang[-1, -1]


@pytest.mark.parametrize("winding", ["ccw", "cw"])
def test_shared_edges_are_watertight_and_owned_by_the_lower_index(winding):
    quad = rm.reference(f"exact-quad-{winding}")
    want = np.zeros((16, 16), bool)
    want[2:11, 2:11] = True  # the quad's corners sit on the centres of pixels 2 and 10: edges are inclusive
    assert np.array_equal(quad["mask"], want)
    i, j = np.nonzero(want)
    # face 0 = (0, 1, 2) holds the side above the diagonal (column >= row) and the diagonal itself; face 1 the rest
    assert np.array_equal(quad["face_ids"][want], np.where(j >= i, 0, 1))
    assert (quad["depth"][want] == 4.0).all()
    fan = rm.reference(f"exact-fan-{winding}")
    case = rm.make_case(f"exact-fan-{winding}")
    e = rm.edge_values(case["vertices"], case["faces"], 16, 16, 16.0, case["R"], case["t"])[0]
    inside = ((e >= 0).all(-1) | (e <= 0).all(-1))  # [T, P]
    assert np.array_equal(fan["mask"].reshape(-1), inside.any(0))
    assert np.array_equal(fan["face_ids"].reshape(-1), np.where(inside.any(0), np.argmax(inside, axis=0), -1))
    assert fan["mask"][8, 8] and fan["face_ids"][8, 8] == 0 and inside[:, 8 * 16 + 8].all()  # the hub: on a corner of every face
    assert fan["mask"].sum() > 60


def test_coplanar_overlap_goes_to_the_lower_index():
    ref, case = rm.reference("exact-coplanar"), rm.make_case("exact-coplanar")
    e = rm.edge_values(case["vertices"], case["faces"], 16, 16, 16.0, case["R"], case["t"])[0]
    inside = ((e >= 0).all(-1) | (e <= 0).all(-1)).reshape(2, 16, 16)
    overlap = inside[0] & inside[1]
    assert overlap.sum() > 10 and (ref["face_ids"][overlap] == 0).all() and (ref["face_ids"][inside[1] & ~inside[0]] == 1).all()


@pytest.mark.parametrize("wrong,name", [("exclusive_edges", "exact-quad-ccw"), ("exclusive_edges", "exact-fan-cw"), ("higher_index_wins", "exact-quad-cw"),
                                         ("higher_index_wins", "exact-coplanar"), ("higher_index_wins", "duplicate"), ("v_not_flipped", "textured-P8"),
                                         ("v_not_flipped", "slivers65"), ("integer_centres", "interpenetrating"), ("integer_centres", "fullscreen"),
                                         ("integer_centres", "exact-quad-ccw")])
def test_wrong_models_are_rejected(wrong, name):
    assert wrong in rm.WRONG
    with pytest.raises(AssertionError):
        rm.compare(rm.reference(name), rm.as_result(rm.reference(name, wrong=wrong)), exact=rm.make_case(name)["exact"])
