"""The float64 model of rf.bake_texture_from_views (tests/texture_views_model.py) on the CPU: on every input the GPU test runs, few texels
are ambiguous (the cap is a condition of the comparison); the crafted exact cases equal their closed forms; and the comparison
rejects wrong models -- no depth test, a nearest-pixel fetch, a fetch without the half-pixel shift, an unflipped y, ignored alphas."""
import numpy as np
import pytest

from tests import mesh_raster_model as mrm
from tests import texture_views_model as tvm


@pytest.mark.parametrize("name", tvm.CASES)
def test_few_texels_are_ambiguous(name):
    ref, depths = tvm.reference(name)
    made = tvm.make_case(name)
    owned = ref["owned"]
    share = ref["ambiguous"][owned].mean()
    seen = (ref["views"][owned] > 0).mean()
    print(f"{name}: {int(owned.sum())} owned texels, {100 * share:.2f} % ambiguous, {100 * seen:.1f} % seen, worst bound {ref['bound'].max():.3e}")
    assert share <= tvm.MAX_AMBIGUOUS, f"{name}: {100 * share:.2f} % of the owned texels are ambiguous (bump its seed in SEED_BUMP)"
    assert np.isfinite(ref["bound"]).all() and np.isfinite(ref["texture"]).all()
    assert ref["views"].max() <= len(made["views"]) and (ref["views"][~owned] == 0).all()
    assert ((ref["weight"] > 0) == (ref["views"] > 0)).all()
    tvm.compare(ref, ref["texture"], ref["weight"], ref["views"])  # (the model passes its own comparison)


def test_the_cases_cover_what_they_claim():
    total_seen = 0
    for name in tvm.CASES:
        ref, depths = tvm.reference(name)
        total_seen += int((ref["views"] > 0).sum())
    assert total_seen > 5000
    # a view behind the mesh and one that looks past it contribute nothing; the others do
    made = tvm.make_case("oct31-P4-40x40-v17")
    _, depths = tvm.reference("oct31-P4-40x40-v17")
    spec = tvm.SPECS["oct31-P4-40x40-v17"]
    for k in range(17):
        one = dict(made, views=[made["views"][k]], images=made["images"][k:k + 1], alphas=made["alphas"][k:k + 1])
        seen = int((tvm.project_case(one, depths[k:k + 1])["views"] > 0).sum())
        assert (seen == 0) == (k in (spec["behind"], spec["nothing"])), (k, seen)
    assert not np.isfinite(depths[spec["behind"]]).any() and not np.isfinite(depths[spec["nothing"]]).any()
    # the zero-area face is seen by no view, its neighbours are
    ref, _ = tvm.reference("oct32-P3-zero-area")
    face = tvm.tm.texel_table(32, 3)["face"]
    assert (ref["views"][face == 3] == 0).all() and (ref["views"][face == 0] > 0).any()
    # the flipped face is seen only under the two-sided flag
    one, _ = tvm.reference("oct32-P4-flipped-one-sided")
    two, _ = tvm.reference("oct32-P4-flipped-two-sided")
    face = tvm.tm.texel_table(32, 4)["face"]
    assert (one["views"][face == 3] == 0).all() and (two["views"][face == 3] > 0).any()
    assert (one["views"] <= two["views"]).all()  # (|cos| also lets back faces near the limb through, within the depth bias)
    # near cuts the front of the ball away
    ref, _ = tvm.reference("oct32-P4-near")
    made = tvm.make_case("oct32-P4-near")
    far = tvm.project_case(dict(made, near=0.0), tvm.depth_buffers(dict(made, near=0.0))[0])
    assert 0 < (ref["views"] > 0).sum() < (far["views"] > 0).sum()
    # an odd face count leaves half of the last block unowned
    ref, _ = tvm.reference("oct31-P4-40x40-v17")
    lay = ref["layout"]
    last = ref["owned"][-lay["block"]:, (15 % lay["cols"]) * lay["block"]:(15 % lay["cols"] + 1) * lay["block"]]
    assert last.any() and not last.all()


@pytest.mark.parametrize("name", tvm.EXACT_CASES)
def test_exact_cases_equal_their_closed_forms(name):
    made = tvm.make_exact(name)
    view = made["views"][0]
    mrm.assert_exact_in_float32(dict(vertices=made["vertices"], faces=made["faces"], H=16, W=16, focal=16.0, R=view["R"], t=view["t"]))
    raster = mrm.rasterise(made["vertices"], made["faces"], 16, 16, 16.0, view["R"], view["t"])
    depths = np.where(raster["mask"], raster["depth"], np.inf)
    want = tvm.exact_expectation(made, raster["face_ids"], depths)
    ref = tvm.project_case(made, depths[None])
    assert np.array_equal(ref["texture"], want["texture"]) and np.array_equal(ref["weight"], want["weight"]) and np.array_equal(ref["views"], want["views"])
    assert np.array_equal(ref["texture"].astype(np.float32).astype(np.float64), ref["texture"])  # every value is a float32
    kinds = {k: int((want["kind"] == k).sum()) for k in ("seen", "occluded", "empty", "outside", "unowned")}
    print(f"{name}: {kinds}")
    face = tvm.tm.texel_table(len(made["faces"]), made["patch"])["face"]
    assert ((want["kind"] == "seen") & (face == 0)).sum() >= 5  # (a texel is seen when the CENTRE of its pixel lies in the face)
    if name == "exact-two":
        back = face == 1
        for kind in ("seen", "occluded", "empty"):
            assert ((want["kind"] == kind) & back).sum() >= 3, kind
        assert (ref["texture"][back & (want["kind"] != "seen")] == np.array(tvm.EXACT_SENTINEL)).all()
        assert (ref["views"][back & (want["kind"] == "occluded")] == 0).all()


@pytest.mark.parametrize("wrong", tvm.WRONG)
def test_the_comparison_rejects_wrong_models(wrong):
    rejected = []
    for name in tvm.CASES:
        ref, _ = tvm.reference(name)
        bad, _ = tvm.reference(name, wrong)
        try:
            tvm.compare(ref, bad["texture"], bad["weight"], bad["views"])
        except AssertionError:
            rejected.append(name)
    print(f"{wrong}: rejected on {len(rejected)} of {len(tvm.CASES)} cases")
    assert rejected, wrong
    if wrong == "alphas_ignored":
        assert all(tvm.make_case(name)["alphas"] is not None for name in rejected)


def test_depth_keys():
    keys = tvm.depth_keys(np.array([[[1.0, np.inf], [0.0, 2.5]]]))
    assert keys.dtype == np.int64 and keys[0, 0, 1] == -1 and keys[0, 1, 0] == 0
    assert keys[0, 0, 0] == int(np.float32(1.0).view(np.uint32)) << 32 and keys[0, 1, 1] == int(np.float32(2.5).view(np.uint32)) << 32
