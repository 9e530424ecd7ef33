"""tests/fusion_model.py, the float64 model of rf_fuse_depth_views, against a brute-force recomputation, hand-written exact cases and
its own float32 evaluation; and the chain model -> finalisation -> tests/mesh_oracle.py on an analytic sphere.  No GPU."""
import numpy as np
import pytest
import torch

from tests import fusion_model as fm
from tests import mesh_oracle

# docs/fusion_errors.md, "The sphere chain": the largest distance of a vertex of the model's mesh from the sphere measured 0.0850; it
# is held below one longest voxel edge of the lattice
SPHERE_CHAIN_MEASURED = 0.0850
SPHERE_CHAIN_BOUND = 0.103125


def run(case, dtype=np.float64, alphas=True, images=True, carve=True, near=0.0, min_alpha=0.5):
    lo, hi, dims, cams, H, W, depths, al, im, trunc = case
    return fm.fuse(lo, hi, dims, cams, H, W, depths, al if alphas else None, im if images else None, near, trunc, min_alpha, carve, dtype=dtype)


@pytest.mark.parametrize("alphas,images,carve", [(True, True, True), (False, False, True), (True, False, False), (False, True, False)])
def test_model_against_brute_force(alphas, images, carve):
    """a tiny sphere case, node by node in Python floats"""
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case(dims=(5, 4, 3), image=(9, 11, 10.0), views=3)
    depths = depths.copy()
    depths[0, 4, 5], depths[1, 3, 4] = np.nan, np.inf  # pixels that say nothing
    al, im = (al if alphas else None), (im if images else None)
    model = fm.fuse(lo, hi, dims, cams, H, W, depths, al, im, 0.0, trunc, 0.5, carve)
    total, observed, hidden, colour = fm.brute_force(lo, hi, dims, cams, H, W, depths, al, im, 0.0, trunc, 0.5, carve)
    assert (model.observed == observed).all() and (model.hidden == hidden).all()
    assert observed.sum() > 0 and (hidden.sum() > 0 or not carve)
    np.testing.assert_allclose(model.tsdf_sum, total, rtol=0, atol=1e-13)
    if images:
        np.testing.assert_allclose(model.colour_sum, colour, rtol=0, atol=1e-13)
    else:
        assert model.colour_sum is None and colour is None


@pytest.mark.parametrize("axis", [2, 0, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_cases(axis, dtype):
    """the slabs of fusion_model.exact_case: every quantity is exact in float32, the expected values are written out by hand"""
    lo, hi, dims, cams, H, W, depths, images, trunc, _ = fm.exact_case(axis)
    assert dims == {2: (8, 8, 1), 0: (1, 8, 8), 1: (8, 1, 8)}[axis]
    for carve, sums, observed, tsdf in ((True, fm.EXACT_SUM_CARVE, fm.EXACT_OBSERVED_CARVE, fm.EXACT_TSDF_CARVE),
                                        (False, fm.EXACT_SUM_PLAIN, fm.EXACT_OBSERVED_PLAIN, fm.EXACT_TSDF_PLAIN)):
        got = fm.fuse(lo, hi, dims, cams, H, W, depths, None, images, 0.0, trunc, 0.5, carve, dtype=dtype)
        assert (got.tsdf_sum == fm.exact_expected(axis, sums)).all()
        assert (got.observed == fm.exact_expected(axis, observed)).all()
        assert (got.hidden == fm.exact_expected(axis, fm.EXACT_HIDDEN)).all()
        assert (got.colour_sum[..., 3] == fm.exact_expected(axis, fm.EXACT_COLOUR_COUNT)).all()
        seen = got.colour_sum[..., 3] > 0
        assert (got.colour_sum[..., :3][seen] == np.array(fm.EXACT_COLOUR_SUM)).all() and (got.colour_sum[..., :3][~seen] == 0).all()
        np.testing.assert_allclose(fm.finalise(got.tsdf_sum, got.observed, got.hidden), fm.exact_expected(axis, tsdf), rtol=0, atol=1e-15)
        # every node sits on a pixel centre: the pixel decision has the largest margin there is
        assert (got.margins["pixel_x"] > 1e3).all() and (got.margins["pixel_y"] > 1e3).all()


def test_classification_and_finalisation():
    """observed, hidden-only and unknown nodes; -1, +1 and the mean"""
    tsdf = fm.finalise(np.array([1.5, 0.0, 0.0, -2.0]), np.array([3, 0, 0, 2]), np.array([0, 2, 0, 5]))
    assert tsdf.tolist() == [0.5, -1.0, 1.0, -1.0]
    full = run(fm.sphere_case())
    observed, hidden_only, unknown = full.observed > 0, (full.observed == 0) & (full.hidden > 0), (full.observed == 0) & (full.hidden == 0)
    assert observed.sum() > 0 and hidden_only.sum() > 0 and unknown.sum() == 0  # (every node is inside some image, and misses carve)
    final = fm.finalise(full.tsdf_sum, full.observed, full.hidden)
    assert (final[hidden_only] == -1.0).all() and (np.abs(final) <= 1.0).all()
    radius = np.linalg.norm(fm.node_positions(*fm.sphere_case()[:3]).astype(np.float64), axis=-1)
    assert (radius[hidden_only] < fm.SPHERE_RADIUS).all()  # only the ball's inside is hidden from everybody
    # without the carve and with a camera that sees only part of the box there are nodes nobody has an opinion on
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case(image=(8, 8, 30.0), views=1)
    narrow = fm.fuse(lo, hi, dims, cams, H, W, depths, None, None, 0.0, trunc, 0.5, False)
    nobody = (narrow.observed == 0) & (narrow.hidden == 0)
    assert nobody.sum() > 0 and (fm.finalise(narrow.tsdf_sum, narrow.observed, narrow.hidden)[nobody] == 1.0).all()


def test_a_miss_in_one_view_frees_a_node_other_views_hide():
    """carving: the slab's hidden column is freed by the one view that looks past it; without the carve it stays solid"""
    lo, hi, dims, cams, H, W, depths, images, trunc, _ = fm.exact_case(2)
    carved = fm.fuse(lo, hi, dims, cams, H, W, depths, None, None, 0.0, trunc, 0.5, True)
    plain = fm.fuse(lo, hi, dims, cams, H, W, depths, None, None, 0.0, trunc, 0.5, False)
    assert (carved.hidden[7] == 2).all() and (carved.observed[7] == 1).all() and (plain.observed[7] == 0).all()
    assert (fm.finalise(carved.tsdf_sum, carved.observed, carved.hidden)[7] == 1.0).all()
    assert (fm.finalise(plain.tsdf_sum, plain.observed, plain.hidden)[7] == -1.0).all()
    # the same through the alpha plane: a positive depth under an alpha below min_alpha is a miss
    alphas = np.ones_like(depths)
    alphas[0, :, 11] = 0.25
    freed = fm.fuse(lo, hi, dims, cams[:1], H, W, depths[:1], alphas[:1], None, 0.0, trunc, 0.5, True)
    kept = fm.fuse(lo, hi, dims, cams[:1], H, W, depths[:1], alphas[:1], None, 0.0, trunc, 0.25, True)
    assert (freed.observed[7] == 1).all() and (freed.hidden[7] == 0).all() and (kept.observed[7] == 0).all() and (kept.hidden[7] == 1).all()


RANDOM_CASES = [dict(), dict(dims=(7, 9, 11), image=(17, 23, 21.0), views=5), dict(dims=(16, 16, 16), image=(48, 48, 60.0), views=8),
                dict(dims=(3, 2, 65), image=(1, 1, 0.5), views=2), dict(dims=(12, 10, 9), image=(25, 31, 28.0), views=17)]


@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_cap_on_undecidable_nodes_and_float32_within_the_bound(case):
    """At most 1 % of the nodes have a decision float32 cannot take (a margin under the error of docs/fusion_errors.md); at every
    other node the float32 evaluation of the rule counts what the float64 one counts and its sums are within the bounds."""
    inputs = fm.sphere_case(**RANDOM_CASES[case])
    for options in (dict(), dict(alphas=False, carve=False), dict(near=3.0)):
        exact, single = run(inputs, **options), run(inputs, np.float32, **options)
        undecided = fm.undecidable(exact)
        assert undecided.mean() <= 0.01
        ok = ~undecided
        assert (exact.observed[ok] == single.observed[ok]).all() and (exact.hidden[ok] == single.hidden[ok]).all()
        assert (np.abs(single.tsdf_sum.astype(np.float64) - exact.tsdf_sum)[ok] <= exact.bound[ok]).all()
        assert (exact.colour_sum[..., 3][ok] == single.colour_sum[..., 3][ok]).all()
        assert (np.abs(single.colour_sum.astype(np.float64) - exact.colour_sum).max(-1)[ok] <= exact.colour_bound[ok]).all()


def test_chunks_continue_the_sums():
    """views 0 .. 16 in one loop = 16 views, then one more on top of their sums, bit for bit (float32)"""
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case(dims=(6, 5, 4), views=8)
    cams, depths, al, im = (cams * 3)[:17], np.concatenate([depths] * 3)[:17], np.concatenate([al] * 3)[:17], np.concatenate([im] * 3)[:17]
    whole = fm.fuse(lo, hi, dims, cams, H, W, depths, al, im, 0.0, trunc, 0.5, True, dtype=np.float32)
    first = fm.fuse(lo, hi, dims, cams[:16], H, W, depths[:16], al[:16], im[:16], 0.0, trunc, 0.5, True, dtype=np.float32)
    rest = fm.fuse(lo, hi, dims, cams[16:], H, W, depths[16:], al[16:], im[16:], 0.0, trunc, 0.5, True, dtype=np.float32,
                   initial=(first.tsdf_sum, first.observed, first.hidden, first.colour_sum))
    assert (whole.tsdf_sum == rest.tsdf_sum).all() and (whole.observed == rest.observed).all() and (whole.hidden == rest.hidden).all()
    assert (whole.colour_sum == rest.colour_sum).all()


def test_sphere_chain():
    """model -> finalisation -> tests/mesh_oracle.py at level 0 of -tsdf: a closed mesh whose vertices lie within the distance of
    docs/fusion_errors.md from the sphere"""
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case()
    fused = fm.fuse(lo, hi, dims, cams, H, W, depths, al, None, 0.0, trunc, 0.5, True)
    tsdf = fm.finalise(fused.tsdf_sum, fused.observed, fused.hidden)
    aabb = [(float(np.float32(a)), float(np.float32(b))) for a, b in zip(lo, hi)]
    out = mesh_oracle.extract(torch.from_numpy((-tsdf).astype(np.float32))[..., None], torch.zeros(dims + (3,)), aabb, 1.0, "identity", 0.0, 1)
    vertices, faces = out["vertices"], out["faces"]
    assert len(faces) > 1000
    closed, oriented, euler = mesh_oracle.manifold_report(faces, len(vertices))
    assert closed and oriented and euler == 2
    distance = np.abs(np.linalg.norm(vertices.astype(np.float64), axis=1) - fm.SPHERE_RADIUS).max()
    print(f"sphere chain: largest distance of a vertex from the sphere {distance:.4f}")
    assert abs(distance - SPHERE_CHAIN_MEASURED) < 5e-4  # what docs/fusion_errors.md records
    assert distance <= SPHERE_CHAIN_BOUND
    assert SPHERE_CHAIN_BOUND == max((b - a) / n for (a, b), n in zip(aabb, dims)) or abs(SPHERE_CHAIN_BOUND - max((b - a) / n for (a, b), n in zip(aabb, dims))) < 1e-6
