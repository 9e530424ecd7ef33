"""The float64 model of the geometry gradients of the mesh render (tests/mesh_fit_model.py) against itself, without a GPU: its analytic
adjoint equals central finite differences of its own forward away from the kinks, its coverage sums to the area of a polygon, few
pixel pairs of the GPU test's inputs are ambiguous, the cases are what their names claim, and the comparison the GPU test makes can
fail -- four wrong models land outside the bound."""
import numpy as np
import pytest

from tests import mesh_fit_model as mfm
from tests import mesh_raster_model as mrm

FD_STEP = 1.0e-6      # world units; moves tau by about 1e-5, a tenth of mfm.KINK
FD_TOLERANCE = 2.0e-5  # relative to the gradient's largest entry: the truncation error of a central difference at this step is far below


def run(name, wrong=None, vertices=None):
    case = mfm.make_case(name)
    ids = mfm.case_face_ids(name)
    vertices = case["vertices"].astype(np.float64) if vertices is None else vertices
    depth, coverage, views = mfm.forward(case, vertices, ids, wrong)
    return case, ids, vertices, depth, coverage, views


def pairs_of(views, key):
    return np.concatenate([v["pairs"][key] for v in views]) if views else np.zeros(0)


def test_the_cases_are_what_their_names_claim():
    hits = {name: [(ids >= 0).sum() for ids in mfm.case_face_ids(name)] for name in mfm.CASES}
    assert hits["tri-1x1"] == [1] and hits["tri-1x2"] == [1] and hits["exact-sliver"] == [0] and hits["fills-the-frame"] == [12 * 16]
    assert hits["patch37-24x32-v3"][2] == 0 and min(hits["patch37-24x32-v3"][:2]) > 100  # the last view looks past the mesh
    assert hits["big-face-72x72"][0] > 4096 and hits["big-face-72x72"][0] < 72 * 72
    fan = mfm.make_case("fan20")
    assert np.bincount(fan["faces"].reshape(-1)).max() == 20  # more corners on one vertex than the wavefront threshold of 16
    assert mfm.make_case("patch37-24x32-v3")["faces"].shape[0] == 37 and mfm.make_case("octahedron-cull0")["faces"].shape[0] == 8
    # near rejects the front face: every hit pixel shows face 1; without it the front face shows
    assert set(np.unique(mfm.case_face_ids("stacked-near2.6"))) == {-1, 1} and 0 in np.unique(mfm.case_face_ids("stacked-near0.0"))
    # culling: the outward octahedron looks the same with and without, the inward one shows its far side
    assert np.array_equal(mfm.case_face_ids("octahedron-cull0"), mfm.case_face_ids("octahedron-cull1"))
    assert not np.array_equal(mfm.case_face_ids("octahedron-cull1"), mfm.case_face_ids("octahedron-cull1-cw"))
    for name in mfm.EXACT_CASES:
        case = mfm.make_case(name)
        mrm.assert_exact_in_float32(dict(case, R=case["views"][0][0], t=case["views"][0][1]))
    # the exact cases: the silhouette through centres gives tau = 0, through midpoints 1/2, through quarters 1/4 and 3/4
    _, _, _, _, coverage, views = run("exact-centres")
    assert set(pairs_of(views, "tau")) == {0.0} and set(np.unique(coverage)) == {0.0, 0.5, 1.0}
    _, _, _, _, coverage, views = run("exact-midpoints")
    assert set(pairs_of(views, "tau")) <= {0.0, 0.5} and 0.5 in set(pairs_of(views, "tau"))
    _, _, _, _, coverage, views = run("exact-quarters")
    assert set(pairs_of(views, "tau")) == {0.25, 0.75} and {0.25, 0.5} <= set(np.unique(coverage)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    _, _, _, _, coverage, views = run("exact-sliver")
    assert not coverage.any()
    _, _, _, _, coverage, views = run("fills-the-frame")
    assert (coverage == 1.0).all() and len(pairs_of(views, "a")) == 0
    _, _, _, _, coverage, _ = run("tri-1x1")
    assert coverage.shape == (1, 1, 1) and coverage[0, 0, 0] == 1.0


@pytest.mark.parametrize("name", mfm.CASES)
def test_few_pairs_are_ambiguous_or_kinked(name):
    """the GPU comparison skips the ambiguous pairs and the finite differences the kinked ones: at most 1 % of a case's pairs each.
    The two cases whose silhouette runs exactly through centres and midpoints ARE the kink (tau = 0 and 1/2 on every pair): float32
    computes them exactly, so the GPU test compares them on every pixel, and their values are asserted above instead."""
    _, _, _, _, _, views = run(name)
    total = len(pairs_of(views, "a"))
    if name in ("exact-centres", "exact-midpoints"):
        assert pairs_of(views, "kink").all()
        return
    assert pairs_of(views, "ambiguous").sum() <= mfm.MAX_AMBIGUOUS * max(total, 1) + (0 if total >= 100 else 1), name
    assert pairs_of(views, "kink").sum() <= mfm.MAX_AMBIGUOUS * max(total, 1) + (0 if total >= 100 else 1), name


def objective(case, ids, vertices, gD, gA, wrong=None):
    depth, coverage, _ = mfm.forward(case, vertices, ids, wrong)
    return float((gD * depth).sum() + (gA * coverage).sum())


def finite_differences(case, ids, vertices, gD, gA, which, wrong=None):
    fd = np.zeros((len(which), 3))
    for row, v in enumerate(which):
        for x in range(3):
            step = np.zeros_like(vertices)
            step[v, x] = FD_STEP
            fd[row, x] = (objective(case, ids, vertices + step, gD, gA, wrong) - objective(case, ids, vertices - step, gD, gA, wrong)) / (2 * FD_STEP)
    return fd


@pytest.mark.parametrize("name", mfm.CASES)
def test_the_adjoint_equals_central_finite_differences(name):
    case, ids, vertices, _, _, views = run(name)
    gD, gA = (g.astype(np.float64) for g in mfm.upstream(case))
    grad, _, _, kinked = mfm.backward(case, vertices, ids, gD, gA, views=views)
    used = np.unique(case["faces"][np.unique(ids[ids >= 0])]) if (ids >= 0).any() else np.zeros(0, np.int64)
    which = np.array([v for v in used if not kinked[v]], np.int64)
    untouched = np.setdiff1d(np.arange(len(vertices)), used)
    assert not grad[untouched].any()  # a vertex of no winning face gets exactly 0
    if name in ("exact-centres", "exact-midpoints") or not len(which):
        return
    which = which[:: max(1, len(which) // 12)]  # (a dozen vertices per case: every kind of term is among them)
    fd = finite_differences(case, ids, vertices, gD, gA, which)
    scale = np.abs(grad).max()
    assert scale > 0 or name in ("exact-sliver",)
    assert np.abs(fd - grad[which]).max() <= FD_TOLERANCE * scale, (name, float(np.abs(fd - grad[which]).max()), scale)


def test_the_depth_gradient_has_the_sign_of_the_finite_difference():
    """dz/dv_k = + w_k n / s: pushing a face away from the camera along the ray raises the depth"""
    case, ids, vertices, depth, _, _ = run("tri-5x7")
    R, t = case["views"][0]
    away = -np.asarray(R, np.float64)[:, 2]  # the viewing direction
    gD, gA = (ids >= 0).astype(np.float64), np.zeros(ids.shape)
    grad = mfm.backward(case, vertices, ids, gD, gA)[0]
    assert (grad @ away).sum() > 0
    moved = mfm.forward(case, vertices + 1e-3 * away, ids)[0]
    assert moved[ids >= 0].mean() > depth[ids >= 0].mean()
    assert abs((moved - depth)[ids >= 0].sum() / 1e-3 - (grad @ away).sum()) < 1e-2 * (grad @ away).sum()


def test_coverage_sums_to_the_area_of_the_polygon():
    """One face whose two axis-aligned legs run at x = 2.25 and y = 2.25 in pixel coordinates (centres at the integers) and whose third edge
    lies outside the 16 x 16 image: the visible region is [2.25, 15.5]^2, area 13.25^2 = 175.5625.  Along a straight edge perpendicular
    to its pairs the spill IS the covered fraction of the strip (tau - 1/2 on the missed side, 1/2 - tau taken from the hit side), so
    every pixel holds its exact area but the one at the corner, which misses the 1/4 x 1/4 square the rule cannot see (it has no
    diagonal pairs): tolerance 1/16.  The hit mask alone counts the 13 x 13 centres inside: 169, off by 6.56 -- the test tells the
    anti-aliased image from the aliased one.  (A rectangle of two faces would not do: the rule takes the WINNING face's three edge
    lines, its interior diagonal included, so the two pixels where the diagonal leaves the rectangle lose more than they should.)"""
    corners = mrm._exact_points([[2.25, 2.25], [40.0, 2.25], [2.25, 40.0]])
    case = mfm._case("exact-quadrant", 16, 16, 16.0, mfm.EXACT_VIEW, corners, np.array([[0, 1, 2]], np.int64), exact=True)
    mrm.assert_exact_in_float32(dict(case, R=case["views"][0][0], t=case["views"][0][1]))
    ids = mfm.model_face_ids(case)
    _, coverage, views = mfm.forward(case, case["vertices"].astype(np.float64), ids)
    area, hard = 13.25 ** 2, float((ids >= 0).sum())
    assert hard == 169.0
    assert abs(coverage.sum() - area) <= 1.0 / 16.0, (coverage.sum(), area)
    assert (coverage[0, 3:, 3:] == 1.0).all() and (coverage[0, 3:, 2] == 0.25).all() and (coverage[0, 2, 3:] == 0.25).all() and not coverage[0, :3, :2].any()
    # a tilted polygon, the quad of the case "quad" in its first view against the shoelace formula: the crossing on the centre line is the
    # strip's mean only to first order and the rule counts a tilted edge once per direction, so the tolerance is 1/4 pixel per pair.  This
    # part is a sanity bound only: on this quad the sum (171.72) is no nearer the area (173.16) than the hit count (174) -- a tilted edge
    # loses in both directions, as the diagonal of exact-midpoints shows at its extreme.  The exact case above is the one that discriminates.
    quad = np.array([[3.3, 2.2], [19.6, 4.1], [17.2, 14.9], [2.4, 13.3]])
    x, y = quad[:, 0], quad[:, 1]
    area = 0.5 * abs(float((x * np.roll(y, -1) - y * np.roll(x, -1)).sum()))
    _, ids, _, _, coverage, views = run("quad")
    hard = float((ids[0] >= 0).sum())
    print(f"mesh fit model: the quad's area is {area:.3f} pixels, its anti-aliased coverage sums to {coverage[0].sum():.3f}, its hit mask to {hard:.0f}")
    assert abs(coverage[0].sum() - area) <= 0.25 * len(views[0]["pairs"]["a"])


@pytest.mark.parametrize("wrong", mfm.WRONG)
def test_the_comparison_can_fail(wrong):
    """each wrong model, compared the way the GPU test compares the device with the right one, lands outside the bound somewhere"""
    outside = False
    for name in ("tri-5x7", "exact-centres", "exact-quarters", "octahedron-cull1-cw", "quad"):
        case, ids, vertices, depth, coverage, views = run(name)
        gD, gA = (g.astype(np.float64) for g in mfm.upstream(case))
        grad, bound, doubt, _ = mfm.backward(case, vertices, ids, gD, gA, views=views)
        _, bad_coverage, bad_views = mfm.forward(case, vertices, ids, wrong)
        bad_grad = mfm.backward(case, vertices, ids, gD, gA, wrong, views=bad_views)[0]
        cover_bound = np.stack([v["coverage_bound"] for v in views])
        unsure = np.stack([v["coverage_unsure"] for v in views]) & (not case["exact"])
        outside |= bool((np.abs(bad_coverage - coverage) > cover_bound)[~unsure].any())
        keep = ~doubt | case["exact"]
        outside |= bool((np.abs(bad_grad - grad) > bound)[keep].any())
    assert outside, wrong


def test_one_adam_step_moves_every_touched_coordinate_by_the_learning_rate():
    case = mfm.make_case("quad")
    ids = mfm.case_face_ids("quad")
    start = case["vertices"].astype(np.float64)
    depth, coverage, _ = mfm.forward(case, start, ids)
    targets = depth + 0.05, np.clip(coverage * 0.9, 0, 1)
    losses, after = mfm.adam_fit(case, start, *targets, iterations=1, lr=1e-3, laplacian_weight=0.0)
    assert losses.shape == (1,) and losses[0] > 0
    step = np.abs(after - start)
    assert np.allclose(step[step > 0], 1e-3, rtol=1e-4) and (step > 0).any()
    # the Laplacian term vanishes at the start and its adjoint is the transpose of the operator
    edges = mfm.edge_list(case["faces"])
    lap, degree = mfm.laplacian(start, edges)
    x, y = np.random.default_rng(0).normal(size=(2,) + start.shape)
    assert abs((mfm.laplacian(x, edges)[0] * y).sum() - (x * mfm.laplacian_adjoint(y, edges, degree)).sum()) < 1e-12
    quiet, _ = mfm.adam_fit(case, start, depth, coverage, iterations=1, lr=1e-3)
    assert quiet[0] == 0.0  # a mesh that renders its own targets starts at loss 0: a fixed point
