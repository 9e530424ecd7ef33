"""The float64 model of the texture fit (tests/texture_fit_model.py) against the rasteriser's model and against itself: its forward on
its own taps is the colour of tests/mesh_raster_model.py, its transposed sum is the adjoint of its forward, a float64 fit of a
representable target goes down, a float32 restatement of the transposed sum lies within the bound of docs/texture_fit_errors.md on
the inputs of the GPU test, and three doctored adjoints do not."""
import numpy as np
import pytest

from tests import texture_fit_model as tfm
from tests.helpers import hash_uniform


@pytest.mark.parametrize("name", tfm.CASES)
def test_forward_on_the_models_own_taps_is_the_rasterisers_colour(name):
    case = tfm.make_case(name)
    taps, colour = tfm.model_taps(name)
    assert np.abs(tfm.forward(taps, case["texture"], case["background"]) - colour).max() <= 1e-12
    hit = tfm.hit_of(taps)
    Ht, Wt = case["texture"].shape[:2]
    for key, edge in (("x0", Wt), ("x1", Wt), ("y0", Ht), ("y1", Ht)):
        assert (taps[key][hit] < edge).all() and (taps[key][hit] >= 0).all() and (taps[key][~hit] == tfm.NO_TAP).all()
    assert ((taps["fx"] >= 0) & (taps["fx"] < 1) & (taps["fy"] >= 0) & (taps["fy"] < 1)).all()


def test_the_cases_cover_what_they_are_there_for():
    counts = {name: tfm.transposed(tfm.model_taps(name)[0], np.zeros((len(tfm.model_taps(name)[0]["x0"]), 3)), *tfm.make_case(name)["texture"].shape[:2])[2]
              for name in tfm.CASES}
    assert counts["T1-P2-48x64-v3"].max() > 4096 and (counts["T1-P2-48x64-v3"] == 0).any()
    assert any(((c > 0) & (c <= 64)).any() for c in counts.values()) and any((c > 64).any() for c in counts.values())
    for name in ("T3-P8-24x40-v3", "T37-P3-37x53-v17"):  # a view that looks past the mesh: every pixel a miss
        case, taps = tfm.make_case(name), tfm.model_taps(name)[0]
        per_view = tfm.hit_of(taps).reshape(len(case["views"]), -1).sum(1)
        assert (per_view == 0).any() and (per_view > 0).any()
    one = tfm.model_taps("T2-tex1x1-24x40-v2")[0]
    hit = tfm.hit_of(one)
    assert hit.any() and (one["x0"][hit] == one["x1"][hit]).all() and (one["y0"][hit] == one["y1"][hit]).all()
    free = tfm.model_taps("T5-tex5x7-24x40-v2")[0]
    assert (free["x0"][tfm.hit_of(free)] == free["x1"][tfm.hit_of(free)]).any()  # clamped duplicates among ordinary taps
    assert {len(tfm.make_case(n)["views"]) for n in tfm.CASES} >= {1, 2, 17} and {len(tfm.make_case(n)["faces"]) for n in tfm.CASES} >= {1, 2, 3, 37}


@pytest.mark.parametrize("name", tfm.CASES)
def test_adjoint_identity(name):
    case = tfm.make_case(name)
    taps, _ = tfm.model_taps(name)
    Ht, Wt = case["texture"].shape[:2]
    x = hash_uniform((Ht, Wt, 3), 11).astype(np.float64)
    y = hash_uniform((len(taps["x0"]), 3), 12).astype(np.float64)
    Ax = tfm.forward(taps, x, 0.0)  # (background 0: the linear part)
    ATy, _, counts = tfm.transposed(taps, y, Ht, Wt)
    lhs, rhs = float((Ax * y).sum()), float((x.reshape(-1, 3) * ATy).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, float(np.abs(Ax * y).sum()))
    assert counts.sum() == 4 * tfm.hit_of(taps).sum()


def test_a_float64_fit_of_a_representable_target_goes_down():
    name = "T3-P8-24x40-v3"
    case = tfm.make_case(name)
    taps, target = tfm.model_taps(name)  # the render of the case's own texture: the optimum is 0
    losses, texture = tfm.adam_fit(taps, np.zeros_like(case["texture"]), target, None, case["background"], 101, 0.05)
    assert losses[0] > losses[9] > losses[99] > 0.0 and losses[100] < 0.05 * losses[0]
    covered = tfm.transposed(taps, np.zeros_like(target), *case["texture"].shape[:2])[2].reshape(case["texture"].shape[:2]) > 0
    assert (texture[~covered] == 0.0).all() and texture.min() >= 0.0 and texture.max() <= 1.0
    l1, _ = tfm.adam_fit(taps, np.zeros_like(case["texture"]), target, None, case["background"], 101, 0.05, loss="l1")
    assert l1[0] > l1[9] > l1[99]


def float32_transposed(taps, grad_colour, Ht, Wt):
    """the sums of rf_texture_sample_backward restated in float32: the weights as the Python layer computes them, one rounding per
    product, the additions one after another in entry order"""
    one = np.float32(1.0)
    pixel = np.nonzero(tfm.hit_of(taps))[0]
    fx, fy = taps["fx"][pixel].astype(np.float32), taps["fy"][pixel].astype(np.float32)
    texel = np.stack([taps["y0"][pixel] * Wt + taps["x0"][pixel], taps["y0"][pixel] * Wt + taps["x1"][pixel], taps["y1"][pixel] * Wt + taps["x0"][pixel],
                      taps["y1"][pixel] * Wt + taps["x1"][pixel]], 1).reshape(-1)
    weight = np.stack([(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy], 1).reshape(-1)
    order = np.argsort(texel, kind="stable")
    terms = weight[order][:, None] * np.asarray(grad_colour, np.float32)[np.repeat(pixel, 4)[order]]
    grad = np.zeros((Ht * Wt, 3), np.float32)
    np.add.at(grad, texel[order], terms)
    assert grad.dtype == np.float32 and terms.dtype == np.float32
    return grad


def float32_taps(taps):
    return dict(taps, fx=taps["fx"].astype(np.float32).astype(np.float64), fy=taps["fy"].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name", tfm.CASES)
def test_float32_sums_lie_within_the_bound_and_doctored_adjoints_do_not(name):
    case = tfm.make_case(name)
    taps = float32_taps(tfm.model_taps(name)[0])
    Ht, Wt = case["texture"].shape[:2]
    P = len(taps["x0"])
    y = hash_uniform((P, 3), 21).astype(np.float32)
    ref, bound, counts = tfm.transposed(taps, y, Ht, Wt)
    err = np.abs(float32_transposed(taps, y, Ht, Wt).astype(np.float64) - ref)
    assert (err <= bound).all() and (err[counts == 0] == 0).all(), (err - bound).max()
    if tfm.hit_of(taps).sum() < 2:
        return
    if Ht * Wt > 1:  # (on a single texel the four weights sum to 1 whichever way round)
        swapped = tfm.transposed(taps, y, Ht, Wt, wrong="fx_fy_swapped")[0]
        assert (np.abs(swapped - ref) > bound).any()
    clamped = (taps["x0"] == taps["x1"]) | (taps["y0"] == taps["y1"])
    if (clamped & tfm.hit_of(taps)).any():
        dropped = tfm.transposed(taps, y, Ht, Wt, wrong="duplicate_dropped")[0]
        assert (np.abs(dropped - ref) > bound).any()
    # the (1 - m) background term of the image model, in the gradient of the loss
    alphas = (0.5 + 0.5 * hash_uniform((P,), 22)).astype(np.float32)
    images = (0.5 + 0.5 * hash_uniform((P, 3), 23)).astype(np.float32)
    right = tfm.loss_and_grad(taps, case["texture"], images, alphas, 1.0)[1]
    wrong = tfm.loss_and_grad(taps, case["texture"], images, alphas, 1.0, wrong="alpha_ignored")[1]
    ref_l, bound_l, _ = tfm.transposed(taps, right, Ht, Wt)
    assert (np.abs(tfm.transposed(taps, wrong, Ht, Wt)[0] - ref_l) > bound_l).any()


def test_crafted_list():
    offsets, pixel, weight, grad_colour = tfm.crafted_list()
    lengths = np.diff(offsets)
    assert {0, 1, 15, 16, 17, 63, 64, 65, 66, 4097}.issubset(set(lengths.tolist())) and lengths.max() > 100000 and int(pixel.max()) < len(grad_colour) and int(pixel.min()) >= 0
    ref, bound = tfm.crafted_reference(offsets, pixel, weight, grad_colour)
    assert (ref[lengths == 0] == 0).all() and (bound[lengths > 0] > 0).all()
    # a float32 sum, one addition after another, lies within it
    grad = np.zeros_like(ref, dtype=np.float32)
    np.add.at(grad, np.repeat(np.arange(len(lengths)), lengths), weight[:, None] * grad_colour[pixel])
    assert (np.abs(grad.astype(np.float64) - ref) <= bound).all()
