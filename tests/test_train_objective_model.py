"""The float64 model of the regularised iteration (tests/train_objective_model.py) on the CPU: the conditions under which the GPU
comparisons of tests/test_hip_combined_step.py say something, with the keys those tests use, and three wrong models the bars reject."""
import pytest

from tests import train_objective_model as tom


@pytest.mark.parametrize("name", list(tom.CASES))
def test_conditions_of_the_cases(name):
    """Per step: no sample of either render within the ReLU band (float32 and float64 decide every gate alike); the distortion gradient
    exceeds 100 x bar on >= 10 % of the density elements and each TV gradient on >= 90 % of its tensor (a dropped term is visible).
    Over the steps: >= 90 % of each tensor has an Adam bar of at most lr / 10, and the densities move by more than 1e-3."""
    dens, feat = tom.case_inputs(name)[:2]
    tr = tom.trajectory(name)
    for t, ev in enumerate(tr["evals"]):
        _, dist_gd, _ = ev["terms"]["distortion"]
        _, tv_gd, tv_gf = ev["terms"]["tv"]
        shares = (tom.exceeds(dist_gd, 100 * ev["bar_d"]), tom.exceeds(tv_gd, 100 * ev["bar_d"]), tom.exceeds(tv_gf, 100 * ev["bar_f"]))
        print(f"conditions {name} step {t}: ReLU band {ev['band']}, above 100 x bar: distortion {shares[0]:.1%} of D, TV {shares[1]:.1%} of D, "
              f"TV {shares[2]:.1%} of F; L = {ev['value']:.6f}")
        assert ev["band"] == (0, 0)
        assert shares[0] >= 0.10 and shares[1] >= 0.90 and shares[2] >= 0.90
    tight_d = float((tr["bar_d"] <= tom.LR / 10).double().mean())
    tight_f = float((tr["bar_f"] <= tom.LR / 10).double().mean())
    move = float((tr["dens"] - dens.double()).abs().max())
    print(f"conditions {name}: Adam bar <= lr / 10 on {tight_d:.1%} of D, {tight_f:.1%} of F; largest density move {move:.3f}; "
          f"exact zeros {int(tr['zero_d'].sum())} of D, {int(tr['zero_f'].sum())} of F")
    assert tight_d >= 0.90 and tight_f >= 0.90
    assert move > 1e-3


def rejected(wrong, right, bar):
    return bool(((wrong - right).abs() > bar).any())


@pytest.mark.parametrize("name", list(tom.CASES))
def test_the_bar_rejects_three_wrong_models(name):
    """the objective without the distortion term, the objective with TV applied twice, and the gradient of step t added to that of
    step t + 1 (a bucket that was not cleared): each misses the bar of the right model, on the tensors it touches"""
    evals = tom.trajectory(name)["evals"]
    for t, ev in enumerate(evals):
        terms = ev["terms"]
        assert not rejected(ev["gd"], ev["gd"], ev["bar_d"]) and not rejected(ev["gf"], ev["gf"], ev["bar_f"])
        assert rejected(ev["gd"] - terms["distortion"][1], ev["gd"], ev["bar_d"])
        assert rejected(ev["gd"] + terms["tv"][1], ev["gd"], ev["bar_d"]) and rejected(ev["gf"] + terms["tv"][2], ev["gf"], ev["bar_f"])
        if t > 0:
            assert rejected(ev["gd"] + evals[t - 1]["gd"], ev["gd"], ev["bar_d"]) and rejected(ev["gf"] + evals[t - 1]["gf"], ev["gf"], ev["bar_f"])


@pytest.mark.parametrize("name", list(tom.CASES))
def test_the_adam_bar_rejects_a_trajectory_without_the_distortion_term(name):
    """two Adam steps on the objective without the distortion term leave the Adam bar of the right trajectory"""
    dens, feat = tom.case_inputs(name)[:2]
    first = tom.trajectory(name)["evals"][0]  # (step 0 starts from the same parameters on both sides)

    def right(D, F, t):
        return first if t == 0 else tom.case_objective(name, D, F, tom.step_keys(t))

    def without_distortion(D, F, t):
        ev = right(D, F, t)
        return dict(ev, gd=ev["gd"] - ev["terms"]["distortion"][1])

    good, wrong = tom.adam_steps(dens, feat, right, 2), tom.adam_steps(dens, feat, without_distortion, 2)
    assert bool(((wrong["dens"] - good["dens"]).abs() > good["bar_d"]).any())


@pytest.mark.parametrize("name", list(tom.CASES))
def test_conditions_of_the_trainer_batch(name):
    """the batch TrainStepper.step() draws itself: no sample in the ReLU band, 130 distinct rays of which part hit the volume, every
    term visible as in the cases"""
    ev = tom.trainer_batch_objective(name)
    o, d, pixels, keys = tom.trainer_batch()
    assert o.shape == d.shape == pixels.shape == (tom.NUM_RAYS, 3) and len(set(map(tuple, d.tolist()))) == tom.NUM_RAYS
    shares = (tom.exceeds(ev["terms"]["distortion"][1], 100 * ev["bar_d"]), tom.exceeds(ev["terms"]["tv"][1], 100 * ev["bar_d"]),
              tom.exceeds(ev["terms"]["tv"][2], 100 * ev["bar_f"]))
    print(f"conditions {name} trainer batch: ReLU band {ev['band']}, above 100 x bar: distortion {shares[0]:.1%} of D, TV {shares[1]:.1%} of D, "
          f"TV {shares[2]:.1%} of F; sum l_r = {ev['distortion_sum']:.4f}")
    assert ev["band"] == (0, 0)
    assert shares[0] >= 0.10 and shares[1] >= 0.90 and shares[2] >= 0.90
