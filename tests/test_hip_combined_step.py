"""TrainStepper with the distortion loss AND both total-variation weights on, on real render gradients, against the float64 model of the
whole objective (tests/train_objective_model.py): the gradient bucket of one iteration on every element, three Adam steps on every
element, a fourth iteration's bucket (a stale bucket fails there), and the path TrainStepper.step() takes in real training, where the
step draws its own batch.  Five step configurations x three storages x two grids (B: non-cubic, anisotropic, off-centre -- the kind of
grid tightening leaves).  tests/test_train_objective_model.py checks on the CPU that these comparisons say something."""

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import train_objective_model as tom
from tests.test_hip_tv import STEPPERS, STORAGES
from thr3ed_atom_amd import ops
from thr3ed_atom_amd.trainers import PosedImagesInMemory, TrainStepper
from thr3ed_atom_amd.voxels import unpack_storage

pytestmark = pytest.mark.gpu


def make_stepper(dev, name, storage, config, monkeypatch):
    c = tom.CASES[name]
    dens, feat, _, _, near, far, _ = tom.case_inputs(name)
    if config == "fused-binned-pieces":
        monkeypatch.setattr(ops, "KERNEL_TIMER", ops.KernelTimer())
    grid = rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*c["voxel"]), grid_location=rf.VoxelGridLocation(*c["location"]),
                        density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=tom.RHO,
                        tunable=True, storage=storage)
    cfg = rf.SHVoxGridRenderConfig(c["S"], rf.CameraBounds(near, far), perturb_sampled_points=True, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    stepper = TrainStepper(model, tom.NUM_RAYS, learning_rate=tom.LR, data_parallel=False, tv_epsilon=tom.TV_EPSILON, **tom.WEIGHTS, **STEPPERS[config])
    # what the options resolved to
    assert stepper.fuse_optimizer is False and stepper.flat.deferred is False and stepper.exchange == "dense"
    assert stepper.merged_bricks == (config in ("fused-binned-merged", "fused-binned-pieces"))
    return grid, stepper


def spy_on_the_bucket(stepper, grid):
    """the gradient bucket as Adam is about to read it, in the reference layout: seen["grad"] = (densities', features')"""
    seen = {}
    real_step = stepper.optimizer.step

    def spy(*args, **kwargs):
        first, second = (None if g is None else g.clone() for g in stepper.flat.views_for_accumulation())
        seen["grad"] = unpack_storage(first, second, grid.storage, grid.grid_dims)
        return real_step(*args, **kwargs)

    stepper.optimizer.step = spy
    return seen


def check_bucket(tag, seen, ev):
    """every element of both tensors against the float64 gradient of L at the bar of the model"""
    gd, gf = seen["grad"]
    ratio_d, ratio_f = tom.worst_ratio(gd, ev["gd"], ev["bar_d"]), tom.worst_ratio(gf, ev["gf"], ev["bar_f"])
    print(f"combined {tag}: bucket max |g - g64| / bar = {ratio_d:.3f} D, {ratio_f:.3f} F")
    assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gf).all())
    assert tuple(gd.shape) == tuple(ev["gd"].shape) and tuple(gf.shape) == tuple(ev["gf"].shape)
    assert ratio_d <= 1.0 and ratio_f <= 1.0, (ratio_d, ratio_f)


def check_stats(stats, ev):
    assert abs(float(stats.specular_loss) - ev["specular_loss"]) <= 1e-5
    assert abs(float(stats.diffuse_loss) - ev["diffuse_loss"]) <= 1e-5
    assert abs(float(stats.distortion) - ev["distortion_sum"]) <= ev["distortion_bar"]
    np.testing.assert_allclose([float(stats.tv_density), float(stats.tv_features)], [ev["tv_density"], ev["tv_features"]], rtol=1e-5)


def case_batch(dev, name):
    _, _, o, d, _, _, pixels = tom.case_inputs(name)
    return rf.Rays(o.to(dev), d.to(dev)), pixels.to(dev)


@pytest.mark.parametrize("name", list(tom.CASES))
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("config", list(STEPPERS))
def test_bucket_of_one_iteration_equals_the_float64_gradient(hip_device, monkeypatch, config, storage, name):
    ev = tom.trajectory(name)["evals"][0]
    grid, stepper = make_stepper(hip_device, name, storage, config, monkeypatch)
    seen = spy_on_the_bucket(stepper, grid)
    rays, pixels = case_batch(hip_device, name)
    torch.manual_seed(tom.SEED)
    stats = stepper.step_on(rays, pixels)
    check_stats(stats, ev)
    check_bucket(f"{config} {storage} {name} step 0", seen, ev)
    stepper.flat.detach()


FOURTH = {"reference": "fused-atomic", "split": "fused-binned-merged", "bricked": "autograd"}  # the configuration that runs a fourth iteration


@pytest.mark.parametrize("name", list(tom.CASES))
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("config", list(STEPPERS))
def test_three_iterations_equal_float64_adam(hip_device, monkeypatch, config, storage, name):
    """EVERY element within its Adam bar of the float64 trajectory; an element whose float64 gradient is exactly 0 in every step keeps
    its bits; and on one configuration per storage a fourth iteration, whose bucket must be the float64 gradient of L at the
    parameters the three steps left (read back from the grid): what an earlier iteration left in the bucket fails here."""
    dens, feat = tom.case_inputs(name)[:2]
    tr = tom.trajectory(name)
    grid, stepper = make_stepper(hip_device, name, storage, config, monkeypatch)
    rays, pixels = case_batch(hip_device, name)
    for it in range(tom.STEPS):
        torch.manual_seed(tom.SEED + it)
        stepper.step_on(rays, pixels)
    got_d, got_f = grid.densities.detach().cpu(), grid.features.detach().cpu()
    ratio_d, ratio_f = tom.worst_ratio(got_d, tr["dens"], tr["bar_d"]), tom.worst_ratio(got_f, tr["feat"], tr["bar_f"])
    print(f"combined {config} {storage} {name}: after {tom.STEPS} steps max |theta - theta64| / Adam bar = {ratio_d:.3f} D, {ratio_f:.3f} F")
    assert ratio_d <= 1.0 and ratio_f <= 1.0, (ratio_d, ratio_f)
    for got, start, zero in ((got_d, dens, tr["zero_d"]), (got_f, feat, tr["zero_f"])):
        assert np.array_equal(got.numpy()[zero.numpy()].view(np.uint32), start.numpy()[zero.numpy()].view(np.uint32))
    if FOURTH[storage] == config:
        keys = tom.step_keys(tom.STEPS)
        ev = tom.case_objective(name, got_d, got_f, keys)
        assert ev["band"] == (0, 0)  # (of the parameters the GPU steps left: float32 and float64 decide every ReLU gate alike)
        seen = spy_on_the_bucket(stepper, grid)
        torch.manual_seed(tom.SEED + tom.STEPS)
        stats = stepper.step_on(rays, pixels)
        check_stats(stats, ev)
        check_bucket(f"{config} {storage} {name} step {tom.STEPS}", seen, ev)
    stepper.flat.detach()


@pytest.mark.parametrize("name", list(tom.CASES))
@pytest.mark.parametrize("storage", ["split", "bricked"])
@pytest.mark.parametrize("config", ["fused-binned-merged", "fused-atomic"])
def test_the_trainers_own_batch(hip_device, monkeypatch, config, storage, name):
    """stepper.step(dataset, image_ids): rf_train_step draws the batch into the executor's buffers (fused-binned-merged) or select()
    draws it (fused-atomic).  The rays and pixels the step used are, bit for bit, those the float64 side rebuilt from the seed; then
    the bucket as above -- a distortion launch on other rays, another jitter stream or another first_ray than the specular render's
    misses the bar."""
    images, pose_mat = tom.trainer_dataset()
    o, d, pixels, _ = tom.trainer_batch()
    ev = tom.trainer_batch_objective(name)
    grid, stepper = make_stepper(hip_device, name, storage, config, monkeypatch)
    _, _, _, _, near, far, _ = tom.case_inputs(name)
    dataset = PosedImagesInMemory(images.to(hip_device), pose_mat.to(hip_device), rf.CameraIntrinsics(tom.BATCH_HW, tom.BATCH_HW, tom.BATCH_FOCAL),
                                  rf.CameraBounds(near, far))
    seen = spy_on_the_bucket(stepper, grid)
    used = {}
    if config == "fused-atomic":
        real_step_on = stepper.step_on

        def step_on(rays, px, *args, **kwargs):
            used["batch"] = (rays.origins.clone(), rays.directions.clone(), px.clone())
            return real_step_on(rays, px, *args, **kwargs)

        stepper.step_on = step_on
    torch.manual_seed(tom.BATCH_SEED)
    stats = stepper.step(dataset, torch.tensor(tom.BATCH_IMAGE_IDS))
    if config == "fused-binned-merged":
        used["batch"] = tuple(stepper._exec[k][: tom.NUM_RAYS] for k in ("origins", "directions", "pixels"))
    for got, want in zip(used["batch"], (o, d, pixels)):
        assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want)
    check_stats(stats, ev)
    check_bucket(f"{config} {storage} {name} own batch", seen, ev)
    stepper.flat.detach()
