"""The hand-over at the end of a stage on the GPU -- node_max_weights, prune_voxel_grid, tighten_voxel_grid, in the trainer's order --
against the chain of the float64 models (tests/stage_handover_model.py).  The pieces have their own tests; this file holds what the
chain alone decides: the keep mask and its counts, the content box after (and without) pruning, the new dims and box, every node of
the resampled tensors, and the render of the result.  tests/test_stage_handover_model.py checks the conditions on the CPU."""
import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import node_weights_model as nm
from tests import stage_handover_model as sh
from tests.test_hip_resample import EVAL_BOUND
from thr3ed_atom_amd.resampling import tightened_dims

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the parity bar on colour and acc (2 TOL on depth): tests/test_hip_parity.py
RENDER_VIEW = 4  # the view from above


def scene(dev, storage):
    dens, feat = nm.scene_grid()
    grid = rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*nm.SCENE_VOXEL), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=nm.SCENE_RHO, tunable=False, storage=storage)
    near, far = sh.scene_bounds()
    bounds = rf.CameraBounds(near, far)
    cfg = rf.SHVoxGridRenderConfig(nm.SCENE_SAMPLES, bounds, perturb_sampled_points=False, white_bkgd=True)
    (h, w, focal), poses = nm.scene_views()
    return grid, rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev), rf.CameraIntrinsics(h, w, focal), poses, bounds, cfg


@pytest.mark.parametrize("storage", ["reference", "split", "bricked"])
def test_prune_then_tighten_equals_the_chain_of_the_models(hip_device, storage):
    c = sh.chain()
    grid, model, intr, poses, bounds, cfg = scene(hip_device, storage)
    # without the pruning step the box reaches the speck's own node: the order of the two steps is part of the contract
    assert rf.content_bounds(grid, sh.TIGHTEN_THRESHOLD) == c["box_unpruned"] and c["box_unpruned"][0][0] == nm.SPECK[0]
    early, early_stats = rf.tighten_voxel_grid(grid, sh.TIGHTEN_THRESHOLD, margin=sh.MARGIN)
    assert early.grid_dims == (19, 16, 16) and early_stats.passing_nodes == c["box_unpruned"][2]

    # the statistic and the keep mask: exact
    M = rf.node_max_weights(model, poses, intr, bounds, nm.SCENE_SAMPLES)
    Mh = M.cpu().numpy().astype(np.float64)
    err_m = float(np.abs(Mh - c["M"]).max())
    assert err_m <= sh.M_BAR
    assert np.array_equal(nm.keep_mask(Mh, nm.SCENE_TAU, sh.DILATE), c["keep"])
    stats = rf.prune_voxel_grid(grid, M, nm.SCENE_TAU, dilate=sh.DILATE)
    assert (stats.kept, stats.pruned) == c["counts"]
    assert np.array_equal(grid.densities.detach().cpu().numpy().view(np.uint32), c["pruned_densities"].view(np.uint32))

    # the content box after pruning: exactly the shell
    assert rf.content_bounds(grid, sh.TIGHTEN_THRESHOLD) == c["box"] == ((5, 5, 5), (18, 18, 18), c["box"][2])
    tight, tstats = rf.tighten_voxel_grid(grid, sh.TIGHTEN_THRESHOLD, margin=sh.MARGIN, num_nodes=sh.BUDGET)
    assert tstats.passing_nodes == c["box"][2] and tstats.old_dims == nm.SCENE_DIMS
    assert tight.grid_dims == tstats.new_dims == c["new_dims"] == tightened_dims(c["crop_dims"], nm.SCENE_VOXEL, sh.BUDGET)
    assert tight.storage == storage and tstats.new_aabb == tight.aabb
    for (lo, hi), (mlo, mhi) in zip(tight.aabb, c["new_aabb"]):
        assert abs(lo - mlo) <= 1e-12 and abs(hi - mhi) <= 1e-12
    # (with margin 1 the crop is nodes 4..19: the box runs from the lower face of voxel 4 to the upper face of voxel 19)
    for (lo, hi), v in zip(tight.aabb, nm.SCENE_VOXEL):
        assert abs(lo - (-1.5 + 4 * v)) <= 1e-12 and abs(hi - (-1.5 + 20 * v)) <= 1e-12

    # every node of the resampled tensors: the bar tests/test_hip_resample.py applies to a non-dyadic scale (the float32 evaluation
    # bound on the source's largest value -- here per tensor, which is tighter: the shell's 1e6 does not widen the features' bar --
    # plus the priced rounding of s)
    got_d, got_f = tight.densities.detach().cpu().numpy().astype(np.float64), tight.features.detach().cpu().numpy().astype(np.float64)
    worst = []
    for got, want, slope, vmax in ((got_d, c["densities"], c["slope_d"], c["source_max"][0]), (got_f, c["features"], c["slope_f"], c["source_max"][1])):
        assert got.shape == want.shape
        bar = EVAL_BOUND * vmax + slope * 2.0**-23 * max(c["crop_dims"])
        worst.append(float((np.abs(got - want) / bar).max()))
    print(f"handover {storage}: max |M - M64| = {err_m:.3e} (bar {sh.M_BAR:.0e}); resampled max |v - v64| / bar = {worst[0]:.3f} D, {worst[1]:.3f} F")
    assert max(worst) <= 1.0, worst

    # the render of the result against the oracle's render of the MODEL chain's tensors
    o, d = sh.view_rays(RENDER_VIEW)
    near, far = sh.scene_bounds()
    ref = orc.render(torch.from_numpy(c["densities"]).float(), torch.from_numpy(c["features"]).float(), o, d, c["new_aabb"], near, far, nm.SCENE_SAMPLES,
                     nm.SCENE_RHO, "relu", white_bkgd=True)
    with torch.no_grad():
        out = rf.VolumetricModel(tight, rf.render_sh_voxel_grid, cfg, device=hip_device).render_rays(rf.Rays(o.to(hip_device), d.to(hip_device)))
    n = o.shape[0]
    errs = {}
    for key, got, bar in (("colour", out.colour, TOL), ("acc", out.extra["accumulated_weight"], TOL), ("depth", out.depth, 2 * TOL)):
        errs[key] = float(np.abs(got.cpu().numpy().astype(np.float64).reshape(n, -1) - ref[key].numpy().astype(np.float64).reshape(n, -1)).max())
        assert errs[key] <= bar, (key, errs[key])
    assert float(ref["acc"].max()) > 0.5 and float(ref["acc"].min()) < 1e-6  # the shell is hit and missed
    print(f"handover {storage}: render of the tightened grid, max error colour {errs['colour']:.3e}, acc {errs['acc']:.3e}, depth {errs['depth']:.3e}")


# --------------------------------------------------------------------------------------------
# one training run with everything on, one with everything at its default
# --------------------------------------------------------------------------------------------
NEW_KEYS = ("tv_density", "tv_features", "distortion", "pruned_nodes", "kept_nodes", "new_dims", "tightened", "test_ssim")


def _kind(row):
    for key, kind in (("specular_loss", "summary"), ("test_psnr", "test"), ("pruned_nodes", "prune"), ("new_dims", "tighten")):
        if key in row:
            return kind
    raise AssertionError(f"a history row of no known kind: {row}")


def test_one_run_with_every_feature_on_and_one_with_every_default(hip_device, tmp_path, monkeypatch):
    from tests.test_hip_tighten import RHO, VOXEL, _training_scene
    from tests.helpers import procedural_grid
    from thr3ed_atom_amd import ops, trainers

    data, cfg, poses, intr = _training_scene(hip_device)
    held_out = trainers.PosedImagesInMemory(data.images[:1], data.poses[:1], intr, data.camera_bounds)
    built_on = []

    class Recording(trainers.TrainStepper):
        def __init__(self, vol_mod, *args, **kwargs):
            built_on.append(tuple(vol_mod.thre3d_repr.grid_dims))
            super().__init__(vol_mod, *args, **kwargs)

    monkeypatch.setattr(trainers, "TrainStepper", Recording)

    def train(out_dir, **kwargs):
        torch.manual_seed(3)
        d0, f0 = procedural_grid((16, 16, 16), 3, 77)
        # content in the middle only, so that there is a box to find after a handful of iterations (as tests/test_hip_tighten.py)
        r = np.indices((16, 16, 16)).astype(np.float32) - 7.5
        d0 = torch.where(torch.from_numpy((np.abs(r).max(0) < 4.0))[..., None], d0.abs(), -d0.abs() - 1.0)
        grid = rf.VoxelGrid(d0.to(hip_device), f0.to(hip_device), rf.VoxelSize(*VOXEL), density_preactivation=torch.nn.Identity(),
                            density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        history = []
        model = trainers.train_sh_vox_grid_vol_mod_with_posed_images(
            model, data, out_dir, test_dataset=held_out, ray_batch_size=256, num_stages=2, num_iterations_per_stage=12, image_batch_cache_size=4, learning_rate=0.03,
            lr_decay_steps_per_stage=10, summary_freq=100, save_freq=1000, test_freq=1000, log=lambda s: None, history=history, random_initializer=lambda t: t, **kwargs)
        return model, history

    model, history = train(tmp_path, tv_density_weight=1e-2, tv_feature_weight=1e-3, distortion_weight=1e-2, prune_threshold=1e-3, tighten_threshold=0.0,
                           report_ssim=True)
    # per stage and in this order: the summary rows (first and last iteration), the held-out test, the pruning row, and after stage 1
    # the tightening row
    assert [(_kind(h), h.get("stage")) for h in history] == [("summary", 1), ("summary", 1), ("test", None), ("prune", 1), ("tighten", 1),
                                                              ("summary", 2), ("summary", 2), ("test", None), ("prune", 2)]
    for h in history:
        if _kind(h) == "summary":
            assert all(np.isfinite(h[k]) and h[k] >= 0.0 for k in ("specular_loss", "diffuse_loss", "tv_density", "tv_features", "distortion")), h
            assert h["tv_density"] > 0.0 and h["tv_features"] > 0.0
        elif _kind(h) == "test":
            assert -1.0 <= h["test_ssim"] <= 1.0 and np.isfinite(h["test_psnr"])
        elif _kind(h) == "prune":
            assert h["pruned_nodes"] + h["kept_nodes"] == int(np.prod(built_on[h["stage"] - 1])) and h["kept_nodes"] > 0
    tighten = history[4]
    assert tighten["tightened"] and tighten["passing_nodes"] > 0 and tighten["old_dims"] == (8, 8, 8)
    # the stage-2 stepper was built on the tightened dims
    assert built_on == [(8, 8, 8), tighten["new_dims"]]
    grid = model.thre3d_repr
    assert grid.grid_dims == tighten["new_dims"] and tuple(grid.aabb) == tuple(tighten["new_aabb"])
    # the final checkpoint reloads to the same bits, and evaluates
    loaded, _ = rf.create_volumetric_model_from_saved_model(tmp_path / "saved_models" / "model_final.pth", rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    assert loaded.thre3d_repr.grid_dims == grid.grid_dims and tuple(loaded.thre3d_repr.aabb) == tuple(grid.aabb)
    assert torch.equal(loaded.thre3d_repr.densities.detach(), grid.densities.detach()) and torch.equal(loaded.thre3d_repr.features.detach(), grid.features.detach())
    scores = trainers.evaluate_sh_vox_grid_vol_mod_with_posed_images(loaded, held_out)
    assert np.isfinite(scores["psnr"]) and np.isfinite(scores["ssim"]) and -1.0 <= scores["ssim"] <= 1.0

    # every option at its default: no launch of the four features, none of their keys
    def forbidden(*args, **kwargs):
        raise AssertionError("a launch of a feature that is off")

    for name in ("tv_grad_raw", "distortion_raw", "node_max_weight_raw", "prune_grid_raw", "node_bounds_raw", "resample_grid_raw"):
        monkeypatch.setattr(ops, name, forbidden)
    del built_on[:]
    model_off, history_off = train(None)
    assert [_kind(h) for h in history_off] == ["summary", "summary", "test"] * 2
    assert not any(k in h for h in history_off for k in NEW_KEYS)
    assert built_on == [(8, 8, 8), (16, 16, 16)] and model_off.thre3d_repr.grid_dims == (16, 16, 16)
