"""Cropping and tightening end to end on the GPU: the render of a cropped field equals the render of the original within what
coordinate rounding alone causes (measured on the oracle, never on the code under test), tighten_voxel_grid follows DVGO's rule and
renders like the oracle, the trainer tightens between stages, and the command-line tool round-trips a checkpoint."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests.helpers import hash_uniform, hotdog_like_camera, procedural_grid, sparse_scene_grid
from thr3ed_atom_amd import ops
from thr3ed_atom_amd.resampling import tightened_dims
from thr3ed_atom_amd.trainers import PosedImagesInMemory, train_sh_vox_grid_vol_mod_with_posed_images

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the project's parity bar on colour and acc (2 TOL on depth): tests/test_hip_parity.py
DIMS, F, S, RHO = (16, 16, 16), 12, 32, 100.0 / 3.0
VOXEL = (3.0 / 16,) * 3
STORAGES = ["reference", "split", "bricked"]


@functools.lru_cache(maxsize=None)
def blob_field():
    """a positive-density blob in the nodes [5..10]^3, negative densities everywhere else; SH degree 1"""
    dens, feat = procedural_grid(DIMS, F, 51)
    dens = -dens.abs() - 0.01
    dens[5:11, 5:11, 5:11] = torch.from_numpy(hash_uniform((6, 6, 6, 1), 52, 0.02, 0.3))
    return dens, feat


@functools.lru_cache(maxsize=None)
def rays():
    cam = hotdog_like_camera()
    pose = rf.pose_spherical(40.0, -35.0, cam["radius"])
    o, d = orc.cast_rays(8, 8, 14.0, torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))  # 64 rays, the box fills the frame
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), cam["near"], cam["far"]


def make_grid(dev, dens, feat, storage="split", location=(0.0, 0.0, 0.0), voxel=VOXEL):
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*voxel), rf.VoxelGridLocation(*location), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=False, storage=storage)


def oracle_render(dens, feat, dims, voxel, location, dtype):
    o, d, near, far = rays()
    out = orc.render(dens, feat, o.to(dtype), d.to(dtype), orc.make_aabb(dims, voxel, location), near, far, S, RHO, "relu")
    return {k: out[k].reshape(o.shape[0], -1).numpy().astype(np.float64) for k in ("colour", "depth", "acc")}


def hip_render(grid, dev):
    o, d, near, far = rays()
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=False, white_bkgd=False)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    with torch.no_grad():
        out = model.render_rays(rf.Rays(o.to(dev), d.to(dev)))
    n = o.shape[0]
    return {"colour": out.colour.cpu().numpy().astype(np.float64).reshape(n, -1), "depth": out.depth.cpu().numpy().astype(np.float64).reshape(n, -1),
            "acc": out.extra["accumulated_weight"].cpu().numpy().astype(np.float64).reshape(n, -1)}


@functools.lru_cache(maxsize=None)
def oracle_spread():
    """(float64 difference, float32 difference) per output between the oracle's renders of the cropped and the original field: the
    first shows that cropping changes nothing, the second what the rounding of coordinates in a different box alone causes"""
    dens, feat = blob_field()
    cd, cf = dens[4:12, 4:12, 4:12].contiguous(), feat[4:12, 4:12, 4:12].contiguous()
    location = tuple(-1.5 + (4 + 11 + 1) / 2 * v for v in VOXEL)
    out = {}
    for dtype in (torch.float64, torch.float32):
        a = oracle_render(dens, feat, DIMS, VOXEL, (0.0, 0.0, 0.0), dtype)
        b = oracle_render(cd, cf, (8, 8, 8), VOXEL, location, dtype)
        out[dtype] = {k: np.abs(a[k] - b[k]) for k in a}
        if dtype == torch.float64:
            assert a["acc"].max() > 0.5 and (a["acc"] < 1e-6).any()  # the blob is hit and missed
    return out[torch.float64], out[torch.float32]


@pytest.mark.parametrize("storage", STORAGES)
def test_the_render_of_a_cropped_field_equals_the_render_of_the_original(hip_device, storage):
    """Every cell with a positive corner keeps all 8 corners and the new border blends non-positive nodes with 0, so sigma is
    unchanged along every ray.  The float64 oracle shows the equality; the float32 oracle's difference between the two grids is the
    spread coordinate rounding causes, and the bar is |hip(cropped) - hip(original)| <= 2 x that + TOL."""
    d64, d32 = oracle_spread()
    for k in d64:
        assert d64[k].max() <= 1e-9, (k, d64[k].max())
    dens, feat = blob_field()
    grid = make_grid(hip_device, dens, feat, storage)
    assert rf.content_bounds(grid, 0.0) == ((5, 5, 5), (10, 10, 10), 216)
    crop = rf.crop_voxel_grid(grid, (5, 5, 5), (10, 10, 10), margin=1)
    assert crop.grid_dims == (8, 8, 8) and crop.storage == storage and torch.equal(crop.densities.cpu(), dens[4:12, 4:12, 4:12])
    a, b = hip_render(grid, hip_device), hip_render(crop, hip_device)
    for k in a:
        diff = np.abs(a[k] - b[k])
        print(f"crop render {storage} {k}: hip diff {diff.max():.3e}, oracle diff float64 {d64[k].max():.3e} float32 {d32[k].max():.3e}")
        assert (diff <= 2 * d32[k] + TOL).all(), (k, diff.max())


@pytest.mark.parametrize("storage", STORAGES)
def test_tighten_follows_the_rule_and_renders_like_the_oracle(hip_device, storage):
    dens, feat = blob_field()
    grid = make_grid(hip_device, dens, feat, storage)
    budget = 16**3
    tight, stats = rf.tighten_voxel_grid(grid, 0.0, margin=1, num_nodes=budget)
    assert stats.passing_nodes == 216 and stats.old_dims == DIMS and stats.old_aabb == grid.aabb and stats.new_aabb == tight.aabb
    # inside the old box, around the blob's box (nodes 5..10: their voxels span [5, 11] v from the old lower face)
    for (lo, hi), (olo, ohi), v in zip(tight.aabb, grid.aabb, VOXEL):
        assert olo <= lo <= olo + 5 * v and olo + 11 * v <= hi <= ohi
    # the rule: the cropped box holds 8^3 voxels of edge v, so budget cubic voxels in it are 16 per axis
    extent = [8 * v for v in VOXEL]
    edge = (extent[0] * extent[1] * extent[2] / budget) ** (1.0 / 3.0)
    want = tuple(max(2, int(np.floor(e / edge + 0.5))) for e in extent)
    assert tight.grid_dims == want == stats.new_dims == tightened_dims((8, 8, 8), VOXEL, budget) == (16, 16, 16)
    assert np.prod([n - 0.5 for n in want]) <= budget <= np.prod([n + 0.5 for n in want])  # within the rounding of the rule
    assert all(abs(tv - e / n) <= 1e-12 for tv, e, n in zip(tight.voxel_size, extent, want))
    # the render of the returned grid against the oracle's render of the very same tensors, at the parity bars
    location = tuple(tight.get_config_dict()["grid_location"])
    ref = oracle_render(tight.densities.cpu(), tight.features.cpu(), tight.grid_dims, tuple(tight.voxel_size), location, torch.float32)
    got = hip_render(tight, hip_device)
    assert ref["acc"].max() > 0.5
    for k, bar in (("colour", TOL), ("acc", TOL), ("depth", 2 * TOL)):
        assert np.abs(got[k] - ref[k]).max() <= bar, (k, np.abs(got[k] - ref[k]).max())
    # an empty field comes back as it is
    empty = make_grid(hip_device, -dens.abs(), feat, storage)
    same, stats = rf.tighten_voxel_grid(empty, 0.0, num_nodes=budget)
    assert same is empty and stats.passing_nodes == 0 and stats.new_dims == DIMS


def _training_scene(dev):
    cam = hotdog_like_camera()
    gd, gf = sparse_scene_grid((16, 16, 16), 3, 11)
    gt = rf.VoxelGrid((gd * 3.0).to(dev), gf.to(dev), rf.VoxelSize(*VOXEL), density_preactivation=torch.nn.Identity(),
                      density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=False)
    bounds = rf.CameraBounds(cam["near"], cam["far"])
    cfg = rf.SHVoxGridRenderConfig(32, bounds, perturb_sampled_points=False, white_bkgd=True)
    gt_model = rf.VolumetricModel(gt, rf.render_sh_voxel_grid, cfg, device=dev)
    intr = rf.CameraIntrinsics(24, 24, 33.0)
    poses = [rf.pose_spherical(90.0 * k, -30.0, cam["radius"]) for k in range(4)]
    images = torch.stack([gt_model.render(p, intr).colour.permute(2, 0, 1) for p in poses])
    pose_mat = torch.stack([torch.cat([p.rotation, p.translation], dim=1) for p in poses]).to(dev)
    return PosedImagesInMemory(images, pose_mat, intr, bounds), cfg, poses, intr


def test_the_trainer_tightens_between_stages_and_is_untouched_when_off(hip_device, tmp_path, monkeypatch):
    data, cfg, poses, intr = _training_scene(hip_device)

    def train(out_dir=None, **kwargs):
        torch.manual_seed(3)
        d0, f0 = procedural_grid((16, 16, 16), 3, 77)
        # an initialisation with content in the middle only, so that there is a box to find after a handful of iterations
        r = np.indices((16, 16, 16)).astype(np.float32) - 7.5
        d0 = torch.where(torch.from_numpy((np.abs(r).max(0) < 4.0))[..., None], d0.abs(), -d0.abs() - 1.0)
        grid = rf.VoxelGrid(d0.to(hip_device), f0.to(hip_device), rf.VoxelSize(*VOXEL), density_preactivation=torch.nn.Identity(),
                            density_postactivation=torch.nn.ReLU(), expected_density_scale=RHO, tunable=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        history = []
        model = train_sh_vox_grid_vol_mod_with_posed_images(model, data, out_dir, ray_batch_size=256, num_stages=2, num_iterations_per_stage=12, image_batch_cache_size=4,
                                                            learning_rate=0.03, lr_decay_steps_per_stage=10, summary_freq=100, save_freq=1000, log=lambda s: None, history=history,
                                                            random_initializer=lambda t: t, **kwargs)
        return model, history, grid.aabb

    model, history, first_aabb = train(tmp_path, tighten_threshold=0.0, tighten_margin=1)
    rows = [h for h in history if "new_dims" in h]
    assert [r["stage"] for r in rows] == [1] and rows[0]["tightened"] and rows[0]["old_dims"] == (8, 8, 8) and rows[0]["passing_nodes"] > 0
    losses = [h["specular_loss"] for h in history if "specular_loss" in h]
    assert losses and all(np.isfinite(v) for v in losses)
    grid = model.thre3d_repr
    assert tuple(grid.aabb) == tuple(rows[0]["new_aabb"]) and grid.grid_dims == rows[0]["new_dims"]
    for (lo, hi), (olo, ohi) in zip(grid.aabb, first_aabb):
        assert olo - 1e-9 <= lo < hi <= ohi + 1e-9
    assert sum(hi - lo for lo, hi in grid.aabb) < sum(hi - lo for lo, hi in first_aabb)  # and it did get tighter
    # the budget of the second stage (16^3) within the rounding of the rule
    assert np.prod([n - 0.5 for n in grid.grid_dims]) <= 16**3 <= np.prod([n + 0.5 for n in grid.grid_dims])
    # the checkpoint reloads and renders
    loaded, _ = rf.create_volumetric_model_from_saved_model(tmp_path / "saved_models" / "model_final.pth", rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    assert loaded.thre3d_repr.grid_dims == grid.grid_dims and tuple(loaded.thre3d_repr.aabb) == tuple(grid.aabb)
    assert torch.equal(loaded.thre3d_repr.densities.detach(), grid.densities.detach())
    frame = loaded.render(poses[0], intr).colour
    assert frame.shape[:2] == (24, 24) and bool(torch.isfinite(frame).all())

    # off: nothing of the feature is launched, no row
    def forbidden(*args, **kwargs):
        raise AssertionError("a tightening launch in a run with tighten_threshold=None")

    monkeypatch.setattr(ops, "node_bounds_raw", forbidden)
    monkeypatch.setattr(ops, "resample_grid_raw", forbidden)
    model_off, history_off, _ = train(None, tighten_threshold=None, tighten_margin=3)
    assert not any("new_dims" in h for h in history_off) and model_off.thre3d_repr.grid_dims == (16, 16, 16)
    assert tuple(model_off.thre3d_repr.aabb) == tuple(first_aabb)


def test_cli_crop_round_trip(hip_device, tmp_path):
    """scripts/crop_sh_based_voxel_grid.py on a tiny checkpoint: the written field is what tighten_voxel_grid returns in process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dens, feat = blob_field()
    cam = hotdog_like_camera()
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False)
    grid = make_grid(hip_device, dens, feat, "reference")
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    src, dst = tmp_path / "model.pth", tmp_path / "cropped.pth"
    torch.save(model.get_save_info(extra_info={"note": "kept"}), src)
    r = subprocess.run([sys.executable, "scripts/crop_sh_based_voxel_grid.py", "-i", str(src), "-o", str(dst), "--threshold", "0", "--margin", "1", "--num_nodes", "1000"],
                       cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "dims: (16, 16, 16) -> (10, 10, 10)" in r.stdout and "nodes above the threshold: 216" in r.stdout
    want, _ = rf.tighten_voxel_grid(grid, 0.0, 1, num_nodes=1000)
    loaded, extra = rf.create_volumetric_model_from_saved_model(dst, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    got = loaded.thre3d_repr
    assert extra == {"note": "kept"} and got.grid_dims == (10, 10, 10) and tuple(got.aabb) == tuple(want.aabb)
    assert torch.equal(got.densities.detach(), want.densities.detach()) and torch.equal(got.features.detach(), want.features.detach())
    o, d, near, far = rays()
    out = loaded.render_rays(rf.Rays(o.to(hip_device), d.to(hip_device)))
    assert bool(torch.isfinite(out.colour).all()) and float(out.extra["accumulated_weight"].max()) > 0.5
