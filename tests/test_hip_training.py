"""Training-side parity on the GPU: the trainer core, the flat gradient bucket, fused Adam,
PSNR after equal steps, exact empty-space skipping, checkpoints, and size-independent properties at the full
BASELINE.json size.  All through the C ABI; the oracle / torch references are the checkers only."""
import os

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from thr3ed_atom_amd import ops
from thr3ed_atom_amd.optim import FlatGrid, FusedAdam
from thr3ed_atom_amd.trainers import PosedImagesInMemory, TrainStepper, train_sh_vox_grid_vol_mod_with_posed_images
from oracle import relu_field_oracle as orc
from tests.helpers import hash_uniform, hotdog_like_camera, identity_regime, load_golden, procedural_grid, signed_density_grid, sparse_scene_grid

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.asarray(a))


def relu_grid(dev, dens, feat, G, rho=100.0 / 3.0, tunable=True, storage="reference"):
    return rf.VoxelGrid(
        dens.clone().to(dev),
        feat.clone().to(dev),
        rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G),
        density_preactivation=torch.nn.Identity(),
        density_postactivation=torch.nn.ReLU(),
        expected_density_scale=rho,
        tunable=tunable,
        storage=storage,
    )


@pytest.mark.parametrize("policy", ["binned-on-every-grid", "production"])
@pytest.mark.parametrize("fused", [True, False, "autograd-unpaired"])
@pytest.mark.parametrize("storage", ["reference", "split", "bricked"])
def test_g9_reference_trainer_trajectory(hip_device, monkeypatch, storage, fused, policy):
    """TrainStepper fed the batches the REAL reference trainer selected reproduces its losses and parameters.  ``policy``:
    tests/conftest.py keeps the binned machinery on every grid; "production" removes that override, so that the path a user gets --
    backward="auto": the atomic adjoint + rf_adam_step on this 16^3 grid (8 bricks < 256) -- follows the reference trainer too
    (modules/trainers.py:278-341)."""
    if policy == "production":
        monkeypatch.delenv("RF_AUTO_BINNED_MIN_BRICKS", raising=False)
    if fused == "autograd-unpaired":  # (fused=False renders the iteration's pair as ONE autograd node by default: here one node per render)
        monkeypatch.setattr(ops, "PAIR_RENDERS", False)
        fused = False
    g = load_golden("g9_trainer_trajectory.npz")
    G, deg, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F = 3 * (deg + 1) ** 2
    grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage=storage)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]), fused=fused)
    if policy == "production":
        assert stepper.backward == "atomic" and not stepper.fuse_optimizer and not stepper.flat.deferred
    for it in range(steps):
        rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
        stats = stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
        np.testing.assert_allclose(stats.specular_loss.item(), g["specular_loss"][it], rtol=1e-5)
        np.testing.assert_allclose(stats.diffuse_loss.item(), g["diffuse_loss"][it], rtol=1e-5)
        if it == 0:
            # Adam's first update is lr * g / (|g| + 1e-8): parameters whose gradient is ~1e-8 amplify float32
            # summation-order noise, so a handful of entries may differ visibly; EVERY entry whose gradient is not noise
            # (|g| > 1e-6, by the oracle's autograd on the same batch) must agree to 2e-5
            o, d, px = (T(g[k][0]) for k in ("origins", "directions", "pixels"))
            cd = T(hash_uniform((G, G, G, 1), 901)).requires_grad_(True)
            cf = T(hash_uniform((G, G, G, F), 900 + F)).requires_grad_(True)
            kw = dict(origins=o, directions=d, aabb=orc.make_aabb((G,) * 3, (3.0 / G,) * 3), near=float(g["near"]), far=float(g["far"]), num_samples=S,
                      density_scale=100.0 / 3.0, white_bkgd=True)
            (torch.nn.functional.l1_loss(orc.render(cd, cf, **kw)["colour"], px) + torch.nn.functional.l1_loss(orc.render(cd, cf, render_diffuse=True, **kw)["colour"], px)).backward()
            for ours, ref, grad in ((grid.densities, g["dens_after_step1"], cd.grad.numpy()), (grid.features, g["feat_after_step1"], cf.grad.numpy())):
                err = np.abs(ours.detach().cpu().numpy() - ref)
                firm = np.abs(grad) > 1e-6
                assert firm.sum() > 100 and err[firm].max() <= 2e-5, (int(firm.sum()), float(err[firm].max()))
                assert np.mean(err <= 2e-5) >= 0.999 and err.max() <= 0.03 * 2 + 1e-6
    dd = np.abs(grid.densities.detach().cpu().numpy() - g["dens_final"])
    df = np.abs(grid.features.detach().cpu().numpy() - g["feat_final"])
    assert np.mean(dd < 1e-4) > 0.99 and np.mean(df < 1e-4) > 0.99


def test_flat_bucket_gradients_equal_plain_autograd(hip_device):
    g = load_golden("g7_grid16_render.npz")
    dens, feat = procedural_grid((16, 16, 16), 27, 81)
    cam = hotdog_like_camera()
    cfg = rf.SHVoxGridRenderConfig(48, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    rays = rf.Rays(T(g["origins"]).to(hip_device), T(g["directions"]).to(hip_device))
    target = T(g["target"]).to(hip_device)
    grids = [relu_grid(hip_device, dens, feat, 16) for _ in range(2)]
    flat = FlatGrid(grids[1])
    assert grids[1].densities.data_ptr() == flat.flat_param.data_ptr()
    for grid in grids:
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        loss = torch.nn.functional.l1_loss(model.render_rays(rays).colour, target)
        loss = loss + torch.nn.functional.l1_loss(model.render_rays(rays, render_diffuse=True).colour, target)
        loss.backward()
    for a, b in ((grids[0].densities.grad, grids[1].densities.grad), (grids[0].features.grad, grids[1].features.grad)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-7 * float(a.abs().max()))
    assert grids[1].densities.grad.data_ptr() == flat.flat_grad.data_ptr()
    flat.zero_grad()
    assert float(flat.flat_grad.abs().max()) == 0.0
    # state_dict is still the reference's two tensors
    assert sorted(grids[1].state_dict().keys()) == ["_densities", "_features"]


def test_split_storage_is_the_same_grid(hip_device, tmp_path):
    """reference <-> split storage: same accessors, same state_dict keys/values, same renders (bit-exact
    interpolation recipe in both layouts), checkpoints interchangeable."""
    dens, feat = procedural_grid((9, 10, 11), 27, 13)
    ref = relu_grid(hip_device, dens, feat, 9, storage="reference")
    spl = relu_grid(hip_device, dens, feat, 9, storage="split")
    assert torch.equal(spl.densities, ref.densities) and torch.equal(spl.features, ref.features)
    sd_ref, sd_spl = ref.state_dict(), spl.state_dict()
    assert sorted(sd_spl.keys()) == sorted(sd_ref.keys()) == ["_densities", "_features"]
    assert all(torch.equal(sd_ref[k], sd_spl[k]) for k in sd_ref)
    assert [tuple(p.shape) for p in spl.parameters()] == [(9, 10, 11, 4), (9, 10, 11, 24)]
    cam = hotdog_like_camera()
    g7 = load_golden("g7_grid16_render.npz")
    rays = rf.Rays(T(g7["origins"]).to(hip_device), T(g7["directions"]).to(hip_device))
    cfg = rf.SHVoxGridRenderConfig(40, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    a, b = rf.render_sh_voxel_grid(ref, rays, cfg), rf.render_sh_voxel_grid(spl, rays, cfg)
    assert torch.equal(a.depth, b.depth) and torch.equal(a.extra["accumulated_weight"], b.extra["accumulated_weight"])
    np.testing.assert_allclose(a.colour.detach().cpu().numpy(), b.colour.detach().cpu().numpy(), rtol=0, atol=5e-7)
    # a checkpoint written from split storage loads into reference storage and vice versa
    model = rf.VolumetricModel(spl, rf.render_sh_voxel_grid, cfg, device=hip_device)
    torch.save(model.get_save_info(extra_info={}), tmp_path / "m.pth")
    for storage in ("reference", "split"):
        creator = lambda info, st=storage: rf.create_voxel_grid_from_saved_info_dict(info, storage=st)
        loaded, _ = rf.create_volumetric_model_from_saved_model(tmp_path / "m.pth", creator, device=hip_device)
        assert loaded.thre3d_repr.storage == storage
        assert torch.equal(loaded.thre3d_repr.features, ref.features) and torch.equal(loaded.thre3d_repr.densities, ref.densities)
    # writing through the accessors reaches the split tensors
    with torch.no_grad():
        spl.densities.mul_(2.0)
    spl.features = ref.features * 3.0
    assert torch.equal(spl.densities, ref.densities * 2.0) and torch.equal(spl.features, ref.features * 3.0)
    up = rf.scale_voxel_grid_with_required_output_size(spl, (12, 12, 12))
    assert up.storage == "split" and up.features.shape == (12, 12, 12, 27)


def test_bricked_storage_is_the_same_grid(hip_device, tmp_path):
    """reference <-> bricked storage (split channels, 8^3-node bricks contiguous, dims padded to multiples of 8): same
    accessors, same state_dict, bit-identical renders and gradients, checkpoints interchangeable."""
    dens, feat = procedural_grid((9, 10, 19), 27, 13)
    ref = relu_grid(hip_device, dens, feat, 9, storage="reference")
    brk = relu_grid(hip_device, dens, feat, 9, storage="bricked")
    assert torch.equal(brk.densities, ref.densities) and torch.equal(brk.features, ref.features)
    assert [tuple(p.shape) for p in brk.parameters()] == [(2, 2, 3, 8, 8, 8, 4), (2, 2, 3, 8, 8, 8, 24)]
    sd_ref, sd_brk = ref.state_dict(), brk.state_dict()
    assert sorted(sd_brk.keys()) == ["_densities", "_features"] and all(torch.equal(sd_ref[k], sd_brk[k]) for k in sd_ref)
    cam = hotdog_like_camera()
    g7 = load_golden("g7_grid16_render.npz")
    rays = rf.Rays(T(g7["origins"]).to(hip_device), T(g7["directions"]).to(hip_device))
    cfg = rf.SHVoxGridRenderConfig(40, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    spl = relu_grid(hip_device, dens, feat, 9, storage="split")
    a, b = rf.render_sh_voxel_grid(spl, rays, cfg), rf.render_sh_voxel_grid(brk, rays, cfg)
    assert torch.equal(a.colour, b.colour) and torch.equal(a.depth, b.depth)  # same arithmetic, different addresses
    target = T(g7["target"]).to(hip_device)
    torch.nn.functional.l1_loss(a.colour, target).backward()
    torch.nn.functional.l1_loss(b.colour, target).backward()
    for x, y in zip(spl.reference_gradients(), brk.reference_gradients()):
        np.testing.assert_allclose(y.cpu().numpy(), x.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(x.abs().max()))
    pts = T(hash_uniform((257, 3), 21, -0.9, 0.9)).to(hip_device)
    assert torch.equal(brk(pts), ref(pts))
    model = rf.VolumetricModel(brk, rf.render_sh_voxel_grid, cfg, device=hip_device)
    torch.save(model.get_save_info(extra_info={}), tmp_path / "m.pth")
    for storage in ("reference", "bricked"):
        creator = lambda info, st=storage: rf.create_voxel_grid_from_saved_info_dict(info, storage=st)
        loaded, _ = rf.create_volumetric_model_from_saved_model(tmp_path / "m.pth", creator, device=hip_device)
        assert loaded.thre3d_repr.storage == storage
        assert torch.equal(loaded.thre3d_repr.features, ref.features) and torch.equal(loaded.thre3d_repr.densities, ref.densities)
    brk.densities = ref.densities * 2.0
    brk.features = ref.features * 3.0
    assert torch.equal(brk.densities, ref.densities * 2.0) and torch.equal(brk.features, ref.features * 3.0)
    up = rf.scale_voxel_grid_with_required_output_size(brk, (12, 12, 12))
    assert up.storage == "bricked" and up.features.shape == (12, 12, 12, 27)


def test_fused_adam_matches_torch_adam(hip_device):
    dens, feat = procedural_grid((5, 6, 7), 27, 3)  # odd sizes: exercises the unaligned tail
    grid = relu_grid(hip_device, dens, feat, 5)
    ref_d = dens.clone().to(hip_device).requires_grad_(True)
    ref_f = feat.clone().to(hip_device).requires_grad_(True)
    ref_opt = torch.optim.Adam([{"params": [ref_d, ref_f], "lr": 0.03}], betas=(0.9, 0.999))
    flat = FlatGrid(grid)
    opt = FusedAdam(flat, lr=0.03)
    for step in range(6):
        gd = T(hash_uniform(tuple(dens.shape), 50 + step)).to(hip_device) * 1e-3
        gf = T(hash_uniform(tuple(feat.shape), 80 + step)).to(hip_device) * (1e-4 if step % 2 else 1.0)
        ref_d.grad, ref_f.grad = gd.clone(), gf.clone()
        ref_opt.step()
        flat.zero_grad()
        grid.densities.grad.copy_(gd)
        grid.features.grad.copy_(gf)
        opt.step(zero_grad=(step % 2 == 0))
        assert (float(flat.flat_grad.abs().max()) == 0.0) == (step % 2 == 0)
    np.testing.assert_allclose(grid.densities.detach().cpu().numpy(), ref_d.detach().cpu().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(grid.features.detach().cpu().numpy(), ref_f.detach().cpu().numpy(), rtol=0, atol=2e-6)


def _make_scene(dev, G, deg, n_views, hw, S):
    cam = hotdog_like_camera()
    F = 3 * (deg + 1) ** 2
    gd, gf = sparse_scene_grid((G, G, G), F, 11)
    gt = relu_grid(dev, gd * 3.0, gf, G, tunable=False)
    bounds = rf.CameraBounds(cam["near"], cam["far"])
    cfg = rf.SHVoxGridRenderConfig(S, bounds, perturb_sampled_points=False, white_bkgd=True)
    gt_model = rf.VolumetricModel(gt, rf.render_sh_voxel_grid, cfg, device=dev)
    intr = rf.CameraIntrinsics(hw, hw, hw * 1.4)
    poses = [rf.pose_spherical(360.0 / n_views * k, -30.0, cam["radius"]) for k in range(n_views)]
    images = torch.stack([gt_model.render(p, intr).colour.permute(2, 0, 1) for p in poses])
    pose_mat = torch.stack([torch.cat([p.rotation, p.translation], dim=1) for p in poses]).to(dev)
    return PosedImagesInMemory(images, pose_mat, intr, bounds), cfg, poses


def test_psnr_after_equal_steps_matches_cpu_reference_path(hip_device):
    """north_star: PSNR within 0.05 dB of the reference after equal training steps.  Same initial grid, same
    ray batches, jitter off: the HIP trainer and the oracle (+ torch.optim.Adam, CPU) are trained side by
    side for 40 steps and evaluated on a held-out view."""
    G, deg, S, R, steps = 20, 1, 48, 1024, 40
    data, cfg, poses = _make_scene(hip_device, G, deg, 8, 40, S)
    F = 3 * (deg + 1) ** 2
    d0, f0 = procedural_grid((G, G, G), F, 77)
    grid = relu_grid(hip_device, d0, f0, G, storage="split")  # the layout the trainer and bench.py use
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, R, learning_rate=0.03)
    cd, cf = d0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    ref_opt = torch.optim.Adam([{"params": [cd, cf], "lr": 0.03}], betas=(0.9, 0.999))
    aabb = orc.make_aabb((G, G, G), (3.0 / G,) * 3)
    kw = dict(aabb=aabb, near=cfg.camera_bounds.near, far=cfg.camera_bounds.far, num_samples=S, density_scale=100.0 / 3.0, white_bkgd=True)
    torch.manual_seed(5)
    ids = torch.arange(7)  # view 7 is held out
    for it in range(steps):
        rays, pixels = stepper.select(data, ids)
        stats = stepper.step_on(rays, pixels)
        o, d, px = rays.origins.cpu(), rays.directions.cpu(), pixels.cpu()
        spec = torch.nn.functional.l1_loss(orc.render(cd, cf, origins=o, directions=d, **kw)["colour"], px)
        diff = torch.nn.functional.l1_loss(orc.render(cd, cf, origins=o, directions=d, render_diffuse=True, **kw)["colour"], px)
        ref_opt.zero_grad()
        (spec + diff).backward()
        ref_opt.step()
        # (the two trajectories differ by float32 summation order and 1-ulp optimizer arithmetic, and Adam amplifies that from
        # step to step: tight while they are still the same trajectory, then only the PSNR statement below)
        np.testing.assert_allclose(stats.specular_loss.item(), spec.item(), rtol=5e-4 if it < 10 else 3e-3)
    # held-out view
    held = data.images[7].permute(1, 2, 0)
    ours = model.render(poses[7], data.camera_intrinsics).colour
    ho, hd = orc.cast_rays(40, 40, data.camera_intrinsics.focal, poses[7].rotation, poses[7].translation)
    ref = orc.render(cd.detach(), cf.detach(), origins=ho.reshape(-1, 3), directions=hd.reshape(-1, 3), **kw)["colour"].reshape(40, 40, 3)
    psnr_hip = float(rf.mse2psnr(torch.nn.functional.mse_loss(ours, held)))
    psnr_ref = float(rf.mse2psnr(torch.nn.functional.mse_loss(ref, held.cpu())))
    assert psnr_hip > 12.0  # it actually learned something (start is ~7 dB)
    assert abs(psnr_hip - psnr_ref) <= 0.05, (psnr_hip, psnr_ref)


def test_full_trainer_two_stages_and_checkpoint_roundtrip(hip_device, tmp_path):
    data, cfg, poses = _make_scene(hip_device, 16, 0, 6, 32, 32)
    d0, f0 = procedural_grid((16, 16, 16), 3, 5)
    model = rf.VolumetricModel(relu_grid(hip_device, d0, f0, 16), rf.render_sh_voxel_grid, cfg, device=hip_device)
    cfg.perturb_sampled_points = True
    history = []
    torch.manual_seed(0)
    model = train_sh_vox_grid_vol_mod_with_posed_images(
        model, data, tmp_path, ray_batch_size=512, num_stages=2, num_iterations_per_stage=30, image_batch_cache_size=4,
        learning_rate=0.03, lr_decay_steps_per_stage=20, save_freq=1000, summary_freq=10, log=lambda s: None, history=history,
    )
    assert model.thre3d_repr.grid_dims == (16, 16, 16)  # 8^3 -> 16^3
    stage2 = [h for h in history if h.get("stage") == 2]
    assert stage2[-1]["specular_loss"] < history[0]["specular_loss"]
    assert stage2[-1]["specular_psnr"] > history[0]["specular_psnr"] + 1.0
    ckpt = tmp_path / "saved_models" / "model_final.pth"
    assert ckpt.exists()
    loaded, extra = rf.create_volumetric_model_from_saved_model(ckpt, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    assert extra["camera_bounds"] == data.camera_bounds
    a = model.render(poses[0], data.camera_intrinsics, perturb_sampled_points=False).colour
    b = loaded.render(poses[0], data.camera_intrinsics, perturb_sampled_points=False).colour
    assert torch.equal(a, b)


@pytest.mark.parametrize("storage", ["reference", "split", "bricked"])
def test_occupancy_skipping_is_exact(hip_device, storage):
    """BASELINE.json configs[4] at reduced size: density-threshold occupancy mask, ReLU field, threshold 0:
    outputs AND gradients are bit-identical with and without the mask on a sparse scene."""
    G, S = 48, 96
    gd, gf = sparse_scene_grid((G, G, G), 27, 21)
    cam = hotdog_like_camera()
    pose = rf.pose_spherical(40.0, -25.0, cam["radius"])
    outs = []
    for use in (False, True):
        grid = relu_grid(hip_device, gd, gf, G, storage=storage)
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True, use_occupancy_mask=use)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(48, 48, 60.0), pose, hip_device))
        out = model.render_rays(rays)
        out.colour.sum().backward()
        rgd, rgf = grid.reference_gradients()
        outs.append((out.colour.detach(), out.depth.detach(), rgd.clone(), rgf.clone(), grid))
    occ = outs[1][4].occupancy
    bits = sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in occ.cpu().tolist())
    assert 0 < bits < 0.5 * (G + 1) ** 3, "the mask should mark most of this scene empty"
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].min()) < 0.9  # something is visible
    # float32 atomics are order-dependent, so gradients are compared to rounding, not bitwise
    for a, b in ((outs[0][2], outs[1][2]), (outs[0][3], outs[1][3])):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-6 * float(a.abs().max()))


# ----------------------------------------------------------------------------------------
# BASELINE.json full size: 128^3 SH-2 grid, 800x800, 256 samples/ray -- size-independent properties
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_size(hip_device):
    cam = hotdog_like_camera()
    gen = torch.Generator(device=hip_device)
    gen.manual_seed(42)
    dens = torch.empty((128, 128, 128, 1), device=hip_device).uniform_(-1, 1, generator=gen)
    feat = torch.empty((128, 128, 128, 27), device=hip_device).uniform_(-1, 1, generator=gen)
    grid = relu_grid(hip_device, dens, feat, 128)
    cfg = rf.SHVoxGridRenderConfig(256, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    pose = rf.pose_spherical(30.0, -30.0, cam["radius"])
    return model, pose, rf.CameraIntrinsics(800, 800, 1111.111), cam


def test_full_size_chunking_permutation_and_background_properties(full_size, hip_device, monkeypatch):
    model, pose, intr, cam = full_size
    whole = model.render(pose, intr, parallel_rays_chunk_size=None)
    chunked = model.render(pose, intr, parallel_rays_chunk_size=32768)
    ragged = model.render(pose, intr, parallel_rays_chunk_size=50001)
    for other in (chunked, ragged):  # rays are independent: any chunking is bit-identical
        assert torch.equal(whole.colour, other.colour) and torch.equal(whole.depth, other.depth)
    assert whole.colour.shape == (800, 800, 3)
    rays = rf.flatten_rays(rf.cast_rays(intr, pose, hip_device))
    perm = torch.randperm(len(rays), device=hip_device)[:100000]
    sub = model.render_rays(rays[perm])
    # any ray order gives the same per-ray result: bit for bit on the per-ray kernel, to summation order against the frame's ray packets
    assert float((sub.colour - whole.colour.reshape(-1, 3)[perm]).abs().max()) <= 2e-6
    monkeypatch.setenv("RF_FRAME_TILES", "0")
    per_ray_frame = model.render(pose, intr, parallel_rays_chunk_size=None)
    monkeypatch.undo()  # (whatever the variable was before the test, it is that again)
    assert torch.equal(sub.colour, per_ray_frame.colour.reshape(-1, 3)[perm])
    # the packet kernel's own self-consistency on the default path: the same pixels through other cuts of the frame (first_ray / num_rays
    # that start inside a pixel row and inside a tile row) are the same bits -- a pixel does not depend on its tile-mates
    import dataclasses

    cfg = dataclasses.replace(model.render_config, perturb_sampled_points=True)  # (keyed jitter: indexed by the pixel, not by the call)
    torch.manual_seed(77)
    ref = rf.render_sh_voxel_grid_frame(model.thre3d_repr, intr, pose, cfg)
    for first, count in ((800 * 3 + 5, 123457), (800 * 397 + 399, 800 * 11 + 3), (800 * 800 - 1, 1)):
        torch.manual_seed(77)
        part = rf.render_sh_voxel_grid_frame(model.thre3d_repr, intr, pose, cfg, first_ray=first, num_rays=count)
        assert torch.equal(part.colour, ref.colour[first : first + count]) and torch.equal(part.depth, ref.depth[first : first + count])
    black = model.render(pose, intr, parallel_rays_chunk_size=None, white_bkgd=False)
    acc = whole.extra["accumulated_weight"]
    assert torch.equal(acc, black.extra["accumulated_weight"]) and torch.equal(whole.depth, black.depth)
    np.testing.assert_allclose((whole.colour - black.colour).cpu().numpy(), (1.0 - acc).expand(-1, -1, 3).cpu().numpy(), atol=2e-7)
    assert float(acc.max()) <= 1.0 + 1e-6 and float(acc.min()) >= 0.0
    # compositing weights are a partition: 0 <= depth <= far * acc
    assert bool((whole.depth <= cam["far"] * acc + 1e-5).all())
    # features do not influence geometry
    f = model.thre3d_repr.features
    saved = f.detach().clone()
    with torch.no_grad():
        f.mul_(-0.5)
    other = model.render(pose, intr, parallel_rays_chunk_size=None)
    with torch.no_grad():
        f.copy_(saved)
    assert torch.equal(other.depth, whole.depth) and torch.equal(other.extra["accumulated_weight"], acc)
    assert not torch.equal(other.colour, whole.colour)


def test_full_size_spot_check_against_oracle(full_size, hip_device):
    """2048 random rays of the full-size frame (and their gradients) against the oracle on the same grid."""
    model, pose, intr, cam = full_size
    grid = model.thre3d_repr
    rays = rf.flatten_rays(rf.cast_rays(intr, pose, hip_device))
    idx = torch.from_numpy(np.random.RandomState(1).choice(len(rays), 2048, replace=False)).to(hip_device)
    sub = rays[idx]
    target = T(hash_uniform((2048, 3), 9, 0.0, 1.0)).to(hip_device)
    grid.zero_grad()
    out = model.render_rays(sub)
    torch.nn.functional.l1_loss(out.colour, target).backward()
    cd = grid.densities.detach().cpu().clone().requires_grad_(True)
    cf = grid.features.detach().cpu().clone().requires_grad_(True)
    ref = orc.render(cd, cf, sub.origins.cpu(), sub.directions.cpu(), orc.make_aabb((128,) * 3, (3.0 / 128,) * 3), cam["near"], cam["far"], 256,
                     100.0 / 3.0, "relu", white_bkgd=True, interp="aten")
    torch.nn.functional.l1_loss(ref["colour"], target.cpu()).backward()
    np.testing.assert_allclose(out.colour.detach().cpu().numpy(), ref["colour"].detach().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(out.extra["accumulated_weight"].detach().cpu().numpy(), ref["acc"].detach().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(out.depth.detach().cpu().numpy(), ref["depth"].detach().numpy(), rtol=0, atol=6e-5)  # H1: fp32 depth noise
    gd, gf = grid.densities.grad.cpu().numpy(), grid.features.grad.cpu().numpy()
    np.testing.assert_allclose(gd, cd.grad.numpy(), rtol=1e-3, atol=1e-5 * np.abs(cd.grad.numpy()).max())
    np.testing.assert_allclose(gf, cf.grad.numpy(), rtol=1e-3, atol=1e-5 * np.abs(cf.grad.numpy()).max())
    grid.zero_grad()


def test_backward_run_to_run_differences_are_rounding_only(full_size, hip_device):
    """H5: float32 atomics make gradients non-bitwise run to run; two runs must agree to rounding."""
    model, pose, intr, cam = full_size
    grid = model.thre3d_repr
    rays = rf.flatten_rays(rf.cast_rays(intr, pose, hip_device))[:8192]
    grads = []
    for _ in range(2):
        grid.zero_grad()
        model.render_rays(rays).colour.square().sum().backward()
        grads.append(grid.features.grad.clone())
    scale = float(grads[0].abs().max())
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-5 * scale
    grid.zero_grad()


def test_keyed_ray_selection(hip_device):
    """rf_select_rays_and_pixels: distinct pixels (a permutation prefix), the same indices as the numpy
    restatement of the keyed bijection, rays identical to cast_rays at those pixels, pixels from the table,
    and a uniform spread over images / image regions."""
    data, cfg, poses = _make_scene(hip_device, 12, 0, 6, 40, 16)
    hw, H, W, f = 1600, 40, 40, data.camera_intrinsics.focal
    ids = torch.tensor([4, 0, 5, 2])
    key = 0x0123456789ABCDEF
    o, d, px, idx = ops.select_rays_and_pixels_hip(H, W, f, data.poses, ids, data.pixels, 3000, key, return_index=True)
    idx_cpu = idx.cpu().numpy()
    assert len(np.unique(idx_cpu)) == 3000 and idx_cpu.min() >= 0 and idx_cpu.max() < 4 * hw
    np.testing.assert_array_equal(idx_cpu, orc.keyed_permutation(np.arange(3000), 4 * hw, key))
    full = ops.select_rays_and_pixels_hip(H, W, f, data.poses, ids, data.pixels, 4 * hw, key, return_index=True)[3]
    assert sorted(full.cpu().tolist()) == list(range(4 * hw))  # a bijection of the whole pixel range
    # rays / pixels of the chosen entries
    b = idx // hw
    rem = idx - b * hw
    img = ids.to(hip_device)[b]
    ro, rd = ops.cast_selected_rays_hip(H, W, f, data.poses[ids.to(hip_device)], idx)
    assert torch.equal(o, ro) and torch.equal(d, rd)
    assert torch.equal(px, data.pixels[img * hw + rem])
    # uniformity: image counts and 4x4 tile counts of a larger draw (chi-square, loose bound)
    big = ops.select_rays_and_pixels_hip(H, W, f, data.poses, ids, data.pixels, 4800, 987654321, return_index=True)[3].cpu().numpy()
    counts = np.bincount(big // hw, minlength=4)
    assert np.all(np.abs(counts - 1200) < 5 * np.sqrt(1200 * 0.75))
    rem = big % hw
    tiles = np.bincount((rem // W // 10) * 4 + (rem % W) // 10, minlength=16)
    assert np.all(np.abs(tiles - 300) < 5 * np.sqrt(300))
    # different keys give different batches; the trainer draws its key from torch's CPU generator
    other = ops.select_rays_and_pixels_hip(H, W, f, data.poses, ids, data.pixels, 3000, key + 1, return_index=True)[3]
    assert not torch.equal(other, idx)
    d0, f0 = procedural_grid((12, 12, 12), 3, 5)
    model = rf.VolumetricModel(relu_grid(hip_device, d0, f0, 12), rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, 512, 0.03, ray_selection="keyed")
    torch.manual_seed(3)
    r1, p1 = stepper.select(data, ids)
    torch.manual_seed(3)
    r2, p2 = stepper.select(data, ids)
    assert torch.equal(r1.origins, r2.origins) and torch.equal(p1, p2) and len(r1) == 512
    # "randperm_blocks": ONE torch.randperm per block of floor(P / R) iterations, consumed in consecutive slices: the batches of a
    # block are disjoint slices of that permutation (rays / pixels of exactly those entries), the block after it draws a new one
    stepper = TrainStepper(model, 1500, 0.03, ray_selection="randperm_blocks")
    torch.manual_seed(5)
    expect = torch.randperm(4 * hw, dtype=torch.long, device=hip_device)
    torch.manual_seed(5)
    seen = []
    for k in range(4):  # 4 x 1500 = 6000 of the 6400 pixels: one block
        r, p = stepper.select(data, ids)
        sel = expect[1500 * k : 1500 * (k + 1)]
        ro, rd = ops.cast_selected_rays_hip(H, W, f, data.poses[ids.to(hip_device)], sel)
        assert torch.equal(r.origins, ro) and torch.equal(r.directions, rd)
        assert torch.equal(p, data.pixels[ids.to(hip_device)[sel // hw] * hw + sel % hw])
        seen.append(sel)
    assert len(torch.unique(torch.cat(seen))) == 6000
    r, _ = stepper.select(data, ids)  # 400 entries are left: a new permutation
    assert stepper._perm_block[1] == 1500 and len(r) == 1500


def _binned_gradients(grid, rays, cfg, target, device, diffuse_too=True, accumulate=False, binning="sort", brick=8):
    """(dL/d first, dL/d second) of L1(spec) [+ L1(diffuse)] through the emit -> sort -> brick-accumulate path"""
    from thr3ed_atom_amd import ops as O

    o, d = rays.origins.contiguous(), rays.directions.contiguous()
    n, S = o.shape[0], cfg.num_samples_per_ray
    near, far = float(np.float32(cfg.camera_bounds.near)), float(np.float32(cfg.camera_bounds.far))
    nb = O.brick_counts(grid, brick)
    num_bricks = nb[0] * nb[1] * nb[2]
    boundaries = torch.arange(num_bricks * 8, dtype=torch.int16, device=device)
    first, second = grid.kernel_tensors()
    # accumulate=False overwrites every element (no zero-fill needed): start from garbage to prove it
    gd = torch.full_like(first, 7.0) if not accumulate else torch.zeros_like(first)
    gf = None if second is None else (torch.full_like(second, -3.0) if not accumulate else torch.zeros_like(second))
    sums = torch.zeros(4, device=device)
    lists, keep = [], []
    merged = binning == "merged"  # fused counting for both lists, then ONE brick pass over (specular, diffuse)
    if merged:
        binning = "fused"
    for i, diffuse in enumerate((False, True) if diffuse_too else (False,)):
        flags = O.render_flags(cfg.white_bkgd, diffuse or cfg.render_diffuse, cfg.optimized_sampling, False)
        is_diffuse = diffuse or cfg.render_diffuse
        hist = torch.zeros(num_bricks * 8, dtype=torch.int32, device=device) if binning in ("count", "fused") else None
        colour, _, _, _, caches = O.render_forward_raw(grid, o, d, None, S, near, far, flags, save=True, key_hist=hist if binning == "fused" else None, brick_size=brick)
        g_colour = O.l1_loss_grad_hip(colour, target, sums[2 * i : 2 * i + 2])
        keys = torch.empty(n * S, dtype=torch.int16, device=device)
        rec = torch.empty((n * S, O.expanded_record_floats(grid, is_diffuse)), device=device)
        srt = torch.empty((n * S, O.expanded_record_floats(grid, is_diffuse)), device=device)
        offsets = torch.full((num_bricks * 8 + 1,), n * S, dtype=torch.int64, device=device)
        cursor = torch.empty(num_bricks * 8, dtype=torch.int32, device=device)
        if binning == "fused":  # the forward pass counted; the backward pass writes expanded records at their final positions
            counted = int(hist.sum())
            assert counted == int(np.unpackbits(caches[3].cpu().numpy().view(np.uint8)).sum())  # one mask bit per counted (= cached) sample
            O.bin_offsets(hist, offsets, cursor)
            O.render_backward_emit_direct_raw(grid, o, d, None, S, near, far, flags, caches, g_colour, None, None, brick, cursor, srt, hist_clear=hist)
            assert int(hist.abs().sum()) == 0 and int(offsets[-1]) == counted
            assert torch.equal(cursor.to(torch.int64), offsets[1:])  # every class filled exactly
        else:
            O.render_backward_emit_raw(grid, o, d, None, S, near, far, flags, caches, g_colour, None, None, brick, keys, rec, hist)
            if binning == "count":
                O.bin_records_by_brick(grid, keys, rec, is_diffuse, hist, cursor, srt, offsets)
                assert int(hist.abs().sum()) == 0 and int(offsets[-1]) == int((keys >= 0).sum())
            else:
                O.sort_records_by_brick(grid, keys, rec, is_diffuse, srt, offsets, boundaries)
        lists.append((srt, offsets, diffuse or cfg.render_diffuse))
        keep.append((keys, rec, caches))
    if merged:
        O.brick_accumulate_raw(grid, brick, lists, gd, gf, accumulate=accumulate)
        if accumulate:
            O.brick_accumulate_raw(grid, brick, lists, gd, gf, accumulate=True)
            gd.mul_(0.5)
            if gf is not None:
                gf.mul_(0.5)
        return gd, gf
    # the specular list first (it writes every channel), the diffuse list (base channels only) on top
    for k, one in enumerate(lists):
        O.brick_accumulate_raw(grid, brick, [one], gd, gf, accumulate=accumulate or k > 0)
    if accumulate:  # adding the same lists once more doubles the result
        for one in lists:
            O.brick_accumulate_raw(grid, brick, [one], gd, gf, accumulate=True)
        gd.mul_(0.5)
        if gf is not None:
            gf.mul_(0.5)
    return gd, gf


@pytest.mark.parametrize("accumulate,binning", [(False, "sort"), (True, "sort"), (False, "count"), (False, "fused"), (False, "merged"), (True, "merged")])
@pytest.mark.parametrize("storage", ["reference", "split", "bricked"])
@pytest.mark.parametrize("case", ["grid16_sh2", "aniso_sh2_abs", "aniso_sh1_softplus", "cube20_sh0", "aniso_sh3", "aniso_sh2_identity"])
def test_binned_backward_equals_atomic_backward(hip_device, storage, case, accumulate, binning):
    """The LDS-aggregated backward (emit -> 16-bit sort by (brick, flags) -> one workgroup per 8^3-node brick that owns
    its nodes exclusively -> plain coalesced stores) gives the gradient of the atomic scatter (and therefore of the reference)
    for specular + diffuse renders, including partial bricks, the grid border, SH degree 0-3 (degree 3 = four 16-channel
    accumulator blocks per tile) and the abs / softplus / identity density modes (identity: signed densities, negative occupancies and
    transmittances above 1 -- both adjoints share the occupancy helper, so this is a consistency check; the oracle checks are in
    tests/test_hip_parity.py)."""
    from thr3ed_atom_amd.voxels import unpack_split

    cam = hotdog_like_camera()
    g7 = load_golden("g7_grid16_render.npz")
    rays = rf.Rays(T(g7["origins"]).to(hip_device), T(g7["directions"]).to(hip_device))
    target = T(g7["target"]).to(hip_device)
    dims, F, mode, voxel, loc, rho = {
        "grid16_sh2": ((16, 16, 16), 27, "relu", (3.0 / 16,) * 3, (0.0, 0.0, 0.0), 100.0 / 3.0),
        "aniso_sh2_abs": ((13, 9, 18), 27, "abs", (0.22, 0.3, 0.16), (0.1, -0.05, 0.1), 1.0),
        "aniso_sh1_softplus": ((9, 17, 8), 12, "softplus", (0.3, 0.17, 0.35), (0.0, 0.0, 0.0), 5.0),
        "cube20_sh0": ((20, 20, 20), 3, "relu", (0.15,) * 3, (0.0, 0.0, 0.0), 100.0 / 3.0),
        "aniso_sh3": ((11, 17, 9), 48, "relu", (0.27, 0.17, 0.3), (0.0, 0.05, 0.0), 20.0),
        "aniso_sh2_identity": ((13, 9, 18), 27, "identity", (0.22, 0.3, 0.16), (0.1, -0.05, 0.1), 5.0),
    }[case]
    acts = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()), "abs": (torch.abs, torch.nn.Identity()),
            "identity": (torch.nn.Identity(), torch.nn.Identity())}[mode]
    dens, feat = signed_density_grid(dims, F, 303) if mode == "identity" else procedural_grid(dims, F, 303)
    if mode == "identity":  # the regime is covered (sigma delta <= -0.5), and no ray's 1e10-long last interval has a negative density
        r64 = orc.render(dens.double(), feat.double(), T(g7["origins"]).double(), T(g7["directions"]).double(), orc.make_aabb(dims, voxel, loc), cam["near"],
                         cam["far"], 40, rho, mode, white_bkgd=True)
        xmin, _, usable = identity_regime(r64["processed"], r64["deltas"])
        assert float(xmin.min()) <= -0.5 and bool(usable.all())
    grid = rf.VoxelGrid(dens.to(hip_device), feat.to(hip_device), rf.VoxelSize(*voxel), rf.VoxelGridLocation(*loc), density_preactivation=acts[0],
                        density_postactivation=acts[1], expected_density_scale=rho, tunable=True, storage=storage)
    cfg = rf.SHVoxGridRenderConfig(40, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    loss = torch.nn.functional.l1_loss(model.render_rays(rays).colour, target)
    loss = loss + torch.nn.functional.l1_loss(model.render_rays(rays, render_diffuse=True).colour, target)
    loss.backward()
    ref_d, ref_f = grid.reference_gradients()
    gd, gf = _binned_gradients(grid, rays, cfg, target, hip_device, accumulate=accumulate, binning=binning)
    gd, gf = grid.unpack(gd, gf)
    assert float(ref_d.abs().max()) > 0 and float(ref_f.abs().max()) > 0
    np.testing.assert_allclose(gd.cpu().numpy(), ref_d.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(ref_d.abs().max()))
    np.testing.assert_allclose(gf.cpu().numpy(), ref_f.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(ref_f.abs().max()))


def test_binned_train_step_follows_reference_trajectory(hip_device):
    g = load_golden("g9_trainer_trajectory.npz")
    G, deg, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F = 3 * (deg + 1) ** 2
    grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage="split")
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]), backward="binned")
    for it in range(steps):
        rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
        stats = stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
        np.testing.assert_allclose(stats.specular_loss.item(), g["specular_loss"][it], rtol=1e-5)
        np.testing.assert_allclose(stats.diffuse_loss.item(), g["diffuse_loss"][it], rtol=1e-5)
    dd = np.abs(grid.densities.detach().cpu().numpy() - g["dens_final"])
    df = np.abs(grid.features.detach().cpu().numpy() - g["feat_final"])
    assert np.mean(dd < 1e-4) > 0.99 and np.mean(df < 1e-4) > 0.99


def test_data_parallel_overlap_wiring(hip_device, monkeypatch):
    """The data-parallel train step reduces the `rest` gradients right after the specular backward (so that the
    collective overlaps the diffuse pass, which only touches `base`) and `base` after the diffuse backward.  With a
    stand-in collective that is the identity (what averaging identical replicas does) the step must equal the
    single-process step; the recorded calls show order and sizes.  (Real RCCL runs are the driver's 2/4/8-GPU bench.)"""
    from thr3ed_atom_amd import distributed as rfdist

    g = load_golden("g9_trainer_trajectory.npz")
    G, deg, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F = 3 * (deg + 1) ** 2
    calls = []

    class Handle:
        def wait(self):
            calls.append("wait")

    def fake_async(bucket):
        calls.append(("async", bucket.numel(), bucket.data_ptr()))
        return Handle()

    results = []
    for dp in (False, True):
        grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage="split")
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]), shard_optimizer=False)
        if dp:
            monkeypatch.setattr(rfdist, "world_size", lambda: 2)
            monkeypatch.setattr(rfdist, "_collectives_on", lambda: True)
            monkeypatch.setattr(rfdist, "all_reduce_mean_async", fake_async)
        for it in range(2):
            rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
            stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
        results.append((grid.densities.detach().clone(), grid.features.detach().clone(), stepper))
    monkeypatch.undo()
    assert torch.allclose(results[0][0], results[1][0], atol=1e-6) and torch.allclose(results[0][1], results[1][1], atol=1e-6)
    flat = results[1][2].flat
    first, second = flat.flat_gradient_parts()
    per_step = [("async", second.numel(), second.data_ptr()), ("async", first.numel(), first.data_ptr()), "wait", "wait"]
    assert calls == per_step * 2
    assert first.numel() == G**3 * 4 and second.numel() == G**3 * (F - 3)


def test_data_parallel_sharded_optimizer_wiring(hip_device, monkeypatch):
    """Default data-parallel step (ZeRO stage 1): `rest` is reduce-scattered right after the specular backward, `base`
    after the diffuse backward, Adam runs on this rank's chunk of each only, and the updated chunks are all-gathered.
    With stand-in collectives for rank 0 of 2 (identity reduce = averaging identical replicas; all-gather delivers
    nothing) the own chunks must equal the single-process step and the other chunks must still hold their old values."""
    from thr3ed_atom_amd import distributed as rfdist

    g = load_golden("g9_trainer_trajectory.npz")
    G, deg, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F = 3 * (deg + 1) ** 2
    calls = []

    class Handle:
        def __init__(self, bucket):
            self.lo, self.hi = 0, bucket.numel() // 2
            self.shard = bucket[: self.hi]

        def wait(self):
            calls.append("wait")

    def fake_reduce_scatter(bucket):
        calls.append(("reduce_scatter", bucket.numel()))
        return Handle(bucket)

    def fake_all_gather(bucket):
        calls.append(("all_gather", bucket.numel()))
        return bucket

    out = []
    for dp in (False, True):
        grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage="split")
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]))
        before = stepper.flat.flat_param.clone()
        if dp:
            monkeypatch.setattr(rfdist, "world_size", lambda: 2)
            monkeypatch.setattr(rfdist, "_collectives_on", lambda: True)
            monkeypatch.setattr(rfdist, "reduce_scatter_mean_async", fake_reduce_scatter)
            monkeypatch.setattr(rfdist, "all_gather_chunks_", fake_all_gather)
        rays = rf.Rays(T(g["origins"][0]).to(hip_device), T(g["directions"][0]).to(hip_device))
        stepper.step_on(rays, T(g["pixels"][0]).to(hip_device))
        out.append((before, stepper.flat.flat_param.clone()))
    monkeypatch.undo()
    (before, full), (_, mine) = out
    nd, nr = G**3 * 4, G**3 * (F - 3)
    own = torch.zeros(nd + nr, dtype=torch.bool, device=full.device)
    own[: nd // 2] = True
    own[nd : nd + nr // 2] = True
    assert float((full - before).abs().max()) > 0
    assert torch.allclose(mine[own], full[own], atol=1e-6) and torch.equal(mine[~own], before[~own])
    assert calls == [("reduce_scatter", nr), ("reduce_scatter", nd), "wait", "wait", ("all_gather", nr), ("all_gather", nd)]


@pytest.mark.parametrize("exchange,shard_optimizer", [("owner", True), ("dense", True), ("dense", False)])
def test_data_parallel_step_through_rccl_single_rank(hip_device, monkeypatch, exchange, shard_optimizer):
    """The data-parallel train step with its collectives really going through RCCL (a process group of ONE rank on this
    GPU: owner-computes = all_gather_into_tensor of the offset tables on RCCL's stream + the side-stream host read + all_to_all +
    the brick pass over a brick range; dense = reduce_scatter_tensor / all_gather_into_tensor / asynchronous all_reduce with
    ReduceOp.AVG) must equal the plain step.  (Multi-rank semantics are covered by the gloo tests; 2/4/8-GPU runs are the driver's.)"""
    import torch.distributed as dist
    from thr3ed_atom_amd import distributed as rfdist

    g = load_golden("g9_trainer_trajectory.npz")
    G, deg, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    if exchange == "owner":
        deg = 2  # (the trajectory's grid is SH degree 1; the optimizer in the brick flush needs whole float4s per node: degree 0 or 2)
    F = 3 * (deg + 1) ** 2
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    monkeypatch.setenv("RF_OWNER_FORCE_COLLECTIVES", "1")  # (a 1-rank group: run the exchange and all-gather calls anyway)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group(backend="nccl", rank=0, world_size=1)
    try:
        out = []
        for dp in (False, True):
            rfdist.FORCE_COLLECTIVES = dp
            grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage="split")
            cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
            model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
            # (dense: the deterministic binned adjoint on both sides -- a fixed summation order -- so that the comparison is tight)
            stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]), shard_optimizer=shard_optimizer, exchange=exchange if dp else "auto",
                                   backward="binned", deterministic=exchange == "dense")
            assert stepper.exchange == (exchange if dp else "dense")
            for it in range(2):
                rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
                stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
            out.append(stepper.flat.flat_param.clone())
        torch.cuda.synchronize()
        # (the record order inside a key class depends on atomic timing, so the two runs sum in different orders: parameters whose
        # gradient is ~1e-8 amplify that through Adam's first steps -- same criterion as the trajectory tests)
        err = (out[0] - out[1]).abs()
        if exchange == "dense":  # same kernels, same record order, same Adam arithmetic: the collectives must not change a bit that matters
            assert float(err.max()) <= 1e-6, float(err.max())
        else:
            assert float((err <= 2e-5).float().mean()) >= 0.999 and float(err.max()) <= float(g["lr"]) * 2 * 2 + 1e-6
    finally:
        rfdist.FORCE_COLLECTIVES = False
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("selection", ["keyed", "randperm"])
def test_global_batch_slices_reproduce_the_single_gpu_step(hip_device, monkeypatch, selection):
    """Strong scaling: with ``global_batch=True`` the ranks draw the SAME keyed permutation and take disjoint
    contiguous slices of it; the average of their gradient buckets is the single-GPU gradient.  Two ranks are played
    one after the other on this GPU (stand-in rank / world size, collectives off)."""
    from thr3ed_atom_amd import distributed as rfdist

    G, deg, S, R = 16, 2, 32, 512
    F = 3 * (deg + 1) ** 2
    cam = hotdog_like_camera()
    images = T(hash_uniform((4, 3, 24, 24), 77, 0.0, 1.0)).to(hip_device)
    cams = [rf.pose_spherical(40.0 * k, -30.0, cam["radius"]) for k in range(4)]
    poses = torch.stack([torch.cat([c.rotation, c.translation.reshape(3, 1)], dim=1) for c in cams]).to(hip_device)
    data = PosedImagesInMemory(images, poses, rf.CameraIntrinsics(24, 24, 33.0), rf.CameraBounds(cam["near"], cam["far"]))

    def run(rank, world):
        grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage="split")
        cfg = rf.SHVoxGridRenderConfig(S, data.camera_bounds, perturb_sampled_points=False, white_bkgd=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, R, learning_rate=0.03, global_batch=True, ray_selection=selection, fuse_optimizer=False)  # (the gradient bucket is what the ranks would exchange)
        monkeypatch.setattr(rfdist, "world_size", lambda: world)
        monkeypatch.setattr(rfdist, "rank", lambda: rank)
        monkeypatch.setattr(rfdist, "_collectives_on", lambda: False)
        torch.manual_seed(5)  # the same CPU generator state on every "rank"
        rays, pixels = stepper.select(data, torch.arange(4))
        stepper.step_on(rays, pixels)
        monkeypatch.undo()
        return rays.origins.clone(), rays.directions.clone(), pixels.clone(), stepper.flat.flat_grad.clone()

    o, d, px, g_full = run(0, 1)
    parts = [run(r, 2) for r in range(2)]
    assert all(p[0].shape[0] == R // 2 for p in parts)
    assert torch.equal(torch.cat([p[0] for p in parts]), o) and torch.equal(torch.cat([p[1] for p in parts]), d)
    assert torch.equal(torch.cat([p[2] for p in parts]), px)
    g_avg = 0.5 * (parts[0][3] + parts[1][3])
    assert float(g_full.abs().max()) > 0
    np.testing.assert_allclose(g_avg.cpu().numpy(), g_full.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(g_full.abs().max()))


def test_deterministic_binned_step_is_bit_reproducible(hip_device):
    """``deterministic=True`` sends both passes through the bricks with the stable radix sort: no float atomics anywhere,
    so two runs of the same training iterations give bit-identical gradients and parameters (the atomic scatter and the
    counting sort's atomic cursors do not promise that)."""
    g = load_golden("g9_trainer_trajectory.npz")
    G, deg, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F = 3 * (deg + 1) ** 2
    runs = []
    for _ in range(2):
        grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage="split")
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]), backward="binned", deterministic=True)
        grads = []
        for it in range(3):
            rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
            stats = stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
            grads.append(stepper.flat.flat_grad.clone())
            np.testing.assert_allclose(stats.specular_loss.item(), g["specular_loss"][it], rtol=1e-5)
        runs.append((grads, stepper.flat.flat_param.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1])


def test_binned_backward_with_mostly_empty_bricks(hip_device):
    """A handful of rays on a 40^3 grid (125 bricks, most of them untouched): the overwrite mode must leave exact zeros
    in every empty brick and the atomic path's gradient elsewhere, starting from garbage."""
    from thr3ed_atom_amd import ops as O

    G, F, S = 40, 27, 48
    cam = hotdog_like_camera()
    grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 31)), T(hash_uniform((G, G, G, F), 32)), G, storage="split")
    pose = rf.pose_spherical(30.0, -30.0, cam["radius"])
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(3, 3, 40.0), pose, hip_device))  # 9 rays through the centre
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    target = T(hash_uniform((len(rays), 3), 5, 0.0, 1.0)).to(hip_device)
    out = rf.render_sh_voxel_grid(grid, rays, cfg)
    torch.nn.functional.l1_loss(out.colour, target).backward()
    ref_d, ref_f = grid.reference_gradients()
    gd, gf = _binned_gradients(grid, rays, cfg, target, hip_device, diffuse_too=False, binning="fused")
    gd, gf = grid.unpack(gd, gf)
    assert float((ref_f == 0).float().mean()) > 0.9  # most of the grid is untouched
    np.testing.assert_allclose(gd.cpu().numpy(), ref_d.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(ref_d.abs().max()))
    np.testing.assert_allclose(gf.cpu().numpy(), ref_f.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(ref_f.abs().max()))
    assert torch.equal(gf == 0, ref_f == 0) or float(((gf == 0) != (ref_f == 0)).float().mean()) < 1e-3


@pytest.mark.parametrize("binning", ["fused", "count", "sort", "merged"])
@pytest.mark.parametrize("seed", list(range(8)))
def test_binned_backward_randomised_shapes(hip_device, seed, binning):
    """Binned backward (each binning path) == atomic backward on randomly drawn grid sizes (partial bricks), ray counts (not multiples
    of the wave count), sample counts, SH degrees, density modes, storages and brick sizes."""
    from thr3ed_atom_amd import ops as O

    rng = np.random.RandomState(100 + seed)
    dims = tuple(int(v) for v in rng.randint(5, 30, size=3))
    deg = int(rng.randint(0, 3))
    F = 3 * (deg + 1) ** 2
    S = int(rng.choice([17, 33, 64, 70]))
    n_rays = int(rng.choice([1, 3, 37, 130]))
    mode = ["relu", "softplus", "abs"][int(rng.randint(0, 3))]
    storage = ["reference", "split", "bricked"][int(rng.randint(0, 3))]
    acts = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()), "abs": (torch.abs, torch.nn.Identity())}[mode]
    cam = hotdog_like_camera()
    voxel = tuple(3.0 / d for d in dims)
    grid = rf.VoxelGrid(T(hash_uniform((*dims, 1), 300 + seed)).to(hip_device), T(hash_uniform((*dims, F), 400 + seed)).to(hip_device), rf.VoxelSize(*voxel),
                        density_preactivation=acts[0], density_postactivation=acts[1], expected_density_scale=5.0 if mode != "abs" else 1.0,
                        tunable=True, storage=storage)
    pose = rf.pose_spherical(float(rng.uniform(0, 360)), float(rng.uniform(-60, -10)), cam["radius"])
    side = int(np.ceil(np.sqrt(n_rays)))
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(side, side, 0.9 * side), pose, hip_device))[:n_rays]
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=bool(seed & 1))
    target = T(hash_uniform((n_rays, 3), 5 + seed, 0.0, 1.0)).to(hip_device)
    spec = rf.render_sh_voxel_grid(grid, rays, cfg)
    diff = rf.render_sh_voxel_grid(grid, rays, rf.SHVoxGridRenderConfig(S, cfg.camera_bounds, perturb_sampled_points=False, white_bkgd=cfg.white_bkgd, render_diffuse=True))
    (torch.nn.functional.l1_loss(spec.colour, target) + torch.nn.functional.l1_loss(diff.colour, target)).backward()
    ref_d, ref_f = grid.reference_gradients()
    gd, gf = _binned_gradients(grid, rays, cfg, target, hip_device, binning=binning, brick=8 if seed & 2 else 4)
    gd, gf = grid.unpack(gd, gf)
    np.testing.assert_allclose(gd.cpu().numpy(), ref_d.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(ref_d.abs().max()) + 1e-12)
    np.testing.assert_allclose(gf.cpu().numpy(), ref_f.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(ref_f.abs().max()) + 1e-12)


@pytest.mark.parametrize("n_rays,storage", [(37, "split"), (130, "bricked"), (1, "split")])
def test_binned_and_atomic_train_steps_agree_for_odd_batches(hip_device, n_rays, storage):
    """Several fused training iterations with jitter on ray batches that fill neither a workgroup nor a wavefront quad:
    the binned step (forward-side counting, direct emit, bricks) must track the atomic step -- this is the trainer-level
    guard for stale per-key counters or cursors between iterations."""
    G, deg, S = 24, 2, 40
    F = 3 * (deg + 1) ** 2
    cam = hotdog_like_camera()
    pose = rf.pose_spherical(50.0, -35.0, cam["radius"])
    side = int(np.ceil(np.sqrt(n_rays)))
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(side, side, 0.9 * side), pose, hip_device))[:n_rays]
    target = T(hash_uniform((n_rays, 3), 9, 0.0, 1.0)).to(hip_device)
    finals = []
    for backward in ("atomic", "binned"):
        grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage=storage)
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, n_rays, learning_rate=0.01, backward=backward)
        torch.manual_seed(77)  # same jitter in both runs
        for _ in range(4):
            stepper.step_on(rays, target)
        finals.append(torch.cat([t.detach().reshape(-1) for t in grid.unpack(*grid.kernel_tensors())]))
    # Adam normalises the step, so summation-order noise on tiny gradients shows up at the 1e-3 * lr level at worst
    assert float((finals[0] - finals[1]).abs().max()) < 2e-3 and float((finals[0] - finals[1]).abs().mean()) < 1e-6


def test_fused_binning_beyond_4096_bricks(hip_device):
    """The fused binning has no 16-bit key arrays, so it also serves grids of more than 4096 bricks (here 136^3 nodes =
    17^3 = 4913 bricks); the per-slot-key variants refuse such a grid instead of wrapping their keys."""
    from thr3ed_atom_amd import ops as O

    G, S = 136, 64
    cam = hotdog_like_camera()
    grid = rf.VoxelGrid(T(hash_uniform((G, G, G, 1), 41)).to(hip_device), T(hash_uniform((G, G, G, 3), 42)).to(hip_device), rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G),
                        density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=20.0,
                        tunable=True, storage="split")
    pose = rf.pose_spherical(30.0, -30.0, cam["radius"])
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(12, 12, 16.0), pose, hip_device))
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    target = T(hash_uniform((len(rays), 3), 5, 0.0, 1.0)).to(hip_device)
    out = rf.render_sh_voxel_grid(grid, rays, cfg)
    torch.nn.functional.l1_loss(out.colour, target).backward()
    ref_d, ref_f = grid.reference_gradients()
    gd, gf = _binned_gradients(grid, rays, cfg, target, hip_device, diffuse_too=False, binning="fused")
    gd, gf = grid.unpack(gd, gf)
    assert float(ref_f.abs().max()) > 0
    np.testing.assert_allclose(gd.cpu().numpy(), ref_d.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(ref_d.abs().max()))
    np.testing.assert_allclose(gf.cpu().numpy(), ref_f.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(ref_f.abs().max()))
    with pytest.raises(RuntimeError, match="unsupported|not supported|UNSUPPORTED"):
        _binned_gradients(grid, rays, cfg, target, hip_device, diffuse_too=False, binning="sort")


def test_psnr_after_equal_steps_with_jitter_through_the_default_fused_path(hip_device):
    """north_star: PSNR within 0.05 dB of the reference after equal training steps -- here WITH stratified jitter and through
    the path the trainer and bench.py run by default (rf_train_step: merged brick pass, float64-atomic diffuse sums, Adam in
    the flush).  Both sides see the same ray batches and the same jitter tables (oracle.keyed_jitter, the numpy restatement
    of the in-kernel generator); the reference side is the oracle + torch.optim.Adam on the CPU."""
    G, deg, S, R, steps = 24, 2, 40, 768, 60
    data, cfg, poses = _make_scene(hip_device, G, deg, 8, 40, S)
    cfg.perturb_sampled_points = True
    F = 3 * (deg + 1) ** 2
    d0, f0 = procedural_grid((G, G, G), F, 78)
    grid = relu_grid(hip_device, d0, f0, G, storage="split")
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, R, learning_rate=0.03)
    assert stepper.merged_bricks and stepper.fuse_optimizer
    cd, cf = d0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    ref_opt = torch.optim.Adam([{"params": [cd, cf], "lr": 0.03}], betas=(0.9, 0.999))
    aabb = orc.make_aabb((G, G, G), (3.0 / G,) * 3)
    kw = dict(aabb=aabb, near=cfg.camera_bounds.near, far=cfg.camera_bounds.far, num_samples=S, density_scale=100.0 / 3.0, white_bkgd=True)
    torch.manual_seed(6)
    ids = torch.arange(7)  # view 7 is held out
    for it in range(steps):
        rays, pixels = stepper.select(data, ids)
        tables = [T(orc.keyed_jitter(1000 + 2 * it + i, 0, R, S)) for i in range(2)]
        stats = stepper.step_on(rays, pixels, t_rand=[t.to(hip_device) for t in tables])
        o, d, px = rays.origins.cpu(), rays.directions.cpu(), pixels.cpu()
        spec = torch.nn.functional.l1_loss(orc.render(cd, cf, origins=o, directions=d, t_rand=tables[0], **kw)["colour"], px)
        diff = torch.nn.functional.l1_loss(orc.render(cd, cf, origins=o, directions=d, render_diffuse=True, t_rand=tables[1], **kw)["colour"], px)
        ref_opt.zero_grad()
        (spec + diff).backward()
        ref_opt.step()
        np.testing.assert_allclose(stats.specular_loss.item(), spec.item(), rtol=1e-3)
    held = data.images[7].permute(1, 2, 0)
    ours = model.render(poses[7], data.camera_intrinsics, perturb_sampled_points=False).colour
    ho, hd = orc.cast_rays(40, 40, data.camera_intrinsics.focal, poses[7].rotation, poses[7].translation)
    ref = orc.render(cd.detach(), cf.detach(), origins=ho.reshape(-1, 3), directions=hd.reshape(-1, 3), **kw)["colour"].reshape(40, 40, 3)
    psnr_hip = float(rf.mse2psnr(torch.nn.functional.mse_loss(ours, held)))
    psnr_ref = float(rf.mse2psnr(torch.nn.functional.mse_loss(ref, held.cpu())))
    assert psnr_hip > 12.0  # it actually learned something (start is ~7 dB)
    assert abs(psnr_hip - psnr_ref) <= 0.05, (psnr_hip, psnr_ref)


@pytest.mark.parametrize("storage,deg", [("split", 2), ("bricked", 0), ("reference", 1)])
def test_binned_backward_with_records_concentrated_in_few_bricks(hip_device, storage, deg):
    """4096 rays of a narrow camera through the centre of a 24^3 grid, 256 samples each: tens of thousands of records land in a
    handful of bricks (dozens of 256-record batches per brick, tile lists hundreds of entries long -- the regime of a trained,
    sparse field), both renders in one brick pass.  Compared with the atomic adjoint of the autograd op."""
    G, S = 24, 256
    F = 3 * (deg + 1) ** 2
    cam = hotdog_like_camera()
    grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 41)) + 0.3, T(hash_uniform((G, G, G, F), 42)), G, rho=2.0, storage=storage)
    pose = rf.pose_spherical(40.0, -25.0, cam["radius"])
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(64, 64, 900.0), pose, hip_device))  # field of view ~4 degrees
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    target = T(hash_uniform((len(rays), 3), 6, 0.0, 1.0)).to(hip_device)
    total_d = total_f = None
    for diffuse in (False, True):
        cfg.render_diffuse = diffuse
        grid.zero_grad()
        out = rf.render_sh_voxel_grid(grid, rays, cfg)
        torch.nn.functional.l1_loss(out.colour, target).backward()
        ref_d, ref_f = grid.reference_gradients()
        total_d = ref_d.clone() if total_d is None else total_d + ref_d
        total_f = ref_f.clone() if total_f is None else total_f + ref_f
    cfg.render_diffuse = False
    assert float((total_f != 0).float().mean()) < 0.35  # the rays only see a thin tube of the volume
    gd, gf = _binned_gradients(grid, rays, cfg, target, hip_device, diffuse_too=True, binning="merged")
    gd, gf = grid.unpack(gd, gf)
    np.testing.assert_allclose(gd.cpu().numpy(), total_d.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(total_d.abs().max()))
    np.testing.assert_allclose(gf.cpu().numpy(), total_f.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(total_f.abs().max()))


@pytest.mark.parametrize("storage,deg", [("split", 2), ("reference", 1), ("bricked", 0)])
def test_brick_pass_over_two_lists_of_the_same_kind(hip_device, storage, deg):
    """rf_brick_accumulate with TWO full-width lists in one call (the ranges of both lists concatenated per brick) == the two
    lists accumulated one after the other == the atomic adjoint of both ray sets."""
    from thr3ed_atom_amd import ops as O

    G, S = 20, 48
    F = 3 * (deg + 1) ** 2
    cam = hotdog_like_camera()
    grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 61)), T(hash_uniform((G, G, G, F), 62)), G, storage=storage)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    first, second = grid.kernel_tensors()
    nb = O.brick_counts(grid, 8)
    nkeys = nb[0] * nb[1] * nb[2] * 8
    near, far = float(np.float32(cam["near"])), float(np.float32(cam["far"]))
    lists, total_d, total_f = [], None, None
    for k, (yaw, hw) in enumerate(((30.0, 24), (200.0, 31))):
        rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(hw, hw, 33.0), rf.pose_spherical(yaw, -30.0, cam["radius"]), hip_device))
        target = T(hash_uniform((len(rays), 3), 70 + k, 0.0, 1.0)).to(hip_device)
        grid.zero_grad()
        torch.nn.functional.l1_loss(rf.render_sh_voxel_grid(grid, rays, cfg).colour, target).backward()
        ref_d, ref_f = grid.reference_gradients()
        total_d = ref_d.clone() if total_d is None else total_d + ref_d
        total_f = ref_f.clone() if total_f is None else total_f + ref_f
        o, d, n = rays.origins.contiguous(), rays.directions.contiguous(), len(rays)
        flags = O.render_flags(True, False, False, False)
        hist = torch.zeros(nkeys, dtype=torch.int32, device=hip_device)
        colour, _, _, _, caches = O.render_forward_raw(grid, o, d, None, S, near, far, flags, save=True, key_hist=hist, brick_size=8)
        sums = torch.zeros(2, device=hip_device)
        g_colour = O.l1_loss_grad_hip(colour, target, sums)
        srt = torch.empty((n * S, O.expanded_record_floats(grid, False)), device=hip_device)
        offsets = torch.empty(nkeys + 1, dtype=torch.int64, device=hip_device)
        cursor = torch.empty(nkeys, dtype=torch.int32, device=hip_device)
        O.bin_offsets(hist, offsets, cursor)
        O.render_backward_emit_direct_raw(grid, o, d, None, S, near, far, flags, caches, g_colour, None, None, 8, cursor, srt, hist_clear=hist)
        lists.append((srt, offsets, False))
    gd = torch.full_like(first, 5.0)
    gf = None if second is None else torch.full_like(second, -5.0)
    O.brick_accumulate_raw(grid, 8, lists, gd, gf, accumulate=False)
    both_d, both_f = grid.unpack(gd, gf)
    np.testing.assert_allclose(both_d.cpu().numpy(), total_d.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(total_d.abs().max()))
    np.testing.assert_allclose(both_f.cpu().numpy(), total_f.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(total_f.abs().max()))
    gd2 = torch.zeros_like(first)
    gf2 = None if second is None else torch.zeros_like(second)
    for one in lists:
        O.brick_accumulate_raw(grid, 8, [one], gd2, gf2, accumulate=True)
    one_d, one_f = grid.unpack(gd2, gf2)
    np.testing.assert_allclose(both_d.cpu().numpy(), one_d.cpu().numpy(), rtol=1e-5, atol=1e-7 * float(total_d.abs().max()))
    np.testing.assert_allclose(both_f.cpu().numpy(), one_f.cpu().numpy(), rtol=1e-5, atol=1e-7 * float(total_f.abs().max()))


def test_autograd_trainer_with_deferred_gradients_equals_the_fused_step(hip_device):
    """TrainStepper(fused=False) on a grid in the reference's own two tensors: forward passes through the torch.autograd.Function
    (rendered from the split shadow), every backward leaves a sorted record list, FusedAdam.step sums all of them in ONE merged brick
    pass with Adam in its flush on the shadow and re-lays the result out into the Parameters.  Must equal the fused step on split
    storage iteration by iteration; ``FlatGrid.materialize()`` must equal plain autograd's gradients."""
    g = load_golden("g9_trainer_trajectory.npz")
    G, _, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F = 27
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=False, white_bkgd=True)
    runs = []
    for storage, fused in (("reference", False), ("split", True)):
        grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G, storage=storage)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, n_rays, learning_rate=float(g["lr"]), fused=fused, data_parallel=False)
        assert stepper.flat.deferred == (not fused)
        losses = []
        for it in range(4):
            rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
            st = stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
            losses.append((st.specular_loss.item(), st.diffuse_loss.item()))
        if not fused:  # the Parameters themselves were updated (they are what a reference user reads and checkpoints)
            assert isinstance(grid.densities, torch.nn.Parameter) and grid.densities.data_ptr() == stepper.flat.flat_param.data_ptr()
        runs.append((losses, grid.densities.detach().clone(), grid.features.detach().clone(), stepper.optimizer.step_count))
    np.testing.assert_allclose(np.array(runs[0][0]), np.array(runs[1][0]), rtol=2e-5)
    assert runs[0][3] == runs[1][3] == 4
    for a, b in ((runs[0][1], runs[1][1]), (runs[0][2], runs[1][2])):
        err = (a - b).abs()
        assert float((err <= 2e-5).float().mean()) >= 0.999 and float(err.max()) <= 0.03 * 2 * 4 + 1e-6
    # the pending lists, summed on demand, are the gradient plain autograd computes
    grids = [relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), G) for _ in range(2)]
    flat = FlatGrid(grids[1], deferred=True)
    assert flat.deferred
    rays = rf.Rays(T(g["origins"][0]).to(hip_device), T(g["directions"][0]).to(hip_device))
    target = T(g["pixels"][0]).to(hip_device)
    for grid in grids:
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        loss = torch.nn.functional.l1_loss(model.render_rays(rays).colour, target)
        loss = loss + torch.nn.functional.l1_loss(model.render_rays(rays, render_diffuse=True).colour, target)
        loss.backward()
    assert len(flat.pending) == 2
    flat.materialize()
    for a, b in ((grids[0].densities.grad, grids[1].densities.grad), (grids[0].features.grad, grids[1].features.grad)):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=2e-4, atol=2e-6 * float(a.abs().max()))
    flat.zero_grad()
    assert flat.pending == []


@pytest.mark.parametrize("storage,bucket", [("split", "none"), ("reference", "none"), ("bricked", "flat"), ("reference", "deferred")])
def test_paired_autograd_node_equals_the_two_single_nodes(hip_device, monkeypatch, storage, bucket):
    """``render_sh_voxel_grid_pair`` / ``VolumetricModel.render_rays_pair`` (both renders of an iteration as ONE autograd node: one
    forward launch, offsets + adjoints in two) against the two single nodes: the same jitter draws (keyed from torch's CPU generator, in
    the same order), outputs bit for bit (the pair kernel runs the single kernels' per-ray code), gradients to the order of the cursor
    atomics -- into fresh tensors, into a flat bucket, as pending lists of a deferred bucket --, upstream gradients of depth and
    accumulated weight (the un-paired adjoints behind the paired forward), and the paired loss against torch's."""
    monkeypatch.setattr(ops, "AUTOGRAD_BACKWARD", "binned")
    cam = hotdog_like_camera()
    dims = (24, 20, 28)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(37, 41, 50.0), rf.pose_spherical(25.0, -35.0, cam["radius"]), hip_device))
    n = len(rays)
    target = T(hash_uniform((n, 3), 19, 0.0, 1.0)).to(hip_device)
    cfg = rf.SHVoxGridRenderConfig(48, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)

    def fresh():
        dens, feat = procedural_grid(dims, 27, 5)
        grid = rf.VoxelGrid(dens.to(hip_device), feat.to(hip_device), rf.VoxelSize(*(3.0 / d for d in dims)), density_preactivation=torch.nn.Identity(),
                            density_postactivation=torch.nn.ReLU(), expected_density_scale=30.0, tunable=True, storage=storage)
        flat = None if bucket == "none" else FlatGrid(grid, deferred=bucket == "deferred")
        return grid, flat, rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)

    def grads(grid, flat):
        if flat is not None and flat.deferred:
            assert len(flat.pending) == 2
            flat.materialize()
        return [t.detach().clone() for t in grid.reference_gradients()]

    for upstream in ("colours", "depth-and-acc"):
        results = []
        for paired in (True, False):
            grid, flat, model = fresh()
            torch.manual_seed(11)
            if paired:
                spec, diff = model.render_rays_pair(rays)
                assert spec.colour.grad_fn is diff.colour.grad_fn is not None and "Pair" in type(spec.colour.grad_fn).__name__
            else:
                spec, diff = model.render_rays(rays), model.render_rays(rays, render_diffuse=True)
            if upstream == "colours":
                total, l0, mse0, l1, mse1 = ops.l1_loss_pair_with_mse(spec.colour, diff.colour, target)
                ref_l0, ref_l1 = torch.nn.functional.l1_loss(spec.colour.detach(), target), torch.nn.functional.l1_loss(diff.colour.detach(), target)
                np.testing.assert_allclose([float(l0), float(l1), float(total)], [float(ref_l0), float(ref_l1), float(ref_l0 + ref_l1)], rtol=2e-6)
                np.testing.assert_allclose([float(mse0), float(mse1)], [float(torch.nn.functional.mse_loss(spec.colour.detach(), target)),
                                                                         float(torch.nn.functional.mse_loss(diff.colour.detach(), target))], rtol=2e-6)
            else:
                total = torch.nn.functional.l1_loss(spec.colour, target) + spec.depth.square().mean() + 0.3 * diff.extra["accumulated_weight"].sum() / n
            total.backward()
            results.append((spec, diff, grads(grid, flat), float(total)))
        (s0, d0, g0, t0), (s1, d1, g1, t1) = results
        for a, b in ((s0, s1), (d0, d1)):
            assert torch.equal(a.colour, b.colour) and torch.equal(a.depth, b.depth) and torch.equal(a.extra["accumulated_weight"], b.extra["accumulated_weight"])
        assert abs(t0 - t1) <= 1e-6 * abs(t1)
        for a, b in zip(g0, g1):
            assert float(b.abs().max()) > 0
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=3e-4, atol=3e-6 * float(b.abs().max()))
    # the paired loss cleans its workspace up after itself: any number of calls, the gradient of its sum = the two L1 gradients
    c0 = s0.colour.detach().clone().requires_grad_(True)
    c1 = d0.colour.detach().clone().requires_grad_(True)
    for _ in range(3):
        total, l0, _, l1, _ = ops.l1_loss_pair_with_mse(c0, c1, target)
    np.testing.assert_allclose(float(total), float(torch.nn.functional.l1_loss(c0, target) + torch.nn.functional.l1_loss(c1, target)), rtol=2e-6)
    (2.0 * total).backward()
    np.testing.assert_allclose(c0.grad.cpu().numpy(), (2.0 * torch.sign(c0.detach() - target) / (3 * n)).cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(c1.grad.cpu().numpy(), (2.0 * torch.sign(c1.detach() - target) / (3 * n)).cpu().numpy(), rtol=1e-6)


_PAIR_SCRIPT = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
import thr3ed_atom_amd as rf
from thr3ed_atom_amd.trainers import TrainStepper
from tests.helpers import hash_uniform, hotdog_like_camera, procedural_grid
dev = torch.device("cuda:0")
cam = hotdog_like_camera()
dens, feat = procedural_grid((24, 24, 24), 27, 5)
grid = rf.VoxelGrid(torch.from_numpy(np.asarray(dens)).to(dev), torch.from_numpy(np.asarray(feat)).to(dev), rf.VoxelSize(3.0 / 24, 3.0 / 24, 3.0 / 24),
                    rf.VoxelGridLocation(), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(),
                    expected_density_scale=30.0, tunable=True, storage="split")
cfg = rf.SHVoxGridRenderConfig(96, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)
model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(31, 33, 40.0), rf.pose_spherical(25.0, -35.0, cam["radius"]), dev))
n = rays.origins.shape[0]
pixels = torch.from_numpy(np.asarray(hash_uniform((n, 3), 19, 0.0, 1.0))).to(dev)
st = TrainStepper(model, n, learning_rate=0.03, fused=True, backward="binned")
losses = []
for it in range(4):
    t_rands = [torch.from_numpy(np.asarray(hash_uniform((n, 96), 100 + 2 * it + i, 0.0, 1.0))).clamp_(0.0, 1.0 - 2.0**-24).to(dev) for i in range(2)]
    s = st.step_on(rays, pixels, t_rand=t_rands)
    losses.append([float(s.specular_loss), float(s.diffuse_loss)])
torch.cuda.synchronize()
d, f = grid.densities.detach().double(), grid.features.detach().double()
print("RESULT " + json.dumps(dict(losses=losses, sums=[float(d.sum()), float(d.abs().sum()), float(f.sum()), float(f.abs().sum())])))
"""


@pytest.mark.gpu
def test_paired_launches_equal_one_launch_per_render(hip_device):
    """rf_train_step runs both renders of an iteration in one launch and both adjoints in one launch; $RF_FWD_PAIR=0 / $RF_EMIT_PAIR=0
    (read once per process) restore one launch per render: same losses, parameters equal to the rounding of the (unordered) cursor
    atomics -- the per-ray code is the same function in both."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for pair in ("1", "0"):
        env = dict(os.environ, RF_FWD_PAIR=pair, RF_EMIT_PAIR=pair)
        r = subprocess.run([sys.executable, "-c", _PAIR_SCRIPT.format(root=root)], env=env, capture_output=True, text=True, timeout=600, cwd=root)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        assert line, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(json.loads(line[0][len("RESULT "):]))
    np.testing.assert_allclose(np.array(outs[0]["losses"]), np.array(outs[1]["losses"]), rtol=2e-6)
    np.testing.assert_allclose(outs[0]["sums"], outs[1]["sums"], rtol=1e-6)


@pytest.mark.parametrize("dims,deg,storage", [((40, 40, 40), 2, "split"), ((38, 41, 43), 2, "split"), ((21, 30, 26), 0, "split"), ((42, 24, 40), 2, "bricked")])
def test_bricks_of_4x8x8_nodes_equal_cubic_bricks(hip_device, dims, deg, storage):
    """RF_BRICK_4X8X8 (the default of the single-process fused step: 256-thread workgroups on bricks of 4 x 8 x 8 nodes, twice the
    keys) against brick_size 8 -- same rays, same jitter keys: the record lists hold the same records (per-key order aside), and
    parameters and both Adam moments agree to float32 summation order after three iterations; grids whose x extent is no multiple of
    4 (partial bricks), SH degree 0 (one list kind) and the bricked node order included.  Also the lists summed into gradient
    TENSORS (rf_brick_accumulate, the deferred bucket's materialize()) for both brick shapes."""
    X, Y, Z = dims
    F = 3 * (deg + 1) ** 2
    S, n = 64, 2048
    cam = hotdog_like_camera()
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(48, 48, 66.0), rf.pose_spherical(20.0, -30.0, cam["radius"]), hip_device))[:n]
    pixels = T(hash_uniform((n, 3), 33, 0.0, 1.0)).to(hip_device)
    results, lists_of = [], []
    for brick_size in (8, ops.BRICK_4X8X8):
        grid = rf.VoxelGrid(T(hash_uniform((X, Y, Z, 1), 31)).to(hip_device), T(hash_uniform((X, Y, Z, F), 32)).to(hip_device), rf.VoxelSize(3.0 / X, 3.0 / Y, 3.0 / Z),
                            density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0,
                            tunable=True, storage=storage)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        st = TrainStepper(model, n, learning_rate=0.03, fused=True, backward="binned", data_parallel=False, brick_size=brick_size)
        assert st.fuse_optimizer and st.brick_size == brick_size
        torch.manual_seed(5)  # (the jitter keys of the renders come from torch's CPU generator)
        for _ in range(3):
            st.step_on(rays, pixels)
        torch.cuda.synchronize()
        t = st._exec["tensors"]
        nrec = [int(t["offsets2"][k][-1]) for k in range(2)]
        assert nrec[0] > 1000 and nrec[1] > 1000
        lists_of.append((grid, brick_size, [(t["pass0"]["sorted"], t["offsets2"][0], False), (t["pass1"]["sorted"], t["offsets2"][1], True)], nrec))
        results.append((st.flat.flat_param.clone(), st.optimizer.exp_avg.clone(), st.optimizer.exp_avg_sq.clone()))
    assert lists_of[0][3] == lists_of[1][3]  # the same samples emit records
    for a, b in zip(results[0], results[1]):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 5e-6 * max(scale, 1e-30) + (2e-5 if a is results[0][0] else 0.0), (float((a - b).abs().max()), scale)
    # the lists of the last iteration as gradient tensors: 4 x 8 x 8 bricks == cubic bricks (each on its own grid's lists)
    grads = []
    for grid, brick_size, lists, _ in lists_of:
        first, second = grid.kernel_tensors()
        gd, gf = torch.full_like(first, 7.0), (None if second is None else torch.full_like(second, 7.0))
        ops.brick_accumulate_raw(grid, brick_size, lists, gd, gf, accumulate=False)
        torch.cuda.synchronize()
        grads.append((gd, gf))
    for a, b in zip(grads[0], grads[1]):
        if a is None:
            continue
        scale = float(a.abs().max())
        assert scale > 0 and float((a - b).abs().max()) <= 2e-5 * scale, (float((a - b).abs().max()), scale)


def test_auto_backward_policy(hip_device, monkeypatch):
    """backward="auto" (the default): the atomic adjoint on the first grids of a progressive schedule -- fewer than 256 bricks of 8^3
    nodes: a handful of brick workgroups would sum the whole batch's records --, the binned one with the optimizer in the brick flush
    from there on; and the two agree on a grid at the boundary after a few iterations (losses to rounding, parameters to Adam's
    tolerance)."""
    monkeypatch.delenv("RF_AUTO_BINNED_MIN_BRICKS", raising=False)
    cam = hotdog_like_camera()
    S, n, F = 48, 2048, 27
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(48, 48, 66.0), rf.pose_spherical(20.0, -30.0, cam["radius"]), hip_device))[:n]
    pixels = T(hash_uniform((n, 3), 33, 0.0, 1.0)).to(hip_device)
    picked, results = {}, {}
    for G in (16, 48, 56):
        for backward in ("auto", "binned", "atomic"):
            if backward != "auto" and G != 48:
                continue
            grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 31)), T(hash_uniform((G, G, G, F), 32)), G, storage="split")
            model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
            st = TrainStepper(model, n, learning_rate=0.03, data_parallel=False, backward=backward)
            if backward == "auto":
                picked[G] = (st.backward, st.fuse_optimizer)
            if G == 48:
                torch.manual_seed(9)
                losses = []
                for _ in range(3):
                    s_ = st.step_on(rays, pixels)
                    losses.append((s_.specular_loss.item(), s_.diffuse_loss.item()))
                results[backward] = (losses, st.flat.flat_param.clone())
    assert picked[16] == ("atomic", False) and picked[48] == ("atomic", False) and picked[56] == ("binned", True)  # 8 / 216 / 343 bricks
    np.testing.assert_allclose(np.array(results["binned"][0]), np.array(results["atomic"][0]), rtol=2e-5)
    np.testing.assert_allclose(np.array(results["auto"][0]), np.array(results["atomic"][0]), rtol=2e-5)
    err = (results["binned"][1] - results["atomic"][1]).abs()
    assert float((err <= 2e-5).float().mean()) >= 0.999 and float(err.max()) <= 0.03 * 2 * 3 + 1e-6


def test_bricks_of_4x8x8_nodes_at_256_cubed(hip_device):
    """The largest grid the 4 x 8 x 8 brick pass takes (2^24 nodes: the one-round flush's 24-bit node indices, 524288 keys): two
    iterations against cubic bricks, parameters and moments to float32 summation order."""
    G, F, S, n = 256, 27, 128, 4096
    cam = hotdog_like_camera()
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(64, 64, 88.0), rf.pose_spherical(20.0, -30.0, cam["radius"]), hip_device))[:n]
    pixels = T(hash_uniform((n, 3), 33, 0.0, 1.0)).to(hip_device)
    gen = torch.Generator(device=hip_device).manual_seed(11)
    dens0 = torch.rand((G, G, G, 1), generator=gen, device=hip_device) * 2.0 - 1.0
    feat0 = torch.rand((G, G, G, F), generator=gen, device=hip_device) * 2.0 - 1.0
    results = []
    for brick_size in (8, ops.BRICK_4X8X8):
        grid = rf.VoxelGrid(dens0.clone(), feat0.clone(), rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                            density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=True, storage="split")
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        st = TrainStepper(model, n, learning_rate=0.03, fused=True, backward="binned", data_parallel=False, brick_size=brick_size)
        assert st.fuse_optimizer
        torch.manual_seed(5)
        for _ in range(2):
            st.step_on(rays, pixels)
        torch.cuda.synchronize()
        results.append((st.flat.flat_param.clone(), st.optimizer.exp_avg.clone(), st.optimizer.exp_avg_sq.clone()))
        st.flat.detach()
        del st, model, grid
        torch.cuda.empty_cache()
    for k, (a, b) in enumerate(zip(results[0], results[1])):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 5e-6 * scale + (2e-5 if k == 0 else 0.0), (k, float((a - b).abs().max()), scale)
    assert float(results[0][1].abs().max()) > 0  # (gradients arrived)


@pytest.mark.parametrize("copies,parts", [(2, 2), (5, 3), (8, 2), (8, 8), (3, 4)])
def test_split_brick_pass_equals_the_plain_owner_pass(hip_device, copies, parts):
    """rf_brick_accumulate_adam_split (several workgroups per owned brick: the source ranks' lists dealt out, partial accumulator
    images merged by the last workgroup to arrive -- across XCDs, inside one launch) == rf_brick_accumulate_adam_range on the same
    lists and the same optimizer state: parameters and both Adam moments to float32 summation order, the scratch left clean.
    ``copies`` copies of this GPU's own record lists stand in for the ranks' lists."""
    G, S, n = 40, 64, 2048
    F = 27
    cam = hotdog_like_camera()
    grid = relu_grid(hip_device, T(hash_uniform((G, G, G, 1), 31)), T(hash_uniform((G, G, G, F), 32)), G, storage="split")
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=True, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(48, 48, 66.0), rf.pose_spherical(20.0, -30.0, cam["radius"]), hip_device))[:n]
    pixels = T(hash_uniform((n, 3), 33, 0.0, 1.0)).to(hip_device)
    st = TrainStepper(model, n, learning_rate=0.03, fused=True, backward="binned", data_parallel=False, brick_size=8)  # (owners sum 8^3 bricks)
    for _ in range(2):
        st.step_on(rays, pixels)
    torch.cuda.synchronize()
    t, opt = st._exec["tensors"], st.optimizer
    nd = st.flat.flat_gradient_parts()[0].numel()
    m, v = (opt.exp_avg[:nd], opt.exp_avg[nd:]), (opt.exp_avg_sq[:nd], opt.exp_avg_sq[nd:])
    lists = [(t["pass0"]["sorted"], t["offsets2"][0], False)] * copies + [(t["pass1"]["sorted"], t["offsets2"][1], True)] * copies
    assert int(t["offsets2"][0][-1]) > 1000 and int(t["offsets2"][1][-1]) > 1000
    nb = (G + 7) // 8
    rng = (nb * nb, 3 * nb * nb)  # x-slabs 1..3 of bricks
    state0 = (st.flat.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())

    def run(split):
        for dst, src in zip((st.flat.flat_param, opt.exp_avg, opt.exp_avg_sq), state0):
            dst.copy_(src)
        ops.brick_accumulate_adam_raw(grid, 8, lists, m, v, 0.03, 0.9, 0.999, 1e-8, 3, brick_range=rng, split=split)
        torch.cuda.synchronize()
        return st.flat.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()

    ref = run(None)
    scratch = ops.brick_split_scratch(grid, rng[1], parts)
    for repeat in range(2):  # (the second launch finds the counters the first one left)
        got = run((parts, scratch))
        assert int(scratch.view(torch.int32)[: rng[1] * (1 + parts)].abs().sum()) == 0
        assert float((got[0] - state0[0]).abs().max()) > 1e-3  # (something was updated)
        for a, b in zip(got, ref):
            scale = float(b.abs().max())
            assert float((a - b).abs().max()) <= 2e-6 * max(scale, 1.0) + 1e-4 * scale * 0 + 3e-6 * scale, (float((a - b).abs().max()), scale)
    with pytest.raises(RuntimeError):  # too small a scratch is refused before anything is launched
        ops.brick_accumulate_adam_raw(grid, 8, lists, m, v, 0.03, 0.9, 0.999, 1e-8, 3, brick_range=rng, split=(parts, scratch[: scratch.numel() // 2]))


def test_l1_loss_with_mse_equals_torch(hip_device):
    """ops.l1_loss_with_mse (one launch, a torch.autograd.Function) against torch.nn.functional.l1_loss / mse_loss and their autograd,
    which the reference's trainer calls (modules/trainers.py:311-317): values, the gradient incl. sign(0) = 0, an upstream factor."""
    n = 5000
    colour = T(hash_uniform((n, 3), 71, 0.0, 1.0)).to(hip_device)
    target = T(hash_uniform((n, 3), 72, 0.0, 1.0)).to(hip_device)
    colour[:7] = target[:7]  # exact zeros of the difference
    for _ in range(3):  # (several slots of the sums ring)
        a = colour.clone().requires_grad_(True)
        b = colour.clone().requires_grad_(True)
        loss, mse = ops.l1_loss_with_mse(a, target)
        ref = torch.nn.functional.l1_loss(b, target)
        np.testing.assert_allclose(loss.item(), ref.item(), rtol=2e-6)
        np.testing.assert_allclose(mse.item(), torch.nn.functional.mse_loss(b.detach(), target).item(), rtol=2e-6)
        assert not mse.requires_grad
        (2.5 * loss).backward()
        (2.5 * ref).backward()
        assert torch.equal(a.grad[:7], torch.zeros_like(a.grad[:7]))
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("dims,deg", [((16, 16, 16), 2), ((20, 24, 32), 2), ((16, 16, 16), 0), ((12, 16, 16), 2), ((16, 12, 16), 2)])
def test_mirror_flush_keeps_the_parameters_in_sync(hip_device, monkeypatch, dims, deg):
    """The strict drop-in's optimizer step (optim.FusedAdam on deferred record lists of a reference-storage grid): the brick flush
    that updates the split shadow writes the Parameters' own layout as well (rf_brick_accumulate_adam_mirror): after every step the
    Parameters hold, bit for bit, what the shadow holds -- like with the separate re-layout launch ($RF_MIRROR_FLUSH=0) --, for both
    tensors, both SH degrees it covers, non-cubic grids and grids it does not take (dims not multiples of the brick: the launch stays)."""
    from thr3ed_atom_amd import optim

    F = 3 * (deg + 1) ** 2
    cam = hotdog_like_camera()
    cfg = rf.SHVoxGridRenderConfig(48, rf.CameraBounds(cam["near"], cam["far"]), perturb_sampled_points=False, white_bkgd=True)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(32, 32, 44.0), rf.pose_spherical(20.0, -30.0, cam["radius"]), hip_device))
    pixels = T(hash_uniform((len(rays), 3), 33, 0.0, 1.0)).to(hip_device)
    out = []
    for mirror in (True, False):
        monkeypatch.setattr(optim, "MIRROR_FLUSH", mirror)
        grid = rf.VoxelGrid(T(hash_uniform((*dims, 1), 31)).to(hip_device), T(hash_uniform((*dims, F), 32)).to(hip_device), rf.VoxelSize(3.0 / dims[0], 3.0 / dims[1], 3.0 / dims[2]),
                            density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=True)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        st = TrainStepper(model, len(rays), learning_rate=0.03, fused=False, data_parallel=False)
        assert st.flat.deferred
        applies = ops.mirror_flush_applies(grid, st.flat.brick_size, grid.densities.data, grid.features.data)
        assert applies == (dims[0] % 4 == 0 and dims[1] % 8 == 0 and dims[2] % 8 == 0)
        for _ in range(3):
            st.step_on(rays, pixels)
        torch.cuda.synchronize()
        # the Parameters == the shadow the next forward pass renders from (converted back by the library)
        sh, _ = grid._shadow(refresh=False)
        base, rest = sh["base"], sh["rest"]
        assert torch.equal(grid.densities.detach()[..., 0], base[..., 0])
        K = F // 3
        feat = grid.features.detach().reshape(*dims, 3, K)
        assert torch.equal(feat[..., 0], base[..., 1:4])
        if K > 1:
            assert torch.equal(feat[..., 1:], rest.reshape(*dims, 3, K - 1))
        out.append((grid.densities.detach().clone(), grid.features.detach().clone()))
        st.flat.detach()
    # ... and the two ways agree with each other up to the run-to-run summation order of the record lists (atomic cursors)
    for a, b in zip(out[0], out[1]):
        err = (a - b).abs()
        assert float((err <= 2e-5).float().mean()) >= 0.999 and float(err.max()) <= 0.03 * 2 * 3 + 1e-6
