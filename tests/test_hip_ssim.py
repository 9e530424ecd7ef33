"""rf_ssim_forward / rf_ssim_backward on the GPU against the float64 model (tests/ssim_model.py): every map pixel under the rounding
bound, the mean, strided layouts bit for bit, the adjoint against float64 autograd with the float32 F.conv2d restatement as the
yardstick, and the three places that use SSIM: held-out evaluation, the trainer's periodic test, pose refinement.  The figures the
tests print are collected in docs/ssim_errors.md."""
import functools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import ssim_model as sm
from tests.helpers import hash_uniform, hotdog_like_camera, procedural_grid
from thr3ed_atom_amd import _lib, ops
from thr3ed_atom_amd.trainers import (
    PosedImagesInMemory,
    evaluate_sh_vox_grid_vol_mod_with_posed_images,
    test_sh_vox_grid_vol_mod_with_posed_images,
    train_sh_vox_grid_vol_mod_with_posed_images,
)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(case, C, kind):
    """(image, target, float64 map, bound): computed once per case and shared"""
    padding, H, W = case
    x, y = sm.images(kind, H, W, C)
    return x, y, sm.ssim_map(x, y, padding), sm.rounding_bound(x, y, padding)


def test_tile_constants_match_the_model():
    assert _lib.SSIM_TILE == (sm.TILE_H, sm.TILE_W) and _lib.SSIM_WINDOW == sm.WINDOW


@pytest.mark.parametrize("case", sm.CASES, ids=sm.case_id)
def test_map_under_the_bound_and_mean(case, hip_device):
    """1. every pixel of the map within the rounding bound of the float64 model (kappa = 26); 2. the mean within
    16 u mean|map| of the float64 mean of the kernel's own map (a float32 tree of depth 9 inside a tile, float64 across the tiles),
    and exactly 1.0 for equal images."""
    padding = case[0]
    for C in (1, 3):
        for kind in sm.KINDS:
            x, y, m64, bound = reference(case, C, kind)
            mean, smap = rf.ssim(x.to(hip_device), y.to(hip_device), padding=padding, return_map=True)
            smap, mean = smap.cpu(), mean.cpu()
            assert smap.shape == m64.shape and mean.shape == () and mean.dtype == torch.float32
            assert bool(torch.isfinite(bound).all())
            ratio = ((smap.double() - m64).abs() / bound).max().item()
            own = smap.double().mean().item()
            mean_err, mean_tol = abs(float(mean) - own), 16 * sm.U * smap.double().abs().mean().item()
            print(f"SSIM_MAP | {sm.case_id(case)} | {C} | {kind} | {ratio:.3f} | {bound.max().item():.2e} | {mean_err / mean_tol:.3f}")
            assert ratio <= 1.0, (kind, C, ratio)
            assert mean_err <= mean_tol, (kind, C, mean_err, mean_tol)
            if kind == "equal":
                assert bool((smap == 1.0).all()) and float(mean) == 1.0
            plain = rf.ssim(x.to(hip_device), y.to(hip_device), padding=padding)  # (no map, no derivative maps: the same bits)
            assert torch.equal(plain.cpu(), mean)


@pytest.mark.parametrize("case", [("valid", 27, 43), ("same", 17, 33), ("same", 5, 7)], ids=sm.case_id)
def test_layouts_give_the_same_bits(case, hip_device):
    """3. contiguous [H, W, C], a [C, H, W] tensor seen through .permute(1, 2, 0), one of each, and a crop of a larger frame: the
    kernel addresses by strides, so the same values give bitwise the same map and mean; so do two runs."""
    padding, H, W = case
    x, y, _, _ = reference(case, 3, "smooth")
    x, y = x.to(hip_device), y.to(hip_device)
    chw = lambda t: t.permute(2, 0, 1).contiguous().permute(1, 2, 0)  # noqa: E731

    def crop(t):
        big = torch.full((H + 7, W + 5, 3), 0.25, device=hip_device)
        big[3:3 + H, 2:2 + W] = t
        return big[3:3 + H, 2:2 + W]

    base_mean, base_map = rf.ssim(x, y, padding=padding, return_map=True)
    variants = {"again": (x, y), "chw": (chw(x), chw(y)), "mixed": (x, chw(y)), "mixed2": (chw(x), y), "crop": (crop(x), crop(y)), "crop+chw": (crop(x), chw(y))}
    assert not chw(x).is_contiguous() and not crop(x).is_contiguous()
    for name, (a, b) in variants.items():
        mean, smap = rf.ssim(a, b, padding=padding, return_map=True)
        assert torch.equal(mean, base_mean) and torch.equal(smap, base_map), name


@pytest.mark.parametrize("case", sm.CASES, ids=sm.case_id)
def test_gradient_against_float64_autograd(case, hip_device):
    """4. d [3 (1 - ssim)] / d image against float64 autograd.  The tolerance is measured here: the kernel's |g - g64|_inf / |g64|_inf
    may be at most 4 x that of the float32 F.conv2d autograd restatement on the same case (the kernel sums 22 separable terms in
    another order than the restatement's 121) + 1e-6.  An [H, W, C] leaf and a [C, H, W] leaf through the permuted view."""
    padding = case[0]
    for C in (1, 3):
        for kind in ("noise", "smooth"):
            x, y, _, _ = reference(case, C, kind)
            g64 = sm.dssim_grad(x, y, padding)
            scale = g64.abs().max().item()
            yardstick = (sm.dssim_grad(x, y, padding, dtype=torch.float32).double() - g64).abs().max().item() / scale
            tol = 4.0 * yardstick + 1e-6
            hwc = x.to(hip_device).requires_grad_(True)
            (3.0 * (1.0 - rf.ssim(hwc, y.to(hip_device), padding=padding))).backward()
            chw = x.permute(2, 0, 1).contiguous().to(hip_device).requires_grad_(True)
            (3.0 * (1.0 - rf.ssim(chw.permute(1, 2, 0), y.to(hip_device), padding=padding))).backward()
            assert chw.grad.shape == (C, *x.shape[:2]) and chw.grad.is_contiguous()
            assert torch.equal(chw.grad.permute(1, 2, 0), hwc.grad)  # the same gradient bits in either layout
            ours = (hwc.grad.cpu().double() - g64).abs().max().item() / scale
            print(f"SSIM_GRAD | {sm.case_id(case)} | {C} | {kind} | {ours:.2e} | {yardstick:.2e} | {ours / tol:.3f}")
            assert ours <= tol, (kind, C, ours, yardstick)


def test_gradient_is_reproducible_and_target_grad_is_refused(hip_device):
    x, y, _, _ = reference(("same", 37, 50), 3, "noise")
    grads = []
    for _ in range(2):
        leaf = x.to(hip_device).requires_grad_(True)
        rf.ssim(leaf, y.to(hip_device), padding="same").backward()
        grads.append(leaf.grad)
    assert torch.equal(grads[0], grads[1])
    with pytest.raises(ValueError, match="symmetric"):
        rf.ssim(x.to(hip_device), y.to(hip_device).requires_grad_(True))
    with pytest.raises(ValueError):
        rf.ssim(x.to(hip_device)[:10], y.to(hip_device)[:10])  # "valid" below 11 rows
    with pytest.raises(ValueError):
        rf.ssim(x.to(hip_device), y.to(hip_device), padding="reflect")
    # the raw entry points: a forward without gradient writes neither map nor derivative maps
    mean, smap, dmaps = ops.ssim_forward_raw(x.to(hip_device), y.to(hip_device), "valid")
    assert smap is None and dmaps is None and mean.shape == ()


# ---- the users of SSIM ---------------------------------------------------------------------------------------------------------------
def _scene(dev, hw=(24, 20)):
    cam = hotdog_like_camera()
    dens, feat = procedural_grid((8, 8, 8), 12, 41)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(3.0 / 8, 3.0 / 8, 3.0 / 8), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=True)
    bounds = rf.CameraBounds(cam["near"], cam["far"])
    cfg = rf.SHVoxGridRenderConfig(24, bounds, perturb_sampled_points=False, white_bkgd=True, render_num_samples_per_ray=40)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    intr = rf.CameraIntrinsics(hw[0], hw[1], 27.0)
    poses = [rf.pose_spherical(70.0 * k, -35.0, cam["radius"]) for k in range(3)]
    images = torch.from_numpy(hash_uniform((3, 3, *hw), 4, 0.0, 1.0))
    pose_mat = torch.stack([torch.cat([p.rotation, p.translation], dim=1) for p in poses])
    return model, PosedImagesInMemory(images.to(dev), pose_mat.to(dev), intr, bounds), poses, intr


def test_evaluation_loop(hip_device):
    """5. PSNR is the existing test loop's, exactly; each per-image SSIM is the model's on the same render within the bound's mean"""
    model, data, poses, intr = _scene(hip_device)
    scores = evaluate_sh_vox_grid_vol_mod_with_posed_images(model, data)
    assert set(scores) == {"psnr", "ssim", "per_image"} and len(scores["per_image"]) == 3
    assert scores["psnr"] == test_sh_vox_grid_vol_mod_with_posed_images(model, data)
    assert scores["ssim"] == float(np.mean([r["ssim"] for r in scores["per_image"]]))
    for k, row in enumerate(scores["per_image"]):
        assert set(row) == {"psnr", "ssim"}
        with torch.no_grad():
            render = model.render(poses[k], intr, optimized_sampling=False, num_samples_per_ray=40).colour.cpu()
        target = data.images[k].permute(1, 2, 0).cpu()
        want = sm.ssim_mean(render, target, "valid").item()
        tol = sm.rounding_bound(render, target, "valid").mean().item()
        print(f"SSIM_EVAL | image {k} | {row['ssim']:.6f} | {want:.6f} | {abs(row['ssim'] - want) / tol:.3f}")
        assert abs(row["ssim"] - want) <= tol


def test_trainer_reports_ssim_only_when_asked(hip_device):
    """5. report_ssim=True adds test_ssim to the periodic test's rows; False leaves the history as it was"""
    histories = {}
    for flag in (False, True):
        torch.manual_seed(3)
        model, data, _, _ = _scene(hip_device)
        history = []
        kwargs = {"report_ssim": True} if flag else {}
        train_sh_vox_grid_vol_mod_with_posed_images(model, data, None, test_dataset=data, ray_batch_size=128, num_stages=1, num_iterations_per_stage=2,
                                                    image_batch_cache_size=3, test_freq=1, summary_freq=100, save_freq=1000, log=lambda s: None,
                                                    history=history, random_initializer=lambda t: t, **kwargs)
        histories[flag] = history
    off, on = ([r for r in histories[f] if "test_psnr" in r] for f in (False, True))
    assert len(off) == len(on) == 2
    assert all(set(r) == {"global_step", "test_psnr"} for r in off) and all(set(r) == {"global_step", "test_psnr", "test_ssim"} for r in on)
    assert all(-1.0 <= r["test_ssim"] <= 1.0 for r in on)
    assert [set(r) for r in histories[False]] == [set(r) - {"test_ssim"} for r in histories[True]]


def test_pose_refinement_with_dssim(hip_device):
    """6. dssim_weight=0 is the plain path bit for bit; with sampled rays it is refused; on full frames the first loss is
    (1 - w) L1 + w (1 - SSIM_same) of the model on that render, and the pose receives a gradient"""
    model, _, poses, _ = _scene(hip_device)
    intr = rf.CameraIntrinsics(24, 24, 30.0)
    with torch.no_grad():
        target = model.render(poses[1], intr, num_samples_per_ray=32).colour
    start = rf.perturb_pose(poses[1], torch.tensor([0.02, -0.01, 0.015]), torch.tensor([0.02, -0.03, 0.01]))
    kwargs = dict(num_iterations=3, learning_rate=1e-2, num_samples_per_ray=32)
    _, plain = rf.refine_camera_pose(model, target, intr, start, **kwargs)
    _, zero = rf.refine_camera_pose(model, target, intr, start, dssim_weight=0.0, **kwargs)
    for a, b in zip(plain, zero):
        assert a["loss"] == b["loss"] and np.array_equal(a["rotation"], b["rotation"]) and np.array_equal(a["translation"], b["translation"])
    with pytest.raises(ValueError, match="whole frame"):
        rf.refine_camera_pose(model, target, intr, start, dssim_weight=0.2, rays_per_iteration=100, **kwargs)
    _, mixed = rf.refine_camera_pose(model, target, intr, start, dssim_weight=0.2, **kwargs)
    start_dev = rf.CameraPose(start.rotation.to(hip_device), start.translation.to(hip_device).reshape(3, 1))
    with torch.no_grad():  # the first iteration's render, by the refinement's own path (rays cast from the unperturbed start pose)
        zero3 = torch.zeros(3, device=hip_device)
        first_rays = rf.flatten_rays(rf.cast_rays(intr, rf.perturb_pose(start_dev, zero3, zero3), hip_device))
        first = model.render_rays(first_rays, num_samples_per_ray=32).colour.reshape(24, 24, 3).cpu()
    l1 = (first.double() - target.cpu().double()).abs().mean().item()
    want = 0.8 * l1 + 0.2 * (1.0 - sm.ssim_mean(first, target.cpu(), "same").item())
    tol = 1e-6 + 0.2 * sm.rounding_bound(first, target.cpu(), "same").mean().item()
    print(f"SSIM_POSE | first loss {mixed[0]['loss']:.7f} | model {want:.7f} | L1 alone {plain[0]['loss']:.7f}")
    assert abs(mixed[0]["loss"] - want) <= tol and abs(mixed[0]["loss"] - plain[0]["loss"]) > 10 * tol
    assert all(np.isfinite(h["loss"]) for h in mixed)
    # the gradient reaches the pose parameters through D-SSIM alone
    omega = torch.zeros(3, device=hip_device, requires_grad=True)
    tau = torch.zeros(3, device=hip_device, requires_grad=True)
    pose = rf.perturb_pose(start_dev, omega, tau)
    rays = rf.flatten_rays(rf.cast_rays(intr, pose, hip_device))
    params = list(model.thre3d_repr.parameters())
    for p in params:
        p.requires_grad_(False)
    out = model.render_rays(rays, num_samples_per_ray=32)
    (1.0 - rf.ssim(out.colour.reshape(24, 24, 3), target, padding="same")).backward()
    for g in (omega.grad, tau.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
