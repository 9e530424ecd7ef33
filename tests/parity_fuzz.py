"""Randomised parity sweep of the HIP path against the oracle -- test infrastructure (it calls the oracle), on a GPU box:

    python -m tests.parity_fuzz [--cases N] [--seed S] [--kind rays|frames|train|misc|composed|binding|long|longframes|longtrain|all]
                                [--mode relu|softplus|abs|identity] [--only i,j,...] [--verbose]

tests/test_hip_parity_fuzz.py replays a fixed set of its cases.

Every case draws a configuration the parametrised tests do not enumerate -- grid dims 2..22 per axis (also below the packet
kernel's 4-node minimum), anisotropic voxels, off-centre location, SH degree, density mode, storage, diffuse / AABB sampling /
background, 1..150 samples, rays that start inside the volume or miss it, odd frame sizes, partial pixel ranges, occupancy mask,
either frame kernel -- and holds the result to the bars of tests/test_hip_parity.py (colour / acc 1e-5, depth 2e-5, gradients to
float32 summation order).  The oracle is the checker (test infrastructure); failures are printed with the case's seed."""
import argparse
import os
import sys
import traceback

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402
from oracle import relu_field_oracle as orc  # noqa: E402
from tests.helpers import hash_uniform, identity_regime, procedural_grid, signed_density_grid  # noqa: E402

TOL = 1e-5
FORCE_MODE = ""
LONG_RAYS = False
BIG_GRIDS = False
ACTS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()), "abs": (torch.abs, torch.nn.Identity()),
        "identity": (torch.nn.Identity(), torch.nn.Identity())}
# Identity/Identity densities are signed (never drawn at random: --mode identity / run_case(..., mode="identity")).  Their grids follow
# tests/helpers.py signed_density_grid, and a ray enters the comparison only if the float64 oracle keeps its transmittance below 8 and
# its last sample (interval 1e10 |d|) off a negative density -- there the reference's own alpha is -inf.  Per identity case:
# (usable rays, rays, min sigma delta over the usable rays), for the replay's non-vacuity check.
IDENTITY_STATS = []


def make_grid(dev, dens, feat, voxel, loc, mode, rho, storage, tunable):
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*voxel), rf.VoxelGridLocation(*loc), density_preactivation=ACTS[mode][0],
                        density_postactivation=ACTS[mode][1], expected_density_scale=rho, tunable=tunable, storage=storage)


def draw_grid(dims, F, seed, mode):
    return signed_density_grid(dims, F, seed % 100000) if mode == "identity" else procedural_grid(dims, F, seed % 100000)


def identity_usable(dens, feat, o, d, aabb, near, far, S, rho, white, diffuse=False, opt=False, t_rand=None, jitter_unknown=False):
    """rays of an identity case that enter the comparison (see IDENTITY_STATS), from the oracle: the transmittance in float64, the last
    sample in float32 as well (with AABB sampling it lies ON the exit face, where the two precisions may disagree on `inside`).
    jitter_unknown: the render jitters with a table not drawn yet -- the ray must also have left the box before the last bin starts."""
    with torch.no_grad():
        r64 = orc.render(dens.double(), feat.double(), o.double(), d.double(), aabb, near, far, S, rho, "identity", white_bkgd=white, render_diffuse=diffuse,
                         optimized_sampling=opt, t_rand=None if t_rand is None else t_rand.double())
        r32 = orc.render(dens, feat, o, d, aabb, near, far, S, rho, "identity", white_bkgd=white, render_diffuse=diffuse, optimized_sampling=opt, t_rand=t_rand)
    xmin, _, usable = identity_regime(r64["processed"], r64["deltas"])
    usable &= (r32["processed"][:, -1, 3] >= 0) & torch.isfinite(r32["colour"]).all(dim=-1)
    # (and sum |w| <= 3: weights alpha T of either sign, |alpha| up to e^|x| - 1, cancel in the float32 sums of both sides -- beyond a few
    # units that noise alone reaches the absolute bars, which were set for 0 <= w, sum w <= 1)
    usable &= r64["weights"].abs().sum(dim=-1) <= 3.0
    if jitter_unknown and S > 1:
        bounds, hit = orc.ray_aabb_bounds(o, d, near, far, aabb)
        usable &= ~hit.reshape(-1) | (bounds[:, 1] < r64["z"][:, -2].float())
    IDENTITY_STATS.append((int(usable.sum()), len(usable), float(xmin[usable].min()) if bool(usable.any()) else 0.0))
    return usable


def draw_common(rng):
    dims = tuple(int(rng.integers(2, 23)) for _ in range(3))
    deg = int(rng.integers(0, 4))
    mode = str(rng.choice(["relu", "relu", "softplus", "abs"]))
    if FORCE_MODE:
        mode = FORCE_MODE
    storage = str(rng.choice(["reference", "split", "bricked"]))
    extent = [float(rng.uniform(1.5, 3.5)) for _ in range(3)]
    voxel = tuple(e / d for e, d in zip(extent, dims))
    loc = tuple(float(rng.uniform(-0.3, 0.3)) for _ in range(3))
    if mode == "identity":
        rho = float(rng.choice([2.0, 5.0, 10.0]))
    else:
        rho = 1.0 if mode == "abs" else float(rng.choice([1.0, 9.0, 100.0 / 3.0]))
    return dims, deg, mode, storage, voxel, loc, rho


def case_rays(rng, dev, seed):
    dims, deg, mode, storage, voxel, loc, rho = draw_common(rng)
    F = 3 * (deg + 1) ** 2
    dens, feat = draw_grid(dims, F, seed, mode)
    n = int(rng.integers(1, 400))
    S = int(rng.choice([1, 2, 3, 17, 40, 63, 64, 65, 128, 150]))
    if LONG_RAYS:  # sample counts around the kernels' internal group sizes (64-sample chunks, 64 chunk masks = 4096 samples per mask group)
        n = int(rng.integers(1, 24))
        S = int(rng.choice([255, 256, 257, 1000, 1024, 4095, 4096, 4097, 4160, 5000]))
    o = torch.from_numpy(hash_uniform((n, 3), seed + 1))
    radius = torch.from_numpy(hash_uniform((n, 1), seed + 2, 0.2, 5.0))  # some origins INSIDE the volume
    o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-3) * radius
    d = torch.from_numpy(hash_uniform((n, 3), seed + 3)) * 1.5 - o
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-3) * (1.0 + 0.2 * torch.from_numpy(hash_uniform((n, 1), seed + 4)))
    if rng.integers(4) == 0:  # axis-parallel rays: zero direction components (the slab test divides by them: sample.py:71-184)
        zero = torch.from_numpy(hash_uniform((n, 3), seed + 7, 0.0, 1.0) < 0.3)
        zero[:, 0] &= ~(zero[:, 1] & zero[:, 2])  # (never all three)
        d = torch.where(zero, torch.zeros_like(d), d)
    near, far = float(rng.uniform(0.05, 2.0)), float(rng.uniform(4.0, 7.0))
    diffuse, opt, white, perturb = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
    t_rand = torch.from_numpy(hash_uniform((n, S), seed + 5, 0.0, 1.0)) if perturb else None
    target = torch.from_numpy(hash_uniform((n, 3), seed + 6, 0.0, 1.0))
    backward = str(rng.choice(["atomic", "binned"]))
    desc = f"rays dims={dims} deg={deg} mode={mode} storage={storage} n={n} S={S} diffuse={diffuse} opt={opt} white={white} perturb={perturb} backward={backward} near={near:.2f}"
    if mode == "identity":
        keep = identity_usable(dens, feat, o, d, orc.make_aabb(dims, voxel, loc), near, far, S, rho, white, diffuse, opt, t_rand)
        if not bool(keep.any()):
            return desc + " (no usable ray)"
        o, d, target = o[keep].contiguous(), d[keep].contiguous(), target[keep].contiguous()
        t_rand = None if t_rand is None else t_rand[keep].contiguous()
        n = len(o)
    grid = make_grid(dev, dens, feat, voxel, loc, mode, rho, storage, True)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=perturb, optimized_sampling=opt, white_bkgd=white, render_diffuse=diffuse)
    from thr3ed_atom_amd import ops

    ops.AUTOGRAD_BACKWARD = backward
    try:
        out = rf.render_sh_voxel_grid(grid, rf.Rays(o.to(dev), d.to(dev)), cfg, None, t_rand=None if t_rand is None else t_rand.to(dev))
        loss = torch.nn.functional.l1_loss(out.colour, target.to(dev)) + 0.1 * out.depth.mean() + 0.05 * out.extra["accumulated_weight"].mean()
        loss.backward()
    finally:
        ops.AUTOGRAD_BACKWARD = "auto"
    dc, fc = dens.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    ref = orc.render(dc, fc, o, d, orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode, white_bkgd=white, render_diffuse=diffuse, optimized_sampling=opt, t_rand=t_rand)
    ref_loss = torch.nn.functional.l1_loss(ref["colour"], target) + 0.1 * ref["depth"].mean() + 0.05 * ref["acc"].mean()
    ref_loss.backward()
    cpu = lambda t: t.detach().cpu().numpy()
    # (depth is a sum of w z: its float32 noise scales with z, which AABB sampling measures in units of |d| -- short directions, long z)
    zmax = max(far, float(ref["depth"].detach().abs().max()))
    if LONG_RAYS:
        # thousands of samples: the float32 sums and products of the REFERENCE carry noise of the order of the bar itself, so the
        # float64-anchored rule of tests/test_hip_parity.py applies to every output: |hip - ref64| <= |ref32 - ref64| + bar
        r64 = orc.render(dens.double(), feat.double(), o.double(), d.double(), orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode, white_bkgd=white,
                         render_diffuse=diffuse, optimized_sampling=opt, t_rand=None if t_rand is None else t_rand.double())
        for name, ours, bar in (("colour", out.colour, TOL), ("depth", out.depth, 2 * TOL * max(1.0, zmax / 6.6)), ("acc", out.extra["accumulated_weight"], TOL)):
            # (the reference's float32 error of THIS batch as the noise scale: another summation order -- wave scans and chunk carries
            # instead of torch.cumprod's sequential product -- is another draw of the same noise, not the same draw)
            noise = float((ref[name].detach().double() - r64[name]).abs().max())
            worst = float((ours.detach().cpu().double() - r64[name]).abs().max())
            assert worst <= 3.0 * noise + bar, f"{desc}: {name} is {worst:.2e} from the float64 value; the float32 reference is {noise:.2e} from it"
    else:
        np.testing.assert_allclose(cpu(out.colour), ref["colour"].detach().numpy(), rtol=0, atol=TOL, err_msg=desc)
        np.testing.assert_allclose(cpu(out.depth), ref["depth"].detach().numpy(), rtol=0, atol=2 * TOL * max(1.0, zmax / 6.6), err_msg=desc)
        np.testing.assert_allclose(cpu(out.extra["accumulated_weight"]), ref["acc"].detach().numpy(), rtol=0, atol=TOL, err_msg=desc)
    # disparity = 1 / max(1e-10, depth / acc): NaN exactly where the reference's is (acc == 0), else the same quotient
    disp, disp_ref = cpu(out.extra["disparity"]).reshape(-1), ref["disparity"].detach().numpy().reshape(-1)
    assert np.array_equal(np.isnan(disp), np.isnan(disp_ref)), desc + ": NaN pattern of the disparity"
    # (compared where the quotient is not a ratio of rounding noise: acc > 1e-2 and depth / acc > 1e-3)
    firm = (~np.isnan(disp_ref)) & (ref["acc"].detach().numpy().reshape(-1) > 1e-2) & (np.nan_to_num(disp_ref, nan=np.inf) < 1e3)
    if firm.any() and not LONG_RAYS:
        np.testing.assert_allclose(disp[firm], disp_ref[firm], rtol=2e-3, atol=1e-6, err_msg=desc + " (disparity)")
    gd, gf = grid.reference_gradients()
    gd_ref, gf_ref = dc.grad.numpy(), fc.grad.numpy()
    np.testing.assert_allclose(cpu(gd), gd_ref, rtol=5e-4, atol=5e-6 * max(np.abs(gd_ref).max(), 1e-12), err_msg=desc)
    np.testing.assert_allclose(cpu(gf), gf_ref, rtol=5e-4, atol=5e-6 * max(np.abs(gf_ref).max(), 1e-12), err_msg=desc)
    return desc


def case_frames(rng, dev, seed):
    dims, deg, mode, storage, voxel, loc, rho = draw_common(rng)
    F = 3 * (deg + 1) ** 2
    dens, feat = draw_grid(dims, F, seed, mode)
    H, W = int(rng.integers(1, 50)), int(rng.integers(1, 50))
    focal = float(rng.choice([20.0, 60.0, 300.0, 900.0]))
    S = int(rng.choice([1, 5, 40, 64, 97]))
    if LONG_RAYS:
        H, W = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        S = int(rng.choice([256, 1000, 1024, 4096, 4100, 5000]))
    tiles = str(rng.choice(["0", "1"]))
    white, diffuse, opt = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
    occ = bool(rng.integers(2)) and mode == "relu"
    pose = rf.pose_spherical(float(rng.uniform(0, 360)), float(rng.uniform(-80, 10)), float(rng.uniform(2.5, 5.0)))
    near, far = float(rng.uniform(0.3, 2.0)), float(rng.uniform(5.5, 8.0))
    desc = f"frame dims={dims} deg={deg} mode={mode} storage={storage} HxW={H}x{W} focal={focal} S={S} tiles={tiles} white={white} diffuse={diffuse} opt={opt} occ={occ}"
    grid = make_grid(dev, dens, feat, voxel, loc, mode, rho, storage, False)
    intr = rf.CameraIntrinsics(H, W, focal)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=False, optimized_sampling=opt, white_bkgd=white, render_diffuse=diffuse,
                                   use_occupancy_mask=occ)
    if occ:
        grid.build_occupancy()
    os.environ["RF_FRAME_TILES"] = tiles
    try:
        frame = rf.render_sh_voxel_grid_frame(grid, intr, pose, cfg)
    finally:
        os.environ.pop("RF_FRAME_TILES", None)
    flat = rf.flatten_rays(rf.cast_rays(intr, pose, dev))
    rows = slice(None)  # (identity: the pixels whose rays are usable)
    if mode == "identity":
        rows = identity_usable(dens, feat, flat.origins.cpu(), flat.directions.cpu(), orc.make_aabb(dims, voxel, loc), near, far, S, rho, white, diffuse, opt)
        if not bool(rows.any()):
            return desc + " (no usable ray)"
    ref = orc.render(dens, feat, flat.origins.cpu(), flat.directions.cpu(), orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode, white_bkgd=white,
                     render_diffuse=diffuse, optimized_sampling=opt)
    if LONG_RAYS:  # the float64-anchored rule (see case_rays)
        r64 = orc.render(dens.double(), feat.double(), flat.origins.cpu().double(), flat.directions.cpu().double(), orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode,
                         white_bkgd=white, render_diffuse=diffuse, optimized_sampling=opt)
        for name, ours, bar in (("colour", frame.colour.reshape(-1, 3), TOL), ("depth", frame.depth.reshape(-1, 1), 2 * TOL * max(1.0, far / 6.6)),
                                ("acc", frame.extra["accumulated_weight"].reshape(-1, 1), TOL)):
            noise = float((ref[name].double() - r64[name])[rows].abs().max())
            worst = float((ours.cpu().double() - r64[name])[rows].abs().max())
            assert worst <= 3.0 * noise + bar, f"{desc}: {name} is {worst:.2e} from the float64 value; the float32 reference is {noise:.2e} from it"
        return desc
    err_c = float((frame.colour.reshape(-1, 3).cpu() - ref["colour"])[rows].abs().max())
    err_a = float((frame.extra["accumulated_weight"].reshape(-1, 1).cpu() - ref["acc"])[rows].abs().max())
    err_d = float((frame.depth.reshape(-1, 1).cpu() - ref["depth"])[rows].abs().max())
    assert err_c <= TOL and err_a <= TOL and err_d <= 2 * TOL * max(1.0, far / 6.6), f"{desc}: colour {err_c:.2e} acc {err_a:.2e} depth {err_d:.2e}"
    return desc


def case_train(rng, dev, seed):
    """Two training iterations (TrainStepper: fused or autograd-driven, either adjoint, either brick shape, Adam in the brick flush or
    from a gradient bucket) against the oracle's autograd + torch.optim.Adam on the same rays, pixels and jitter."""
    from thr3ed_atom_amd.trainers import TrainStepper

    dims = tuple(int(rng.integers(4, 21)) for _ in range(3))
    if BIG_GRIDS:  # many bricks per axis, partial bricks on every axis: the (brick, flags) key ranges of the binned adjoint
        dims = tuple(int(rng.integers(4, 73)) for _ in range(3))
    deg = int(rng.integers(0, 4))
    mode = str(rng.choice(["relu", "relu", "softplus", "abs"]))
    if FORCE_MODE:
        mode = FORCE_MODE
    storage = str(rng.choice(["reference", "split", "bricked"]))
    voxel = tuple(3.0 / d for d in dims)
    if mode == "identity":
        rho = float(rng.choice([2.0, 5.0]))
    else:
        rho = 1.0 if mode == "abs" else float(rng.choice([5.0, 100.0 / 3.0]))
    F = 3 * (deg + 1) ** 2
    dens, feat = draw_grid(dims, F, seed, mode)
    n = int(rng.choice([1, 3, 37, 64, 130, 257]))
    # (not fewer than 17 samples here: with 2 or 3 the 1e10-long last interval often lies inside the volume and the float32 forward
    # rounding of the REFERENCE itself shows as 1e-4 relative noise on small gradients -- tests/debug_train_case.py: HIP and the float32
    # oracle are equally far from the float64 oracle there -- which Adam's normalised update turns into parameter differences above the
    # allowance below; that regime is held to the gradient bar by the ray cases and golden G13)
    S = int(rng.choice([17, 33, 40, 64, 70]))
    if LONG_RAYS:  # (the adjoints' chunk-mask groups: 64 masks = 4096 samples)
        n = int(rng.choice([1, 3, 17, 40]))
        S = int(rng.choice([256, 1000, 4096, 4100, 4200]))
    fused = bool(rng.integers(2))
    backward = str(rng.choice(["atomic", "binned"]))
    fuse_opt = bool(rng.integers(2)) if (fused and backward == "binned") else None
    white, diffuse_reg = bool(rng.integers(2)), bool(rng.integers(2))
    if fuse_opt and (storage == "reference" or deg not in (0, 2) or not diffuse_reg):
        fuse_opt = False  # (Adam in the brick flush: the merged pass over both renders' lists, split / bricked storage, SH degree 0 or 2)
    perturb = fused  # (a jitter TABLE is taken by the fused step only; the autograd-driven step is compared without jitter)
    brick = None if not (fused and backward == "binned") else [None, 4, 8][int(rng.integers(3))]
    lr = 0.03
    desc = (f"train dims={dims} deg={deg} mode={mode} storage={storage} n={n} S={S} fused={fused} backward={backward} fuse_optimizer={fuse_opt} brick={brick} "
            f"white={white} diffuse_reg={diffuse_reg}")
    o = torch.from_numpy(hash_uniform((n, 3), seed + 1))
    o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-3) * 4.0
    d = torch.from_numpy(hash_uniform((n, 3), seed + 3)) * 1.2 - o
    d = d / d.norm(dim=-1, keepdim=True)
    pixels = torch.from_numpy(hash_uniform((n, 3), seed + 6, 0.0, 1.0))
    near, far = 1.8, 6.6
    if mode == "identity":  # (both renders of the step: specular and diffuse, jittered by tables drawn below)
        keep = identity_usable(dens, feat, o, d, orc.make_aabb(dims, voxel), near, far, S, rho, white, jitter_unknown=perturb)
        keep &= identity_usable(dens, feat, o, d, orc.make_aabb(dims, voxel), near, far, S, rho, white, diffuse=True, jitter_unknown=perturb)
        if not bool(keep.any()):
            return desc + " (no usable ray)"
        o, d, pixels = o[keep].contiguous(), d[keep].contiguous(), pixels[keep].contiguous()
        n = len(o)
    grid = make_grid(dev, dens, feat, voxel, (0.0, 0.0, 0.0), mode, rho, storage, True)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=perturb, white_bkgd=white)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    kw = dict(fused=fused, backward=backward, apply_diffuse_render_regularization=diffuse_reg, data_parallel=False)
    if fuse_opt is not None:
        kw["fuse_optimizer"] = fuse_opt
    if brick is not None:
        kw["brick_size"] = brick
    stepper = TrainStepper(model, n, learning_rate=lr, **kw)
    cd, cf = dens.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [cd, cf], "lr": lr}], betas=(0.9, 0.999))
    aabb = orc.make_aabb(dims, voxel)
    rays = rf.Rays(o.to(dev), d.to(dev))
    firm, grads = None, []
    for it in range(2):
        t_rands = [torch.from_numpy(hash_uniform((n, S), seed + 10 + 2 * it + i, 0.0, 1.0)).clamp_(0.0, 1.0 - 2.0**-24) for i in range(2)]
        stats = stepper.step_on(rays, pixels.to(dev), t_rand=[t.to(dev) for t in t_rands] if perturb else None)
        opt.zero_grad()
        losses = []
        for k, diffuse in enumerate((False, True) if diffuse_reg else (False,)):
            out = orc.render(cd, cf, o, d, aabb, near, far, S, rho, mode, white_bkgd=white, render_diffuse=diffuse, t_rand=t_rands[k] if perturb else None)
            losses.append(torch.nn.functional.l1_loss(out["colour"], pixels))
        sum(losses).backward()
        np.testing.assert_allclose(float(stats.specular_loss), losses[0].item(), rtol=5e-5, atol=1e-7, err_msg=desc + f" it={it}")
        if diffuse_reg:
            np.testing.assert_allclose(float(stats.diffuse_loss), losses[1].item(), rtol=5e-5, atol=1e-7, err_msg=desc + f" it={it}")
        g_now = torch.cat([cd.grad.reshape(-1), cf.grad.reshape(-1)]).clone()
        grads.append(g_now)
        firm_now = g_now.abs() > max(1e-6, 1e-3 * float(g_now.abs().max()))
        firm = firm_now if firm is None else (firm & firm_now)
        opt.step()
    torch.cuda.synchronize()
    ours = torch.cat([grid.densities.detach().reshape(-1), grid.features.detach().reshape(-1)]).cpu()
    ref = torch.cat([cd.detach().reshape(-1), cf.detach().reshape(-1)])
    err = (ours - ref).abs()
    # Adam normalises the step: a parameter whose gradient is summation noise may move by a whole update in the other direction; every
    # parameter with a firm gradient in both iterations must agree tightly (the criterion of test_bench_train_step_against_oracle_...).
    # "Tightly" scales with the conditioning of the second update's first moment, 0.09 g1 + 0.1 g2: where the two iterations' gradients
    # nearly cancel, float32 summation-order noise of the gradients (taken as 3e-4 relative, atomics included) is amplified by
    # cond = (0.09 |g1| + 0.1 |g2|) / |0.09 g1 + 0.1 g2|
    assert float(err.max()) <= 2 * 2 * lr + 1e-6, f"{desc}: max parameter error {float(err.max()):.3e}"
    num = 0.09 * grads[0].abs() + 0.1 * grads[1].abs()
    cond = num / (0.09 * grads[0] + 0.1 * grads[1]).abs().clamp_min(1e-30)
    allowed = (2e-5 + lr * 3e-4 * cond).clamp_max(2 * lr)
    # ... for all but a handful of them: a sample within ~1e-6 of the ReLU kink (or of the box faces) falls on the other side once the
    # two parameter sets differ by the first iteration's rounding, which changes the gradients of its 8 corners discontinuously -- the
    # reference trainer's own run-to-run behaviour (docs/experiments.md C); a systematic error shows on whole fractions of the grid
    if int(firm.sum()) >= 200:  # (a handful of rays leaves a handful of firm gradients: too few for a fraction; the bounds above and below still hold)
        inside = (err[firm] <= allowed[firm]).float().mean()
        assert float(inside) >= 0.995, f"{desc}: only {float(inside):.4f} of the {int(firm.sum())} firm-gradient parameters within the allowance (max error {float(err[firm].max()):.3e})"
    assert float((err <= 5e-5).float().mean()) >= 0.97, f"{desc}: only {float((err <= 5e-5).float().mean()):.4f} of the parameters within 5e-5"
    return desc


def case_misc(rng, dev, seed):
    """The smaller entry points in random set-ups: point queries (+ adjoint), the stage transition, the keyed batch selection, frames cut
    into pixel ranges with the in-kernel jitter."""
    from thr3ed_atom_amd import ops

    what = str(rng.choice(["query", "upsample", "select", "ranges"]))
    dims, deg, mode, storage, voxel, loc, rho = draw_common(rng)
    F = 3 * (deg + 1) ** 2
    if what == "query":
        dens, feat = draw_grid(dims, F, seed, mode)
        m = int(rng.integers(1, 3000))
        lo = np.array([l - 0.5 * v * d_ for l, v, d_ in zip(loc, voxel, dims)], dtype=np.float32)
        hi = np.array([l + 0.5 * v * d_ for l, v, d_ in zip(loc, voxel, dims)], dtype=np.float32)
        u = hash_uniform((m, 3), seed + 1, -0.2, 1.2)  # in, out and (below) on the faces of the box
        pts = lo + (hi - lo) * u
        face = hash_uniform((m,), seed + 2, 0.0, 1.0) < 0.15
        axis = (hash_uniform((m,), seed + 3, 0.0, 3.0)).astype(np.int64).clip(0, 2)
        side = hash_uniform((m,), seed + 4, 0.0, 1.0) < 0.5
        eps = hash_uniform((m,), seed + 5, -1e-4, 1e-4)
        rows = np.nonzero(face)[0]
        pts[rows, axis[rows]] = np.where(side[rows], lo[axis[rows]], hi[axis[rows]]) + eps[rows]
        pts = torch.from_numpy(pts.astype(np.float32))
        desc = f"query dims={dims} deg={deg} mode={mode} storage={storage} points={m}"
        grid = make_grid(dev, dens, feat, voxel, loc, mode, rho, storage, True)
        out = grid(pts.to(dev))
        gout = torch.from_numpy(hash_uniform((m, F + 1), seed + 6))
        (out * gout.to(dev)).sum().backward()
        cd, cf = dens.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        aabb = orc.make_aabb(dims, voxel, loc)
        ref = orc.voxel_grid_forward(cd, cf, pts, aabb, rho, mode)
        (ref * gout).sum().backward()
        o_, r_ = out.detach().cpu().numpy(), ref.detach().numpy()
        assert np.array_equal(o_[:, :F], r_[:, :F]), desc + ": interpolated features are not bit-identical"
        if mode == "softplus":
            np.testing.assert_allclose(o_[:, F], r_[:, F], rtol=2e-6, atol=1e-7, err_msg=desc)
        else:
            assert np.array_equal(o_[:, F], r_[:, F]), desc + ": densities are not bit-identical"
        assert np.array_equal(grid.test_inside_volume(pts.to(dev)).cpu().numpy().reshape(-1), orc.inside_aabb(pts, aabb).numpy().reshape(-1)), desc
        gd, gf = grid.reference_gradients()
        for ours, refg in ((gd, cd.grad), (gf, cf.grad)):
            np.testing.assert_allclose(ours.detach().cpu().numpy(), refg.numpy(), rtol=1e-4, atol=1e-5 * max(float(refg.abs().max()), 1e-12), err_msg=desc)
        return desc
    if what == "upsample":
        src = tuple(int(rng.integers(2, 13)) for _ in range(3))
        dst = tuple(int(rng.integers(2, 31)) for _ in range(3))
        dens, feat = procedural_grid(src, F, seed % 100000)
        desc = f"upsample {src} -> {dst} deg={deg} storage={storage}"
        grid = make_grid(dev, dens, feat, tuple(3.0 / d_ for d_ in src), (0.0, 0.0, 0.0), "relu", 3.0, storage, False)
        up = rf.scale_voxel_grid_with_required_output_size(grid, dst)
        ref = torch.from_numpy(orc.trilinear_upsample_recipe(torch.cat([feat, dens], dim=-1).numpy(), dst, vector_width=8))
        assert up.grid_dims == tuple(dst) and up.storage == storage, desc
        assert torch.equal(up.features.detach().cpu(), ref[..., :-1]) and torch.equal(up.densities.detach().cpu(), ref[..., -1:]), desc + ": not bit-identical"
        return desc
    if what == "select":
        H, W, M = int(rng.integers(1, 60)), int(rng.integers(1, 60)), int(rng.integers(1, 7))
        nsel = int(rng.integers(1, M + 1))
        ids = torch.from_numpy(rng.choice(M, nsel, replace=False).astype(np.int64))
        P = nsel * H * W
        n = int(rng.integers(1, P + 1))
        first = int(rng.integers(0, P - n + 1))
        key = int(rng.integers(0, 2**63 - 1)) * 2 + int(rng.integers(0, 2))
        focal = float(rng.uniform(10.0, 900.0))
        poses = torch.stack([torch.cat([p.rotation, p.translation], dim=1) for p in
                             (rf.pose_spherical(float(rng.uniform(0, 360)), float(rng.uniform(-80, 10)), 4.0) for _ in range(M))]).to(dev)
        table = torch.from_numpy(hash_uniform((M * H * W, 3), seed + 1, 0.0, 1.0)).to(dev)
        desc = f"select HxW={H}x{W} images={nsel}/{M} n={n} first={first}"
        o, d, px, idx = ops.select_rays_and_pixels_hip(H, W, focal, poses, ids, table, n, key, return_index=True, first_index=first)
        want = orc.keyed_permutation(np.arange(first, first + n), P, key)
        assert np.array_equal(idx.cpu().numpy(), want), desc + ": indices differ from the restated bijection"
        assert len(np.unique(want)) == n, desc
        hw = H * W
        img = ids.to(dev)[idx // hw]
        assert torch.equal(px, table[img * hw + idx % hw]), desc + ": pixels"
        ro, rd = ops.cast_selected_rays_hip(H, W, focal, poses[ids.to(dev)], idx)
        assert torch.equal(o, ro) and torch.equal(d, rd), desc + ": rays"
        return desc
    # "ranges": a frame with the in-kernel (keyed) jitter, whole and cut into three pixel ranges, either kernel; and against the oracle
    # fed with the restated jitter table
    dens, feat = procedural_grid(dims, F, seed % 100000)
    H, W = int(rng.integers(1, 45)), int(rng.integers(1, 45))
    focal = float(rng.choice([30.0, 80.0, 400.0]))
    S = int(rng.choice([3, 33, 64, 80]))
    tiles = str(rng.choice(["0", "1"]))
    pose = rf.pose_spherical(float(rng.uniform(0, 360)), float(rng.uniform(-80, 10)), float(rng.uniform(3.0, 5.0)))
    near, far = 1.0, 7.0
    desc = f"ranges dims={dims} deg={deg} mode={mode} storage={storage} HxW={H}x{W} focal={focal} S={S} tiles={tiles}"
    grid = make_grid(dev, dens, feat, voxel, loc, mode, rho, storage, False)
    intr = rf.CameraIntrinsics(H, W, focal)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=True, white_bkgd=True)
    n = H * W
    cuts = sorted(int(c) for c in rng.integers(0, n + 1, size=2))
    os.environ["RF_FRAME_TILES"] = tiles
    try:
        torch.manual_seed(seed % 2**31)
        key = ops.draw_jitter_key()
        torch.manual_seed(seed % 2**31)
        whole = rf.render_sh_voxel_grid_frame(grid, intr, pose, cfg)
        parts = []
        for a_, b_ in ((0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], n)):
            if b_ > a_:
                torch.manual_seed(seed % 2**31)
                parts.append(rf.render_sh_voxel_grid_frame(grid, intr, pose, cfg, first_ray=a_, num_rays=b_ - a_))
    finally:
        os.environ.pop("RF_FRAME_TILES", None)
    for name in ("colour", "depth"):
        cat = torch.cat([getattr(p, name).reshape(-1, getattr(p, name).shape[-1]) for p in parts])
        assert torch.equal(cat, getattr(whole, name).reshape(cat.shape)), desc + f": {name} depends on how the frame is cut ({cuts})"
    flat = rf.flatten_rays(rf.cast_rays(intr, pose, dev))
    table = torch.from_numpy(orc.keyed_jitter(key, 0, n, S))
    ref = orc.render(dens, feat, flat.origins.cpu(), flat.directions.cpu(), orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode, white_bkgd=True, t_rand=table)
    err_c = float((whole.colour.reshape(-1, 3).cpu() - ref["colour"]).abs().max())
    err_d = float((whole.depth.reshape(-1, 1).cpu() - ref["depth"]).abs().max())
    assert err_c <= TOL and err_d <= 2.5 * TOL, f"{desc}: colour {err_c:.2e} depth {err_d:.2e}"
    return desc


def _renamed_occupancy(densities, deltas):  # the default law under another name: un-fusable, so the render is COMPOSED
    return 1.0 - torch.exp(-(densities * deltas))


def case_composed(rng, dev, seed):
    """render_sh_voxel_grid with callables the fused kernels do not recognise (the default laws, re-stated): the composed path --
    rf_grid_query in the middle of torch ops, through autograd -- against the oracle, forward and gradients."""
    from thr3ed_atom_amd.renderers import fused_kernels_apply

    dims, deg, mode, storage, voxel, loc, rho = draw_common(rng)
    F = 3 * (deg + 1) ** 2
    dens, feat = procedural_grid(dims, F, seed % 100000)
    n = int(rng.integers(1, 300))
    S = int(rng.choice([2, 3, 17, 40, 64, 65, 128]))
    if LONG_RAYS:
        n = int(rng.integers(1, 24))
        S = int(rng.choice([256, 1000, 1024, 4096, 5000]))
    o = torch.from_numpy(hash_uniform((n, 3), seed + 1))
    o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-3) * torch.from_numpy(hash_uniform((n, 1), seed + 2, 0.2, 5.0))
    d = torch.from_numpy(hash_uniform((n, 3), seed + 3)) * 1.5 - o
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-3) * (1.0 + 0.2 * torch.from_numpy(hash_uniform((n, 1), seed + 4)))
    near, far = float(rng.uniform(0.05, 2.0)), float(rng.uniform(4.0, 7.0))
    diffuse, opt, white, perturb = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
    which = int(rng.integers(1, 4))  # bit 0: occupancy law renamed, bit 1: tone map re-stated
    t_rand = torch.from_numpy(hash_uniform((n, S), seed + 5, 0.0, 1.0)) if perturb else None
    target = torch.from_numpy(hash_uniform((n, 3), seed + 6, 0.0, 1.0))
    desc = f"composed dims={dims} deg={deg} mode={mode} storage={storage} n={n} S={S} diffuse={diffuse} opt={opt} white={white} perturb={perturb} callables={which}"
    grid = make_grid(dev, dens, feat, voxel, loc, mode, rho, storage, True)
    kw = {}
    if which & 1:
        kw["density2occupancy"] = _renamed_occupancy
    if which & 2:
        kw["radiance_hdr_tone_map"] = lambda x: torch.sigmoid(x)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=perturb, optimized_sampling=opt, white_bkgd=white, render_diffuse=diffuse, **kw)
    assert not fused_kernels_apply(grid, cfg), desc
    out = rf.render_sh_voxel_grid(grid, rf.Rays(o.to(dev), d.to(dev)), cfg, None, t_rand=None if t_rand is None else t_rand.to(dev))
    loss = torch.nn.functional.l1_loss(out.colour, target.to(dev)) + 0.1 * out.depth.mean() + 0.05 * out.extra["accumulated_weight"].mean()
    loss.backward()
    dc, fc = dens.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    ref = orc.render(dc, fc, o, d, orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode, white_bkgd=white, render_diffuse=diffuse, optimized_sampling=opt, t_rand=t_rand)
    ref_loss = torch.nn.functional.l1_loss(ref["colour"], target) + 0.1 * ref["depth"].mean() + 0.05 * ref["acc"].mean()
    ref_loss.backward()
    cpu = lambda t: t.detach().cpu().numpy()
    zmax = max(far, float(ref["depth"].detach().abs().max()))
    if LONG_RAYS:  # the float64-anchored rule (see case_rays)
        r64 = orc.render(dens.double(), feat.double(), o.double(), d.double(), orc.make_aabb(dims, voxel, loc), near, far, S, rho, mode, white_bkgd=white,
                         render_diffuse=diffuse, optimized_sampling=opt, t_rand=None if t_rand is None else t_rand.double())
        for name, ours, bar in (("colour", out.colour, TOL), ("depth", out.depth, 2 * TOL * max(1.0, zmax / 6.6)), ("acc", out.extra["accumulated_weight"], TOL)):
            noise = float((ref[name].detach().double() - r64[name]).abs().max())
            worst = float((ours.detach().cpu().double() - r64[name]).abs().max())
            assert worst <= 3.0 * noise + bar, f"{desc}: {name} is {worst:.2e} from the float64 value; the float32 reference is {noise:.2e} from it"
    else:
        np.testing.assert_allclose(cpu(out.colour), ref["colour"].detach().numpy(), rtol=0, atol=TOL, err_msg=desc)
        np.testing.assert_allclose(cpu(out.depth), ref["depth"].detach().numpy(), rtol=0, atol=2 * TOL * max(1.0, zmax / 6.6), err_msg=desc)
        np.testing.assert_allclose(cpu(out.extra["accumulated_weight"]), ref["acc"].detach().numpy(), rtol=0, atol=TOL, err_msg=desc)
    gd, gf = grid.reference_gradients()
    gd_ref, gf_ref = dc.grad.numpy(), fc.grad.numpy()
    np.testing.assert_allclose(cpu(gd), gd_ref, rtol=5e-4, atol=5e-6 * max(np.abs(gd_ref).max(), 1e-12), err_msg=desc)
    np.testing.assert_allclose(cpu(gf), gf_ref, rtol=5e-4, atol=5e-6 * max(np.abs(gf_ref).max(), 1e-12), err_msg=desc)
    return desc


class ReferenceLikeGrid(torch.nn.Module):
    """A module with exactly the attributes the reference's VoxelGrid has (thre3d_reprs/voxels.py:93-124) and none of this package's:
    what `VolumetricModel(thre3d_repr=<reference grid>, ...)` hands to a render procedure."""

    def __init__(self, densities, features, voxel_size, location, pre, post, rho):
        super().__init__()
        self._densities = torch.nn.Parameter(densities)
        self._features = torch.nn.Parameter(features)
        self._density_preactivation, self._density_postactivation = pre, post
        self._feature_preactivation = self._feature_postactivation = torch.nn.Identity()
        self._radiance_transfer_function = None
        self._grid_location, self._voxel_size, self._expected_density_scale, self._tunable = location, voxel_size, rho, True
        self.width_x, self.depth_y, self.height_z = densities.shape[:3]
        half = [n_ * v / 2 for n_, v in zip(densities.shape[:3], voxel_size)]
        self._aabb = tuple((c - h, c + h) for c, h in zip(location, half))

    densities = property(lambda self: self._densities)
    features = property(lambda self: self._features)
    aabb = property(lambda self: self._aabb)


_BINDING = {}


def load_binding(backward: str):
    """integration/renderers_hip.py (the file a maintainer adds to the reference) imported against stand-ins for the three reference
    names it needs -- the reference itself does not exist on the GPU box --, one instance per adjoint policy (read at import)."""
    import importlib.util
    import types

    from thr3ed_atom_amd import _lib, constants

    if backward in _BINDING:
        return _BINDING[backward]
    names = ["thre3d_atom", "thre3d_atom.rendering", "thre3d_atom.rendering.volumetric", "thre3d_atom.rendering.volumetric.render_interface", "thre3d_atom.utils",
             "thre3d_atom.utils.constants"]
    saved = {n_: sys.modules.get(n_) for n_ in names}
    mods = {n_: types.ModuleType(n_) for n_ in names}
    mods["thre3d_atom.rendering.volumetric.render_interface"].Rays = rf.Rays
    mods["thre3d_atom.rendering.volumetric.render_interface"].RenderOut = rf.RenderOut
    mods["thre3d_atom.utils.constants"].EXTRA_DISPARITY = constants.EXTRA_DISPARITY
    mods["thre3d_atom.utils.constants"].EXTRA_ACCUMULATED_WEIGHTS = constants.EXTRA_ACCUMULATED_WEIGHTS
    env = {k: os.environ.get(k) for k in ("RELU_FIELD_HIP_LIB", "RELU_FIELD_HIP_BACKWARD", "RELU_FIELD_HIP_MIN_BRICKS")}
    os.environ.update(RELU_FIELD_HIP_LIB=_lib.LIB_PATH, RELU_FIELD_HIP_BACKWARD=backward, RELU_FIELD_HIP_MIN_BRICKS="0")
    sys.modules.update(mods)
    try:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration", "renderers_hip.py")
        spec = importlib.util.spec_from_file_location(f"renderers_hip_fuzz_{backward}", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n_, m in saved.items():
            if m is None:
                sys.modules.pop(n_, None)
            else:
                sys.modules[n_] = m
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _BINDING[backward] = mod
    return mod


def case_binding(rng, dev, seed):
    """The reference-side binding (integration/renderers_hip.py) on a module with the reference VoxelGrid's attributes: the single
    procedure, the pair procedure and the frame entry, against the oracle."""
    dims, deg, mode, storage, voxel, loc, rho = draw_common(rng)
    F = 3 * (deg + 1) ** 2
    dens, feat = draw_grid(dims, F, seed, mode)
    backward = str(rng.choice(["atomic", "binned"]))
    rh = load_binding(backward)
    what = str(rng.choice(["single", "pair", "frame"]))
    S = int(rng.choice([2, 3, 17, 40, 64, 65, 128]))
    near, far = float(rng.uniform(0.05, 2.0)), float(rng.uniform(4.0, 7.0))
    opt, white = bool(rng.integers(2)), bool(rng.integers(2))
    grid = ReferenceLikeGrid(dens.to(dev), feat.to(dev), voxel, loc, ACTS[mode][0], ACTS[mode][1], rho).to(dev)
    aabb = orc.make_aabb(dims, voxel, loc)
    desc = f"binding[{what}] dims={dims} deg={deg} mode={mode} S={S} opt={opt} white={white} backward={backward}"
    cpu = lambda t: t.detach().cpu().numpy()
    if what == "frame":
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        focal = float(rng.choice([30.0, 80.0, 400.0]))
        diffuse = bool(rng.integers(2))
        pose = rf.pose_spherical(float(rng.uniform(0, 360)), float(rng.uniform(-80, 10)), float(rng.uniform(3.0, 5.0)))
        intr = rf.CameraIntrinsics(H, W, focal)
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=False, optimized_sampling=opt, white_bkgd=white, render_diffuse=diffuse)
        out = rh.render_frame_hip(grid, intr, pose, cfg)
        flat = rf.flatten_rays(rf.cast_rays(intr, pose, dev))
        rows = slice(None)  # (identity: the pixels whose rays are usable)
        if mode == "identity":
            rows = identity_usable(dens, feat, flat.origins.cpu(), flat.directions.cpu(), aabb, near, far, S, rho, white, diffuse, opt)
            if not bool(rows.any()):
                return desc + " (no usable ray)"
        ref = orc.render(dens, feat, flat.origins.cpu(), flat.directions.cpu(), aabb, near, far, S, rho, mode, white_bkgd=white, render_diffuse=diffuse, optimized_sampling=opt)
        err_c = float((out.colour.reshape(-1, 3).cpu() - ref["colour"])[rows].abs().max())
        err_d = float((out.depth.reshape(-1, 1).cpu() - ref["depth"])[rows].abs().max())
        assert err_c <= TOL and err_d <= 2 * TOL * max(1.0, far / 6.6), f"{desc} HxW={H}x{W}: colour {err_c:.2e} depth {err_d:.2e}"
        return desc
    n = int(rng.integers(1, 300))
    o = torch.from_numpy(hash_uniform((n, 3), seed + 1))
    o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-3) * torch.from_numpy(hash_uniform((n, 1), seed + 2, 0.2, 5.0))
    d = torch.from_numpy(hash_uniform((n, 3), seed + 3)) * 1.5 - o
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-3) * (1.0 + 0.2 * torch.from_numpy(hash_uniform((n, 1), seed + 4)))
    target = torch.from_numpy(hash_uniform((n, 3), seed + 6, 0.0, 1.0))
    if mode == "identity":  # (the pair procedure renders specular and diffuse)
        keep = identity_usable(dens, feat, o, d, aabb, near, far, S, rho, white, opt=opt)
        keep &= identity_usable(dens, feat, o, d, aabb, near, far, S, rho, white, diffuse=True, opt=opt)
        if not bool(keep.any()):
            return desc + " (no usable ray)"
        o, d, target = o[keep].contiguous(), d[keep].contiguous(), target[keep].contiguous()
        n = len(o)
    rays = rf.Rays(o.to(dev), d.to(dev))
    dc, fc = dens.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    if what == "single":
        diffuse = bool(rng.integers(2))
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=False, optimized_sampling=opt, white_bkgd=white, render_diffuse=diffuse)
        outs = [rh.render_sh_voxel_grid_hip(grid, rays, cfg)]
        refs = [orc.render(dc, fc, o, d, aabb, near, far, S, rho, mode, white_bkgd=white, render_diffuse=diffuse, optimized_sampling=opt)]
    else:
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=False, optimized_sampling=opt, white_bkgd=white)
        outs = list(rh.render_sh_voxel_grid_pair_hip(grid, rays, cfg))
        refs = [orc.render(dc, fc, o, d, aabb, near, far, S, rho, mode, white_bkgd=white, render_diffuse=df, optimized_sampling=opt) for df in (False, True)]
    # (the pair procedure back-propagates the two colours only -- the trainer's use -- and says so when anything else carries a gradient)
    if what == "single":
        (torch.nn.functional.l1_loss(outs[0].colour, target.to(dev)) + 0.1 * outs[0].depth.mean()).backward()
        (torch.nn.functional.l1_loss(refs[0]["colour"], target) + 0.1 * refs[0]["depth"].mean()).backward()
    else:
        sum(torch.nn.functional.l1_loss(x.colour, target.to(dev)) for x in outs).backward()
        sum(torch.nn.functional.l1_loss(r_["colour"], target) for r_ in refs).backward()
    for x, r_ in zip(outs, refs):
        zmax = max(far, float(r_["depth"].detach().abs().max()))
        np.testing.assert_allclose(cpu(x.colour), r_["colour"].detach().numpy(), rtol=0, atol=TOL, err_msg=desc)
        np.testing.assert_allclose(cpu(x.depth), r_["depth"].detach().numpy(), rtol=0, atol=2 * TOL * max(1.0, zmax / 6.6), err_msg=desc)
    for ours, refg in ((grid.densities.grad, dc.grad), (grid.features.grad, fc.grad)):
        assert ours is not None, desc + ": no gradient arrived at the module's Parameters"
        np.testing.assert_allclose(cpu(ours), refg.numpy(), rtol=5e-4, atol=5e-6 * max(float(refg.abs().max()), 1e-12), err_msg=desc)
    return desc


def case_seed(run_seed: int, i: int) -> int:
    return run_seed * 1000003 + i * 7919


def run_case(run_seed: int, i: int, kind: str, dev, mode: str = "") -> str:
    """case i of the run: its description; raises AssertionError on a parity miss (kind "long" = ray cases with 255..5000 samples)"""
    global FORCE_MODE, LONG_RAYS, BIG_GRIDS
    FORCE_MODE = mode
    BIG_GRIDS = kind == "bigtrain"
    if BIG_GRIDS:
        kind = "train"
    LONG_RAYS = kind in ("long", "longframes", "longtrain", "longcomposed")
    if LONG_RAYS:
        kind = {"long": "rays", "longframes": "frames", "longtrain": "train", "longcomposed": "composed"}[kind]
    seed = case_seed(run_seed, i)
    rng = np.random.default_rng(seed)
    if kind == "all":
        kind = "rays" if i % 2 == 0 else "frames"
    try:
        return {"rays": case_rays, "frames": case_frames, "train": case_train, "misc": case_misc, "composed": case_composed, "binding": case_binding}[kind](rng, dev, seed)
    finally:
        FORCE_MODE = ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kind", default="all")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated case indices (re-run failures)")
    ap.add_argument("--mode", default="", help="restrict the density mode (relu / softplus / abs / identity)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fails = 0
    only = {int(x) for x in a.only.split(",") if x}
    for i in range(a.cases):
        if only and i not in only:
            continue
        try:
            desc = run_case(a.seed, i, a.kind, dev, a.mode)
            if a.verbose:
                print("ok  ", i, desc, flush=True)
        except Exception as e:  # noqa: BLE001
            fails += 1
            print(f"FAIL case {i} seed {case_seed(a.seed, i)} kind {a.kind}: {type(e).__name__}: {str(e)[:1500]}", flush=True)
            if not isinstance(e, AssertionError):
                traceback.print_exc()
    print(f"fuzz_parity: {a.cases - fails} / {a.cases} cases passed (seed {a.seed}, kind {a.kind})")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
