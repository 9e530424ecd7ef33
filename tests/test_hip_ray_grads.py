"""Gradients of renders with respect to rays, points and camera poses (rf_render_backward_rays, rf_grid_query_backward_points,
the pose Function of cast_rays) against torch.autograd through the oracle.  Needs a real MI355X: every test is marked ``gpu``.

Bar (the project's H1 rule scaled for gradients), per component and batch:
    |hip - ref64| <= |ref32 - ref64| + C_GRAD * max |ref64| + ABS_FLOOR
The measured margin (largest |hip - ref64| - |ref32 - ref64| over max |ref64|) is printed by every comparison; it was at most a few
1e-7 of the batch maximum on the MI355X.  A batch whose gradient vanishes analytically (dL/d(acc) alone, of rays whose last sample is
opaque: ~1e-16 in float64) is judged against the scale of the same rays' mixed-loss gradient instead (floor_scale): the float32 sums
of terms of that order leave a residue of ~1e-6 there, in the kernel as in the float32 reference.
"""
import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from thr3ed_atom_amd import ops
from oracle import relu_field_oracle as orc
from tests.helpers import hash_uniform, hotdog_like_camera, procedural_grid, sparse_scene_grid

pytestmark = pytest.mark.gpu

C_GRAD = 1e-4

ACTS = {
    "relu": (torch.nn.Identity(), torch.nn.ReLU()),
    "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
    "abs": (torch.abs, torch.nn.Identity()),
    "identity": (torch.nn.Identity(), torch.nn.Identity()),
}


def make_grid(dev, dens, feat, voxel, storage, mode="relu", rho=1.0, tunable=False):
    pre, post = ACTS[mode]
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*voxel), density_preactivation=pre, density_postactivation=post,
                        expected_density_scale=rho, tunable=tunable, storage=storage)


def near_far():
    cam = hotdog_like_camera()
    return float(np.float32(cam["near"])), float(np.float32(cam["far"]))


def make_rays(n, seed, half):
    """Rays of every kind: through the box from a camera sphere (non-unit lengths), grazing, missing, starting inside, and with a
    zero direction component."""
    u = hash_uniform((n, 8), seed, -1.0, 1.0).astype(np.float64)
    o = np.empty((n, 3))
    d = np.empty((n, 3))
    for i in range(n):
        cam = u[i, :3] / (np.linalg.norm(u[i, :3]) + 1e-3) * 4.0
        kind = i % 6
        tgt = u[i, 3:6] * half * (0.6 if kind != 1 else 1.0)
        if kind == 1:  # grazing: aim at a point just outside a face
            tgt[0] = np.sign(tgt[0] + 1e-3) * half[0] * 1.02
        if kind == 2:  # missing
            tgt = tgt + 3.0 * np.sign(u[i, 6] + 1e-3) * half
        o[i] = cam
        if kind == 3:  # starting inside the box
            o[i] = u[i, 3:6] * half * 0.5
            tgt = o[i] + u[i, :3]
        d[i] = tgt - o[i]
        if kind == 4:  # a zero direction component (origin inside that slab)
            o[i, 2] = 0.3 * half[2] * u[i, 7]
            d[i, 2] = 0.0
        d[i] = d[i] / np.linalg.norm(d[i]) * (0.5 + 1.5 * abs(u[i, 7]))  # non-unit lengths
    return torch.from_numpy(o.astype(np.float32)), torch.from_numpy(d.astype(np.float32))


def check(name, hip, r32, r64, floor_scale=0.0):
    hip, r32, r64 = (t.detach().cpu().to(torch.float64) for t in (hip, r32, r64))
    scale = max(r64.abs().max().item(), floor_scale)
    excess = ((hip - r64).abs() - (r32 - r64).abs()).max().item()
    print(f"{name}: max|ref64| {scale:.3e}, max|hip-ref64| {(hip - r64).abs().max().item():.3e}, margin {excess / max(scale, 1e-30):.2e} of max")
    assert torch.isfinite(hip).all(), name
    assert ((hip - r64).abs() <= (r32 - r64).abs() + C_GRAD * scale).all(), f"{name}: excess {excess:.3e} (scale {scale:.3e})"


def oracle_ray_grads(dens, feat, o, d, aabb, near, far, S, rho, mode, white, diffuse, aabb_sampling, t_rand, weights, dtype):
    oo = o.to(dtype).clone().requires_grad_(True)
    dd = d.to(dtype).clone().requires_grad_(True)
    out = orc.render(dens.to(dtype), feat.to(dtype), oo, dd, aabb, near, far, S, rho, mode, white_bkgd=white, render_diffuse=diffuse,
                     optimized_sampling=aabb_sampling, t_rand=t_rand)
    wc, wd, wa = (w.to(dtype) for w in weights)
    loss = (out["colour"] * wc).sum() + (out["depth"] * wd).sum() + (out["acc"] * wa).sum()
    loss.backward()
    return oo.grad, dd.grad


def hip_ray_grads(grid, o, d, S, near, far, t_rand, white, diffuse, aabb_sampling, occ, weights, dev, dtype=torch.float32):
    oo = o.to(dev, dtype).clone().requires_grad_(True)
    dd = d.to(dev, dtype).clone().requires_grad_(True)
    colour, depth, acc, _ = ops.relu_field_render(grid, oo, dd, S, near, far, t_rand=t_rand, white_bkgd=white, render_diffuse=diffuse,
                                                  optimized_sampling=aabb_sampling, use_occupancy=occ)
    wc, wd, wa = (w.to(dev) for w in weights)
    loss = (colour * wc).sum() + (depth * wd).sum() + (acc * wa).sum()
    loss.backward()
    assert oo.grad.dtype == dtype and dd.grad.dtype == dtype and oo.grad.shape == o.shape
    return oo.grad, dd.grad


# (K, diffuse, mode, white, aabb, jitter, occupancy, S, dims, rho)
CASES = [
    (9, False, "relu", True, False, None, False, 48, (10, 12, 9), 5.0),
    (9, False, "relu", False, True, None, False, 48, (10, 12, 9), 5.0),
    (1, False, "softplus", True, True, "table", False, 40, (8, 8, 8), 2.0),
    (4, False, "abs", False, True, "keyed", False, 40, (9, 7, 8), 3.0),
    (16, False, "identity", True, False, "keyed", False, 36, (8, 8, 8), 0.5),
    (16, False, "relu", False, True, "table", False, 36, (8, 9, 10), 5.0),
    (9, True, "softplus", False, True, None, False, 40, (8, 8, 8), 2.0),
    (4, False, "relu", True, True, None, True, 64, (12, 12, 12), 8.0),
    (9, False, "abs", True, True, None, False, 1, (8, 8, 8), 3.0),
    (9, False, "relu", False, True, "keyed", False, 130, (8, 8, 8), 3.0),
]


@pytest.mark.parametrize("storage", ["reference", "split", "bricked"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_ray_grads_match_oracle(storage, case):
    K, diffuse, mode, white, aabb_sampling, jitter, occ, S, dims, rho = CASES[case]
    dev = torch.device("cuda:0")
    if occ:
        dens, feat = sparse_scene_grid(dims, 3 * K, 40 + case)
    else:
        dens, feat = procedural_grid(dims, 3 * K, 40 + case)
    if mode == "identity":  # (positive densities: a negative sigma over the last sample's 1e10-long interval makes the reference's alpha -inf)
        dens = dens.abs() + 0.05
    voxel = (3.0 / dims[0], 2.8 / dims[1], 3.1 / dims[2])
    aabb = orc.make_aabb(dims, voxel)
    half = np.array([hi for _, hi in aabb])
    n = 48
    o, d = make_rays(n, 7 + case, half)
    near, far = near_far()
    t_rand = t_tab = None
    if jitter == "table":
        t_tab = torch.from_numpy(hash_uniform((n, S), 99 + case, 0.0, 1.0))
        t_rand = t_tab.to(dev)
    elif jitter == "keyed":
        key = 0x1234_5678_9ABC + case
        t_rand = ops.KeyedJitter(key, 0)
        t_tab = torch.from_numpy(orc.keyed_jitter(key, 0, n, S))
    grid = make_grid(dev, dens, feat, voxel, storage, mode, rho)
    w = [torch.from_numpy(hash_uniform(shape, 300 + case + j)) for j, shape in enumerate([(n, 3), (n, 1), (n, 1)])]
    # the mixed loss, then each upstream gradient alone
    mixed_scale = [0.0, 0.0]
    for name, weights in (("mixed", w), ("colour", [w[0], 0 * w[1], 0 * w[2]]), ("depth", [0 * w[0], w[1], 0 * w[2]]), ("acc", [0 * w[0], 0 * w[1], w[2]])):
        go, gd = hip_ray_grads(grid, o, d, S, near, far, t_rand, white, diffuse, aabb_sampling, occ, weights, dev)
        args = (dens, feat, o, d, aabb, near, far, S, rho, mode, white, diffuse, aabb_sampling, t_tab, weights)
        r32 = oracle_ray_grads(*args, torch.float32)
        r64 = oracle_ray_grads(*args, torch.float64)
        check(f"case {case} {storage} {name} d/do", go, r32[0], r64[0], mixed_scale[0])
        check(f"case {case} {storage} {name} d/dd", gd, r32[1], r64[1], mixed_scale[1])
        if name == "mixed":
            mixed_scale = [r64[0].abs().max().item(), r64[1].abs().max().item()]


def test_ray_grads_float64_inputs_and_long_rays():
    """float64 rays get float64 gradients; rays of more than 4096 samples walk many chunks."""
    dev = torch.device("cuda:0")
    dims = (8, 8, 8)
    dens, feat = procedural_grid(dims, 12, 5)
    voxel = (3.0 / 8,) * 3
    aabb = orc.make_aabb(dims, voxel)
    o, d = make_rays(6, 3, np.array([hi for _, hi in aabb]))
    near, far = near_far()
    S = 4500
    grid = make_grid(dev, dens, feat, voxel, "split", "relu", 2.0)
    w = [torch.from_numpy(hash_uniform(shape, 11 + j)) for j, shape in enumerate([(6, 3), (6, 1), (6, 1)])]
    for aabb_sampling in (False, True):
        go, gd = hip_ray_grads(grid, o.double(), d.double(), S, near, far, None, True, False, aabb_sampling, False, w, dev, torch.float64)
        args = (dens, feat, o, d, aabb, near, far, S, 2.0, "relu", True, False, aabb_sampling, None, w)
        r32, r64 = oracle_ray_grads(*args, torch.float32), oracle_ray_grads(*args, torch.float64)
        check(f"long aabb={aabb_sampling} d/do", go, r32[0], r64[0])
        check(f"long aabb={aabb_sampling} d/dd", gd, r32[1], r64[1])


def test_surface_then_empty_space_interval_coupling():
    """A surface followed by empty space under AABB sampling: the cached sample in front of an uncached one still moves that
    sample's z through its interval (the +|d| g_delta term attributed at the cached sample)."""
    dev = torch.device("cuda:0")
    dims = (16, 16, 16)
    dens, feat = sparse_scene_grid(dims, 27, 3)
    dens = torch.where(dens > 0, dens, torch.full_like(dens, -1.0))  # empty space (sigma = 0 under ReLU) around a solid core
    voxel = (3.0 / 16,) * 3
    aabb = orc.make_aabb(dims, voxel)
    n = 32
    u = hash_uniform((n, 3), 8, -0.3, 0.3).astype(np.float32)
    o = torch.from_numpy(np.tile(np.array([[0.0, 0.0, 4.0]], np.float32), (n, 1)))
    d = torch.from_numpy(np.stack([u[:, 0], u[:, 1], -np.ones(n, np.float32)], axis=-1))
    near, far = near_far()
    grid = make_grid(dev, dens, feat, voxel, "split", "relu", 1.0)
    w = [torch.from_numpy(hash_uniform(shape, 21 + j)) for j, shape in enumerate([(n, 3), (n, 1), (n, 1)])]
    go, gd = hip_ray_grads(grid, o, d, 96, near, far, None, False, False, True, False, w, dev)
    args = (dens, feat, o, d, aabb, near, far, 96, 1.0, "relu", False, False, True, None, w)
    r32, r64 = oracle_ray_grads(*args, torch.float32), oracle_ray_grads(*args, torch.float64)
    check("surface/empty d/do", go, r32[0], r64[0])
    check("surface/empty d/dd", gd, r32[1], r64[1])


@pytest.mark.parametrize("storage", ["reference", "split", "bricked"])
@pytest.mark.parametrize("mode", ["relu", "softplus", "abs", "identity"])
def test_point_grads_of_grid_query(storage, mode):
    dev = torch.device("cuda:0")
    dims = (7, 9, 8)
    dens, feat = procedural_grid(dims, 27, 61)
    voxel = (3.0 / 7, 3.0 / 9, 3.0 / 8)
    aabb = orc.make_aabb(dims, voxel)
    grid = make_grid(dev, dens, feat, voxel, storage, mode, 3.0)
    pts = torch.from_numpy(hash_uniform((500, 3), 62, -1.7, 1.7))
    g_out = torch.from_numpy(hash_uniform((500, 28), 63))
    p = pts.to(dev).requires_grad_(True)
    (grid(p) * g_out.to(dev)).sum().backward()
    ref = {}
    for dt in (torch.float32, torch.float64):
        q = pts.to(dt).clone().requires_grad_(True)
        (orc.voxel_grid_forward(dens.to(dt), feat.to(dt), q, aabb, 3.0, mode) * g_out.to(dt)).sum().backward()
        ref[dt] = q.grad
    check(f"grid_query {storage} {mode}", p.grad, ref[torch.float32], ref[torch.float64])


def test_point_grads_of_interpolate_tensors_and_composed_render():
    dev = torch.device("cuda:0")
    dims = (8, 8, 8)
    dens, feat = procedural_grid(dims, 12, 71)
    voxel = (3.0 / 8,) * 3
    aabb = orc.make_aabb(dims, voxel)
    grid = make_grid(dev, dens, feat, voxel, "reference", "relu", 1.0)
    pts = torch.from_numpy(hash_uniform((300, 3), 72, -1.6, 1.6))
    g_out = torch.from_numpy(hash_uniform((300, 13), 73))
    p = pts.to(dev).requires_grad_(True)
    (ops.interpolate_tensors(grid, dens.to(dev), feat.to(dev), p) * g_out.to(dev)).sum().backward()
    ref = {}
    for dt in (torch.float32, torch.float64):
        q = pts.to(dt).clone().requires_grad_(True)
        both = torch.cat([orc.trilinear_recipe(feat.to(dt), orc.normalise_points(q, aabb)), orc.trilinear_recipe(dens.to(dt), orc.normalise_points(q, aabb))], dim=-1)
        (both * g_out.to(dt)).sum().backward()
        ref[dt] = q.grad
    check("interpolate_tensors", p.grad, ref[torch.float32], ref[torch.float64])

    # the composed path (torch sampler and compositor around the HIP grid query, with density noise): ray-differentiable through the
    # point gradients -- against the oracle, then once more with a non-default density2occupancy
    from thr3ed_atom_amd import composable

    n, S = 24, 32
    o, d = make_rays(n, 74, np.array([hi for _, hi in aabb]))
    near, far = near_far()
    # (non-negative: a negative density over the last sample's 1e10-long interval makes alpha -inf, in the reference too)
    noise = torch.from_numpy(hash_uniform((n, S), 75, 0.0, 0.5))
    wc = torch.from_numpy(hash_uniform((n, 3), 76))

    def composed(d2o):
        oo, dd = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
        rays = rf.Rays(oo, dd)
        pts_on = composable.sample_uniform_points_on_rays(rays, rf.CameraBounds(near, far), S, perturb=False)
        procd = composable.process_points_with_sh_voxel_grid(pts_on, rays, grid)
        out = composable.accumulate_radiance_density_on_rays(procd, rays, density_noise=noise.to(dev), white_bkgd=False, density2occupancy=d2o)
        (out.colour * wc.to(dev)).sum().backward()
        return oo.grad, dd.grad

    go, gd = composed(composable.density2occupancy_pb)
    ref = {}
    for dt in (torch.float32, torch.float64):
        oo, dd = o.to(dt).clone().requires_grad_(True), d.to(dt).clone().requires_grad_(True)
        out = orc.render(dens, feat, oo, dd, aabb, near, far, S, 1.0, "relu", white_bkgd=False, density_noise=noise)
        (out["colour"] * wc.to(dt)).sum().backward()
        ref[dt] = (oo.grad, dd.grad)
    check("composed d/do", go, ref[torch.float32][0], ref[torch.float64][0])
    check("composed d/dd", gd, ref[torch.float32][1], ref[torch.float64][1])
    go, gd = composed(lambda s, dl: 1.0 - torch.exp(-torch.nn.functional.softplus(s) * dl))
    assert torch.isfinite(go).all() and torch.isfinite(gd).all() and go.abs().max() > 0


def _oracle_pose_grads(dens, feat, aabb, H, W, focal, R, t, S, rho, target, aabb_sampling, dtype):
    RR = R.clone().requires_grad_(True)
    tt = t.clone().requires_grad_(True)
    # the oracle's cast_rays is float32 by construction (misc.py:31-32); re-express it differentiably in `dtype`
    xs = (torch.arange(W, dtype=dtype) + 0.5 - W * 0.5) / focal
    ys = -((torch.arange(H, dtype=dtype) + 0.5 - H * 0.5) / focal)
    cam = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), -torch.ones(H, W, dtype=dtype)], dim=-1).reshape(-1, 3)
    dirs = cam @ RR.to(dtype).T
    origins = tt.to(dtype).reshape(1, 3).expand(H * W, 3)
    near, far = near_far()
    out = orc.render(dens.to(dtype), feat.to(dtype), origins, dirs, aabb, near, far, S, rho, "relu", white_bkgd=True, optimized_sampling=aabb_sampling)
    torch.nn.functional.l1_loss(out["colour"], target.to(dtype)).backward()
    return RR.grad, tt.grad


@pytest.mark.parametrize("aabb_sampling", [False, True])
def test_pose_grads_match_oracle(aabb_sampling):
    dev = torch.device("cuda:0")
    dims = (16, 16, 16)
    dens, feat = sparse_scene_grid(dims, 27, 81)
    voxel = (3.0 / 16,) * 3
    aabb = orc.make_aabb(dims, voxel)
    grid = make_grid(dev, dens, feat, voxel, "reference", "relu", 10.0)
    near, far = near_far()
    cfg = rf.SHVoxGridRenderConfig(32, rf.CameraBounds(near, far), perturb_sampled_points=False, white_bkgd=True, optimized_sampling=aabb_sampling)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    H = W = 16
    focal = 20.0
    pose = rf.pose_spherical(30.0, -30.0, hotdog_like_camera()["radius"])
    target = torch.from_numpy(hash_uniform((H * W, 3), 82, 0.0, 1.0))
    R = pose.rotation.clone().to(dev).requires_grad_(True)
    t = pose.translation.clone().to(dev).requires_grad_(True)
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(H, W, focal), rf.CameraPose(R, t), dev))
    torch.nn.functional.l1_loss(model.render_rays(rays).colour, target.to(dev)).backward()
    assert R.grad is not None and t.grad is not None and t.grad.shape == (3, 1)
    r32 = _oracle_pose_grads(dens, feat, aabb, H, W, focal, pose.rotation, pose.translation, 32, 10.0, target, aabb_sampling, torch.float32)
    r64 = _oracle_pose_grads(dens, feat, aabb, H, W, focal, pose.rotation.double(), pose.translation.double(), 32, 10.0, target, aabb_sampling, torch.float64)
    check(f"pose aabb={aabb_sampling} dR", R.grad, r32[0], r64[0])
    check(f"pose aabb={aabb_sampling} dt", t.grad, r32[1], r64[1])


@pytest.mark.parametrize("backward", ["atomic", "binned"])
def test_nothing_changes_where_nothing_new_is_asked(backward, monkeypatch):
    """Forward outputs and grid gradients are bitwise the same whether or not the rays require grad; two ray-gradient backward
    passes are bitwise identical; the pair op with ray gradients equals two single ops."""
    monkeypatch.setattr(ops, "AUTOGRAD_BACKWARD", backward)
    dev = torch.device("cuda:0")
    dims = (16, 16, 16)
    dens, feat = procedural_grid(dims, 27, 91)
    voxel = (3.0 / 16,) * 3
    near, far = near_far()
    o, d = make_rays(256, 92, np.array([1.5, 1.5, 1.5]))
    o, d = o.to(dev), d.to(dev)
    wc = torch.from_numpy(hash_uniform((256, 3), 93)).to(dev)

    def run(ray_grad):
        grid = make_grid(dev, dens, feat, voxel, "split", "relu", 3.0, tunable=True)
        oo, dd = o.clone().requires_grad_(ray_grad), d.clone().requires_grad_(ray_grad)
        outs = ops.relu_field_render(grid, oo, dd, 64, near, far, t_rand=ops.KeyedJitter(5), white_bkgd=True, optimized_sampling=True)
        (outs[0] * wc).sum().backward()
        gd, gf = grid.reference_gradients()
        return [x.detach().clone() for x in outs] + [gd.clone(), gf.clone()], (oo.grad, dd.grad)

    base, none = run(False)
    base2, _ = run(False)
    with_rays, g1 = run(True)
    _, g2 = run(True)
    assert none == (None, None)
    for a, b in zip(base[:4], with_rays[:4]):  # forward outputs: bit for bit
        assert torch.equal(a.nan_to_num(), b.nan_to_num())
    # grid gradients: the same launches either way.  Both grid adjoints sum in an order that varies from run to run (float atomics
    # resp. records placed by atomic cursors), so they are bitwise equal where two plain runs are, and within that spread otherwise
    for a, a2, b in zip(base[4:], base2[4:], with_rays[4:]):
        spread = (a - a2).abs().max().item()
        print(f"{backward}: grid gradient run-to-run spread {spread:.3e}, with ray gradients {(a - b).abs().max().item():.3e}")
        if spread == 0.0:
            assert torch.equal(a, b)
        else:
            assert (a - b).abs().max().item() <= 4.0 * spread + 1e-6 * a.abs().max().item()
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])  # the ray adjoint itself: bitwise deterministic

    # the pair op with ray gradients = the two single ops
    grid = make_grid(dev, dens, feat, voxel, "split", "relu", 3.0, tunable=False)
    oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    p0, p1 = ops.relu_field_render_pair(grid, oo, dd, 64, near, far, white_bkgd=True)
    ((p0[0] + 2.0 * p1[0]) * wc).sum().backward()
    oo2, dd2 = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    s0 = ops.relu_field_render(grid, oo2, dd2, 64, near, far, white_bkgd=True)
    s1 = ops.relu_field_render(grid, oo2, dd2, 64, near, far, white_bkgd=True, render_diffuse=True)
    ((s0[0] + 2.0 * s1[0]) * wc).sum().backward()
    assert torch.equal(oo.grad, oo2.grad) and torch.equal(dd.grad, dd2.grad)


def test_refine_camera_pose_end_to_end():
    """A target rendered at a known pose of a 64^3 sparse scene; refine_camera_pose from 3 degrees and 0.05 world units away.
    Measured once on an MI355X (600 iterations, lr 1e-2 decaying to 1e-4): 0.35 deg / 0.023 after 100 iterations, 0.063 deg / 0.0044
    after 200, below 0.02 deg (the float32 resolution of the angle) / 0.00012 at the end.  Bars: 0.2 degrees and 0.005 world units."""
    dev = torch.device("cuda:0")
    dims = (64, 64, 64)
    dens, feat = sparse_scene_grid(dims, 27, 101)
    grid = make_grid(dev, dens, feat, (3.0 / 64,) * 3, "split", "relu", 30.0, tunable=True)
    near, far = near_far()
    cfg = rf.SHVoxGridRenderConfig(96, rf.CameraBounds(near, far), perturb_sampled_points=False, white_bkgd=True, optimized_sampling=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    intr = rf.CameraIntrinsics(48, 48, 60.0)
    true_pose = rf.pose_spherical(40.0, -35.0, hotdog_like_camera()["radius"])
    with torch.no_grad():
        target = model.render(true_pose, intr).colour
    axis = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float32)
    start = rf.perturb_pose(true_pose, axis / axis.norm() * np.deg2rad(3.0), torch.tensor([0.03, -0.04, 0.0]))
    from thr3ed_atom_amd.pose_refinement import pose_error

    e0 = pose_error(start, true_pose)
    pose, history = rf.refine_camera_pose(model, target, intr, start, num_iterations=600, learning_rate=1e-2)
    e1 = pose_error(pose, true_pose)
    for it in (100, 200, 300, 400, 500):
        e = pose_error(rf.CameraPose(torch.from_numpy(history[it]["rotation"]), torch.from_numpy(history[it]["translation"])), true_pose)
        print(f"refine: iteration {it}: {e[0]:.4f} deg / {e[1]:.5f}, L1 {history[it]['loss']:.6f}")
    print(f"refine: start {e0[0]:.3f} deg / {e0[1]:.4f}, final {e1[0]:.4f} deg / {e1[1]:.5f}, L1 {history[0]['loss']:.5f} -> {history[-1]['loss']:.5f}")
    assert abs(e0[0] - 3.0) < 1e-3 and abs(e0[1] - 0.05) < 1e-6
    params = [t for t in grid.kernel_tensors() if t is not None]
    assert all(t.grad is None for t in params)  # the field stays frozen
    assert all(t.requires_grad for t in params)  # ... and trainable again afterwards
    assert e1[0] < 0.2 and e1[1] < 0.005


def test_refine_cli_on_a_trained_checkpoint(tmp_path):
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)

    def run(args):
        return subprocess.run([sys.executable] + args, cwd=root, env=env, capture_output=True, text=True, timeout=900)

    out = tmp_path / "run"
    r = run(["scripts/train_sh_based_voxel_grid.py", "-o", str(out), "--synthetic", "True", "--synthetic_size", "48", "--grid_dims", "32", "32", "32",
             "--sh_degree", "0", "--ray_batch_size", "2048", "--train_num_samples_per_ray", "64", "--render_num_samples_per_ray", "64",
             "--num_stages", "1", "--num_iterations_per_stage", "20", "--save_frequency", "1000", "--test_frequency", "1000",
             "--summary_frequency", "10", "--num_workers", "2", "--feedback_frequency", "1000", "--fast_debug_mode", "False"])
    assert r.returncode == 0, r.stderr[-2000:]
    image = tmp_path / "image.npy"
    np.save(image, hash_uniform((24, 24, 3), 5, 0.0, 1.0))
    res = tmp_path / "refined"
    r = run(["scripts/refine_camera_pose.py", "-i", str(out / "saved_models" / "model_final.pth"), "--image", str(image), "-o", str(res),
             "--yaw", "20", "--pitch", "-30", "--num_iterations", "3", "--num_samples_per_ray", "32"])
    assert r.returncode == 0, r.stderr[-2000:]
    m = np.load(res / "refined_pose.npy")
    assert m.shape == (3, 4) and np.isfinite(m).all()
    assert (res / "refined_pose.json").exists() and ((res / "refined_render.png").exists() or (res / "refined_render.npy").exists())


@pytest.mark.parametrize("storage", ["reference", "split"])
def test_pose_and_ray_grads_match_reference_fixture(storage):
    """Against the reference's own float32 gradients (g16_ray_pose_grads.npz), with the oracle's float64 as the yardstick:
    |hip - orc64| <= |reference - orc64| + C_GRAD * max |orc64|."""
    from tests.helpers import load_golden
    from tests.ray_grads_common import GOLDEN_CASES, golden_inputs, oracle_pose_grads

    g = load_golden("g16_ray_pose_grads.npz")
    dev = torch.device("cuda:0")
    for i, case in enumerate(GOLDEN_CASES):
        inp = golden_inputs(case)
        grid = make_grid(dev, inp["dens"], inp["feat"], inp["voxel"], storage, "relu", inp["rho"])
        near, far = inp["bounds"]
        cfg = rf.SHVoxGridRenderConfig(inp["num_samples"], rf.CameraBounds(near, far), perturb_sampled_points=False, white_bkgd=case["white"],
                                       optimized_sampling=case["aabb"])
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        R = inp["rotation"].to(dev).requires_grad_(True)
        t = inp["translation"].to(dev).requires_grad_(True)
        rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(*inp["intrinsics"]), rf.CameraPose(R, t), dev))
        rays.origins.retain_grad()
        rays.directions.retain_grad()
        torch.nn.functional.l1_loss(model.render_rays(rays).colour, inp["target"].to(dev)).backward()
        r64 = oracle_pose_grads(inp, case["aabb"], case["white"], torch.float64)
        for key, hip, o64 in zip(("R_grad", "t_grad", "origins_grad", "directions_grad"), (R.grad, t.grad, rays.origins.grad, rays.directions.grad), r64):
            check(f"g16 case {i} {storage} {key}", hip, torch.from_numpy(g[f"c{i}_{key}"]), o64)
