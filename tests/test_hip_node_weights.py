"""Visibility statistics and pruning on the GPU: rf_node_max_weight against the float64 model (tests/node_weights_model.py) and
its exact properties, rf_prune_grid against the numpy model bit for bit, the end-to-end scene, and the trainer integration."""
import functools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import node_weights_model as nm
from tests.helpers import hash_uniform, hotdog_like_camera, procedural_grid, signed_density_grid, sparse_scene_grid
from thr3ed_atom_amd import _lib, ops
from thr3ed_atom_amd.trainers import PosedImagesInMemory, train_sh_vox_grid_vol_mod_with_posed_images
from thr3ed_atom_amd.voxels import brick_nodes, unpack_storage

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the project's bar on acc = sum_i w_i: every w_i * b_k is one term of such a sum, and max is 1-Lipschitz
STORAGES = ["reference", "split", "bricked"]
MODES = ["relu", "softplus", "abs", "identity"]
ACTIVATIONS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
               "abs": (torch.abs, torch.nn.Identity()), "identity": (torch.nn.Identity(), torch.nn.Identity())}
DIMS = [(2, 2, 2), (3, 4, 5), (9, 8, 17), (16, 16, 24)]
SAMPLES = [1, 7, 64, 65, 130]  # a single sample, a partial chunk, one full chunk, the lane-63 -> lane-0 hand-over, a third chunk
OPTIONS = ["plain", "aabb", "occupancy", "t_rand", "keyed"]
RAY_SIDES = [8, 12, 16, 22]  # 64 .. 484 rays (pixel rays of a wide camera: part of them miss the box)


def T(a):
    return torch.from_numpy(np.asarray(a))


def voxel_of(dims):
    return (3.0 / max(dims),) * 3


def rho_of(mode):
    # identity: sigma < 0 in pockets makes the transmittance grow; a small scale keeps the weights O(1), where the absolute bar means something
    return 0.5 if mode == "identity" else 100.0 / 3.0


@functools.lru_cache(maxsize=None)
def raw_grid(dims, F, mode):
    return signed_density_grid(dims, F, 21) if mode == "identity" else procedural_grid(dims, F, 21)


def make_grid(dev, dens, feat, dims, storage, mode, rho=None):
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*voxel_of(dims)), density_preactivation=ACTIVATIONS[mode][0],
                        density_postactivation=ACTIVATIONS[mode][1], expected_density_scale=rho_of(mode) if rho is None else rho, tunable=False, storage=storage)


@functools.lru_cache(maxsize=None)
def rays_of(side, S):
    """(origins, directions, near, far) on the CPU: the pixel rays of a wide camera; a single-sample ray samples z = near, so near
    is put inside the volume there"""
    cam = hotdog_like_camera()
    pose = rf.pose_spherical(40.0, -35.0, cam["radius"])
    o, d = orc.cast_rays(side, side, side * 0.9, torch.as_tensor(pose.rotation), torch.as_tensor(pose.translation))
    near = 3.9 if S == 1 else cam["near"]
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), float(np.float32(near)), cam["far"]


def kernel_cases():
    """dims x storage x S in full; the other factors are dealt out so that every storage and every S meets each of their values"""
    cases = []
    for j, (dims, storage) in enumerate((d, st) for d in DIMS for st in STORAGES):
        for s, S in enumerate(SAMPLES):
            option = OPTIONS[(2 * j + s) % 5]
            if S == 1 and option == "aabb":  # (the one sample would sit ON the box: t = t_enter -- nothing to compare)
                option = "plain"
            cases.append((dims, storage, S, (3, 27)[(j + s // 2 + j // 4) % 2], MODES[(j + s) % 4], option, RAY_SIDES[(j + 3 * s + j // 4) % 4]))
    return cases


def test_the_case_table_meets_every_value_of_every_factor():
    cases = kernel_cases()
    for col, values in ((3, (3, 27)), (4, MODES), (5, OPTIONS), (6, RAY_SIDES)):
        for storage in STORAGES:
            assert {c[col] for c in cases if c[1] == storage} == set(values), (col, storage)
        for S in SAMPLES:
            assert {c[col] for c in cases if c[2] == S} | ({"aabb"} if S == 1 else set()) >= set(values), (col, S)
        for dims in DIMS:
            assert {c[col] for c in cases if c[0] == dims} == set(values), (col, dims)


@functools.lru_cache(maxsize=None)
def reference(dims, F, mode, S, option, side):
    """(M64, jitter table or None, model weights w [N,S]) of the case -- computed once, never modified"""
    dens, _ = raw_grid(dims, F, mode)
    o, d, near, far = rays_of(side, S)
    t_rand = None
    if option == "t_rand":
        t_rand = T(hash_uniform((o.shape[0], S), 77, 0.0, 1.0))
    elif option == "keyed":
        t_rand = T(orc.keyed_jitter(0xC0FFEE1234, 5, o.shape[0], S).astype(np.float32))
    M64, w, _ = nm.model_max_weight(dens, orc.make_aabb(dims, voxel_of(dims)), rho_of(mode), mode, o, d, near, far, S, optimized_sampling=(option == "aabb"), t_rand=t_rand)
    return M64, t_rand, w


def launch(grid, o, d, S, near, far, option, t_rand, out, dev, first_ray=0):
    flags = 0
    jitter = None
    if option == "aabb":
        flags |= _lib.FLAG_AABB_SAMPLING
    if option == "occupancy":
        grid.build_occupancy()
        flags |= _lib.FLAG_OCCUPANCY_SKIP
    if option == "t_rand":
        jitter = t_rand.to(dev).contiguous()
    if option == "keyed":
        jitter = ops.KeyedJitter(0xC0FFEE1234, 5 + first_ray)
    # (the two flags the statistic must ignore ride along on every other case)
    flags |= (_lib.FLAG_WHITE_BKGD | _lib.FLAG_RENDER_DIFFUSE) if S % 2 else 0
    ops.node_max_weight_raw(grid, ops.RayBatch(o.to(dev), d.to(dev), S, near, far, t_rand=jitter), flags, out)


@pytest.mark.parametrize("dims,storage,S,F,mode,option,side", kernel_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_equals_the_float64_model(hip_device, dims, storage, S, F, mode, option, side):
    """|M - M64| <= TOL on every node, with rays that miss the box in the batch; the statistic is not vacuous."""
    dens, feat = raw_grid(dims, F, mode)
    M64, t_rand, w = reference(dims, F, mode, S, option, side)
    o, d, near, far = rays_of(side, S)
    assert (np.abs(w).sum(-1) == 0).any() or S == 1, "no ray of the batch misses the box"
    assert M64.max() > 1e-3 and M64.max() < 64.0, M64.max()
    grid = make_grid(hip_device, dens, feat, dims, storage, mode)
    out = torch.zeros(dims, device=hip_device)
    launch(grid, o, d, S, near, far, option, t_rand, out, hip_device)
    M = out.cpu().numpy().astype(np.float64)
    err = np.abs(M - M64).max()
    print(f"node_max_weight {dims} {storage} S={S} F={F} {mode} {option} {o.shape[0]} rays: max |M - M64| = {err:.3e} (max M64 {M64.max():.3f})")
    assert np.isfinite(M).all() and (M >= 0).all()
    assert err <= TOL, err


def padding_mask(grid, like):
    X, Y, Z = grid.grid_dims
    real = brick_nodes(torch.ones((X, Y, Z, 1), device=like.device))
    return (real == 0).expand_as(like)


@pytest.mark.parametrize("storage", STORAGES)
def test_exact_properties_of_the_statistic(hip_device, storage):
    """max(prefill, statistic) with untouched nodes keeping their bits; idempotent; independent of the ray order and of how the
    rays are split into calls (keyed jitter: first_ray); NaN in bricked padding and behind the buffer's end is never read or written."""
    dims, F, mode, S, side = (9, 8, 17), 27, "relu", 65, 16
    dens, feat = raw_grid(dims, F, mode)
    o, d, near, far = rays_of(side, S)
    n = o.shape[0]
    grid = make_grid(hip_device, dens, feat, dims, storage, mode)
    if storage == "bricked":
        for t in grid.kernel_tensors():
            t.data[padding_mask(grid, t)] = float("nan")
    nodes = int(np.prod(dims))
    whole = torch.full((nodes + 64,), float("nan"), device=hip_device)  # NaN sentinels after the buffer's end

    def run(order=None, pieces=None, prefill=None):
        whole[:nodes] = 0.0 if prefill is None else prefill.reshape(-1)
        out = whole[:nodes].view(dims)
        oo, dd = (o, d) if order is None else (o[order], d[order])
        if pieces is None:
            launch(grid, oo, dd, S, near, far, "keyed" if order is None else "plain", None, out, hip_device)
        else:
            for lo, hi in pieces:
                launch(grid, oo[lo:hi].contiguous(), dd[lo:hi].contiguous(), S, near, far, "keyed", None, out, hip_device, first_ray=lo)
        assert bool(torch.isnan(whole[nodes:]).all()), "written past the end of the buffer"
        return out.clone()

    keyed = run()
    assert bool(torch.isfinite(keyed).all()) and float(keyed.max()) > 1e-3
    assert torch.equal(run(pieces=[(0, 100), (100, n)]), keyed)  # one call == two calls with first_ray set
    plain = run(order=torch.arange(n))
    perm = T(np.argsort(hash_uniform((n,), 5), kind="stable"))
    assert torch.equal(run(order=perm), plain)  # arrival order does not matter
    # prefill 0.25 on a checkerboard
    ix = np.indices(dims).sum(0) % 2 == 0
    prefill = torch.where(T(ix).to(hip_device), torch.tensor(0.25, device=hip_device), torch.tensor(0.0, device=hip_device))
    got = run(prefill=prefill)
    assert torch.equal(got, torch.maximum(prefill, keyed))
    assert bool((got == 0.25).any()) and bool((got > 0.25).any())
    # a second launch on the result changes no bit
    whole[:nodes] = got.reshape(-1)
    again = whole[:nodes].view(dims)
    launch(grid, o, d, S, near, far, "keyed", None, again, hip_device)
    assert torch.equal(again, got)


# --------------------------------------------------------------------------------------------
# rf_prune_grid
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 5), (9, 8, 17)], ids=lambda d: "x".join(map(str, d)))
def test_prune_equals_the_numpy_model_bit_for_bit(hip_device, dims, dilate, storage):
    """keep mask, densities, features, bricked padding (NaN sentinels) and the counts, every density mode"""
    for i, mode in enumerate(MODES):
        F = (3, 27)[i % 2]
        dens, feat = procedural_grid(dims, F, 31 + i)
        # a sparse statistic with entries below, at and above the threshold
        u = hash_uniform(dims, 41 + i, 0.0, 1.0)
        threshold = 0.5 if i % 2 else 0.0
        M = np.where(u > 0.93, u, np.where(u > 0.88, np.float32(threshold), np.float32(0.0))).astype(np.float32)
        if max(dims) == 1:
            M[...] = 0.7 if dilate == 1 else 0.0
        fill = {"relu": 0.0, "softplus": -3.0, "abs": 0.0, "identity": -0.25}[mode]
        keep64, new64, counts64 = nm.prune(dens.numpy(), M, threshold, dilate, fill, mode)
        grid = make_grid(hip_device, dens, feat, dims, storage, mode)
        tensors = grid.kernel_tensors()
        if storage == "bricked":
            for t in tensors:
                if t is not None:
                    t.data[padding_mask(grid, t)] = float("nan")
        before = [None if t is None else t.clone() for t in tensors]
        keep = torch.full(dims, 7, dtype=torch.uint8, device=hip_device)
        counts = torch.tensor([100, 1000], dtype=torch.int64, device=hip_device)
        ops.prune_grid_raw(grid, T(M).to(hip_device), threshold, dilate, fill, keep=keep, counts=counts)
        assert np.array_equal(keep.cpu().numpy().astype(bool), keep64) and int(keep.max()) <= 1
        assert counts.tolist() == [100 + counts64[0], 1000 + counts64[1]]  # added to
        d_after, f_after = unpack_storage(tensors[0], tensors[1], storage, dims)
        assert np.array_equal(d_after.cpu().numpy().view(np.uint32), new64.view(np.uint32)), mode
        assert np.array_equal(f_after.cpu().numpy().view(np.uint32), feat.numpy().view(np.uint32))
        if storage == "bricked":
            for t in tensors:
                if t is not None:
                    pad = padding_mask(grid, t)
                    assert bool(torch.isnan(t[pad]).all()) and bool(torch.isfinite(t[~pad]).all())
        if storage != "reference":  # everything but the density element keeps its bits
            assert torch.equal(tensors[0][..., 1:].isnan() | (tensors[0][..., 1:] == before[0][..., 1:]), torch.ones_like(tensors[0][..., 1:], dtype=torch.bool))
        # the Python entry: same result from the original grid, stats returned
        grid2 = make_grid(hip_device, dens, feat, dims, storage, mode)
        stats = rf.prune_voxel_grid(grid2, T(M).to(hip_device), threshold, dilate, fill_density=fill)
        assert stats == rf.PruneStats(*counts64)
        assert np.array_equal(grid2.densities.detach().cpu().numpy().view(np.uint32), new64.view(np.uint32))


# --------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------
def scene_setup(dev, storage="split"):
    cam = hotdog_like_camera()
    dens, feat = nm.scene_grid()
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(*nm.SCENE_VOXEL), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(),
                        expected_density_scale=nm.SCENE_RHO, tunable=False, storage=storage)
    bounds = rf.CameraBounds(cam["near"], cam["far"])
    cfg = rf.SHVoxGridRenderConfig(nm.SCENE_SAMPLES, bounds, perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    (h, w, focal), poses = nm.scene_views()
    return grid, model, rf.CameraIntrinsics(h, w, focal), poses, bounds


def render_all(model, intr, poses, dev):
    rays, frames = [], []
    with torch.no_grad():
        for pose in poses:
            flat = rf.flatten_rays(rf.cast_rays(intr, pose, dev))
            out = model.render_rays(flat)
            rays.append((out.colour.clone(), out.depth.clone(), out.extra["accumulated_weight"].clone()))
            frames.append(model.render(pose, intr, perturb_sampled_points=False).colour.clone())
    return rays, frames


def occupied_cells(grid):
    occ = grid.build_occupancy().cpu().numpy().view(np.uint32)
    return int(sum(bin(int(v)).count("1") for v in occ))


def test_pruning_the_scene_end_to_end(hip_device):
    """threshold 0 / dilate 0 on one grid: bit-identical ray renders, the packet kernel within TOL, the blob at the fill.
    threshold tau / dilate 1 on a FRESH grid (the default dilation keeps the few wall nodes that the 32 x 32 rays happen not to
    weight, which dilate 0 turns into pinholes of the mesh): the speck goes too, fewer occupied cells, a smaller mesh without the blob."""
    grid, model, intr, poses, bounds = scene_setup(hip_device)
    shell, blob, speck = nm.scene_regions()
    M = rf.node_max_weights(model, poses, intr, bounds, nm.SCENE_SAMPLES)
    Mh = M.cpu().numpy()
    assert Mh[blob].max() == 0.0 and 0.0 < Mh[speck].max() < nm.SCENE_TAU < Mh[shell].max()
    rays_before, frames_before = render_all(model, intr, poses, hip_device)
    cells_before = occupied_cells(grid)
    mesh_before = rf.extract_mesh(grid, 1.0)
    # the blob's box, one voxel of margin (its surface lies between the blob's outermost nodes and their negative neighbours)
    lo, hi = ((nm.BLOB[0] - 1 + 0.5) * nm.SCENE_VOXEL[0] - 1.5, (nm.BLOB[1] + 1 + 0.5) * nm.SCENE_VOXEL[0] - 1.5)
    inside_blob = lambda v: bool(((v > lo) & (v < hi)).all(dim=-1).any())  # noqa: E731
    assert inside_blob(mesh_before.vertices)

    stats = rf.prune_voxel_grid(grid, M, threshold=0.0, dilate=0)
    assert stats.kept == int((Mh > 0).sum()) and stats.kept + stats.pruned == Mh.size
    rays_after, frames_after = render_all(model, intr, poses, hip_device)
    for before, after in zip(rays_before, rays_after):
        for a, b in zip(before, after):
            assert torch.equal(a, b)  # colour, depth, acc: bit-identical
    for a, b in zip(frames_before, frames_after):  # the packet kernel
        assert float((a - b).abs().max()) <= TOL
    dens = grid.densities.detach().cpu().numpy()[..., 0]
    assert (dens[blob] == 0.0).all() and dens[speck].item() == np.float32(2e-4)
    assert occupied_cells(grid) < cells_before
    assert not inside_blob(rf.extract_mesh(grid, 1.0).vertices)

    grid, model, *_ = scene_setup(hip_device)
    stats = rf.prune_voxel_grid(grid, M, threshold=nm.SCENE_TAU, dilate=1)
    dens = grid.densities.detach().cpu().numpy()[..., 0]
    assert dens[speck].item() == 0.0 and (dens[blob] == 0.0).all() and (dens[shell] == np.float32(nm.SHELL_DENSITY)).all()
    assert stats.kept == int(nm.keep_mask(Mh, nm.SCENE_TAU, 1).sum())
    assert occupied_cells(grid) < cells_before
    mesh_after = rf.extract_mesh(grid, 1.0)
    assert mesh_after.vertices.shape[0] < mesh_before.vertices.shape[0] and not inside_blob(mesh_after.vertices)


def test_a_reference_storage_grid_renders_the_pruned_values_on_the_next_call(hip_device):
    """(the split shadow of the forward passes is refreshed) -- and a VoxelGrid-like module of another class prunes through its view"""
    grid, model, intr, poses, bounds = scene_setup(hip_device, storage="reference")
    twin, twin_model, *_ = scene_setup(hip_device, storage="split")
    flat = rf.flatten_rays(rf.cast_rays(intr, poses[0], hip_device))
    with torch.no_grad():
        model.render_rays(flat)  # builds the shadow
        M = rf.node_max_weights(grid, poses[:1], intr, bounds, nm.SCENE_SAMPLES)
        # one view only: what it does not see and the threshold removes changes the render of the SECOND view
        rf.prune_voxel_grid(grid, M, threshold=0.05, dilate=0)
        rf.prune_voxel_grid(twin, M, threshold=0.05, dilate=0)
        other = rf.flatten_rays(rf.cast_rays(intr, poses[2], hip_device))
        a, b = model.render_rays(other), twin_model.render_rays(other)
    assert torch.equal(grid.densities.detach(), twin.densities.detach())
    assert torch.equal(a.colour, b.colour) and torch.equal(a.depth, b.depth)

    class Foreign(torch.nn.Module):  # the reference VoxelGrid's attribute names, nothing else
        def __init__(self, src):
            super().__init__()
            self.densities, self.features = torch.nn.Parameter(src.densities.detach().clone()), torch.nn.Parameter(src.features.detach().clone())
            self.aabb, self._expected_density_scale = src.aabb, src.expected_density_scale
            self._density_preactivation, self._density_postactivation = torch.nn.Identity(), torch.nn.ReLU()

    fresh, *_ = scene_setup(hip_device, storage="reference")
    foreign = Foreign(fresh)
    Mf = rf.node_max_weights(foreign, poses[:1], intr, bounds, nm.SCENE_SAMPLES)
    assert torch.equal(Mf, M)
    rf.prune_voxel_grid(foreign, Mf, threshold=0.05, dilate=0)
    assert torch.equal(foreign.densities.detach(), grid.densities.detach())


# --------------------------------------------------------------------------------------------
# integration
# --------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, result_dir):
    import os

    from thr3ed_atom_amd import distributed as rfdist

    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    rfdist.init_from_env(backend="gloo")
    dev = torch.device("cuda:0")
    grid, model, intr, poses, bounds = scene_setup(dev)
    M = rf.node_max_weights(model, poses, intr, bounds, nm.SCENE_SAMPLES)
    np.save(os.path.join(result_dir, f"M{rank}.npy"), M.cpu().numpy())
    torch.distributed.destroy_process_group()


def test_two_gloo_ranks_give_the_single_process_statistic_bit_for_bit(hip_device, tmp_path):
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    grid, model, intr, poses, bounds = scene_setup(hip_device)
    single = rf.node_max_weights(model, poses, intr, bounds, nm.SCENE_SAMPLES).cpu().numpy()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        assert np.array_equal(np.load(tmp_path / f"M{rank}.npy").view(np.uint32), single.view(np.uint32))


def _training_scene(dev):
    cam = hotdog_like_camera()
    gd, gf = sparse_scene_grid((16, 16, 16), 3, 11)
    gt = rf.VoxelGrid((gd * 3.0).to(dev), gf.to(dev), rf.VoxelSize(3.0 / 16, 3.0 / 16, 3.0 / 16), density_preactivation=torch.nn.Identity(),
                      density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False)
    bounds = rf.CameraBounds(cam["near"], cam["far"])
    cfg = rf.SHVoxGridRenderConfig(32, bounds, perturb_sampled_points=False, white_bkgd=True)
    gt_model = rf.VolumetricModel(gt, rf.render_sh_voxel_grid, cfg, device=dev)
    intr = rf.CameraIntrinsics(24, 24, 33.0)
    poses = [rf.pose_spherical(90.0 * k, -30.0, cam["radius"]) for k in range(4)]
    images = torch.stack([gt_model.render(p, intr).colour.permute(2, 0, 1) for p in poses])
    pose_mat = torch.stack([torch.cat([p.rotation, p.translation], dim=1) for p in poses]).to(dev)
    return PosedImagesInMemory(images, pose_mat, intr, bounds), cfg


def _train(dev, data, cfg, **kwargs):
    torch.manual_seed(3)
    d0, f0 = procedural_grid((16, 16, 16), 3, 77)
    grid = rf.VoxelGrid(d0.to(dev), f0.to(dev), rf.VoxelSize(3.0 / 16, 3.0 / 16, 3.0 / 16), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    history = []
    model = train_sh_vox_grid_vol_mod_with_posed_images(model, data, None, ray_batch_size=256, num_stages=2, num_iterations_per_stage=12, image_batch_cache_size=4,
                                                        learning_rate=0.03, lr_decay_steps_per_stage=10, summary_freq=100, log=lambda s: None, history=history, **kwargs)
    g = model.thre3d_repr
    return g.densities.detach().clone(), g.features.detach().clone(), history


def test_the_trainer_prunes_per_stage_and_is_untouched_when_off(hip_device, monkeypatch):
    data, cfg = _training_scene(hip_device)
    dens_on, _, history = _train(hip_device, data, cfg, prune_threshold=1e-3, prune_dilate=1)
    rows = [h for h in history if "pruned_nodes" in h]
    assert [r["stage"] for r in rows] == [1, 2]  # 8^3 before the upsampling, 16^3 after the last stage
    assert rows[0]["pruned_nodes"] + rows[0]["kept_nodes"] == 8**3 and rows[1]["pruned_nodes"] + rows[1]["kept_nodes"] == 16**3
    assert rows[1]["pruned_nodes"] > 0 and int((dens_on[..., 0] <= 0).sum()) >= rows[1]["pruned_nodes"]
    # off: the parent's code path -- the same bits as a run without the arguments, and nothing of the feature is launched
    plain = _train(hip_device, data, cfg)

    def forbidden(*args, **kwargs):
        raise AssertionError("a pruning launch in a run with prune_threshold=None")

    monkeypatch.setattr(ops, "node_max_weight_raw", forbidden)
    monkeypatch.setattr(ops, "prune_grid_raw", forbidden)
    off = _train(hip_device, data, cfg, prune_threshold=None, prune_dilate=3)
    again = _train(hip_device, data, cfg)
    if torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1]):
        assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    else:  # (the binned adjoint orders a brick's records by atomic timing: where the parent's own runs differ in bits, so may this one)
        spread = max(float((again[i] - plain[i]).abs().max()) for i in (0, 1))
        assert max(float((off[i] - plain[i]).abs().max()) for i in (0, 1)) <= 4 * spread
    assert not any("pruned_nodes" in h for h in off[2]) and len(off[2]) == len(plain[2])
    assert not torch.equal(dens_on, plain[0])


def test_cli_train_prune_render_round_trip(hip_device, tmp_path):
    """scripts/train_sh_based_voxel_grid.py with --prune_threshold, scripts/prune_sh_based_voxel_grid.py on its checkpoint (the
    train script's data options), scripts/render_sh_based_voxel_grid.py on the pruned checkpoint."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)

    def run(args):
        return subprocess.run([sys.executable] + args, cwd=root, env=env, capture_output=True, text=True, timeout=600)

    out = tmp_path / "run"
    data = ["--synthetic", "True", "--synthetic_size", "32", "--train_num_samples_per_ray", "48"]
    r = run(["scripts/train_sh_based_voxel_grid.py", "-o", str(out), "--grid_dims", "16", "16", "16", "--sh_degree", "0", "--ray_batch_size", "1024",
             "--render_num_samples_per_ray", "48", "--num_stages", "2", "--num_iterations_per_stage", "15", "--save_frequency", "1000", "--test_frequency", "1000",
             "--summary_frequency", "10", "--prune_threshold", "1e-3", "--prune_dilate", "1"] + data)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "after stage 1" in r.stdout and "after stage 2" in r.stdout
    ckpt, pruned = out / "saved_models" / "model_final.pth", tmp_path / "pruned.pth"
    r = run(["scripts/prune_sh_based_voxel_grid.py", "-i", str(ckpt), "-o", str(pruned), "--threshold", "0.02", "--dilate", "0"] + data)
    assert r.returncode == 0, r.stderr[-2000:]
    kept, gone = (int(r.stdout.split(f"{word} nodes: ")[1].split()[0]) for word in ("kept", "pruned"))
    before, after = (int(v) for v in r.stdout.split("occupied cells: ")[1].split()[0:3:2])
    assert kept + gone == 16**3 and gone > 0 and after <= before
    a, _ = rf.create_volumetric_model_from_saved_model(ckpt, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    b, _ = rf.create_volumetric_model_from_saved_model(pruned, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    da, db = a.thre3d_repr.densities.detach(), b.thre3d_repr.densities.detach()
    assert bool((db <= da).all()) and int((db != da).sum()) <= gone and torch.equal(a.thre3d_repr.features.detach(), b.thre3d_repr.features.detach())
    frames = tmp_path / "frames"
    r = run(["scripts/render_sh_based_voxel_grid.py", "-i", str(pruned), "-o", str(frames), "--overridden_num_samples_per_ray", "48", "--camera_path", "thre360",
             "--num_frames", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(os.listdir(frames)) == 2
