"""Surface normals and quantile depth on the GPU: rf_render_geometry against the float64 model (tests/geometry_model.py), its exact
properties, a cross-check against rf_grid_query_backward_points, its error paths, and the layers above it (ops.render_geometry,
VolumetricModel.render_geometry, back_project_points, the two scripts)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import geometry_model as gm
from tests.helpers import hash_uniform
from thr3ed_atom_amd import _lib, ops
from thr3ed_atom_amd.constants import EXTRA_ACCUMULATED_WEIGHTS, EXTRA_NORMALS
from thr3ed_atom_amd.voxels import brick_nodes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIVATIONS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
               "abs": (torch.abs, torch.nn.Identity()), "identity": (torch.nn.Identity(), torch.nn.Identity())}
WORST = {"normal": 0.0}  # the largest |N - N64| / bound_r met (printed per case)


def T(a):
    return torch.from_numpy(np.asarray(a))


def make_grid(dev, dens, feat, dims, storage, mode, rho=None, voxel=None):
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*(voxel or gm.voxel_of(dims))), density_preactivation=ACTIVATIONS[mode][0],
                        density_postactivation=ACTIVATIONS[mode][1], expected_density_scale=gm.rho_of(mode) if rho is None else rho, tunable=False, storage=storage)


def poison_padding(grid):
    """NaN in the padding nodes of bricked storage: never read"""
    if grid.storage == "bricked":
        X, Y, Z = grid.grid_dims
        for t in grid.kernel_tensors():
            if t is not None:
                real = brick_nodes(torch.ones((X, Y, Z, 1), device=t.device))
                t.data[(real == 0).expand_as(t)] = float("nan")


def batch_of(dev, dims, o, d, S, near, far, option, first_ray=0, count=None):
    """(RayBatch, flags) of a case's option; the two flags the pass must ignore ride along on odd S"""
    flags, jitter, camera = 0, None, None
    if option == "aabb":
        flags |= _lib.FLAG_AABB_SAMPLING
    if option == "occupancy":
        flags |= _lib.FLAG_OCCUPANCY_SKIP
    if option == "t_rand":
        jitter = gm.case_jitter(S, option)[first_ray : first_ray + (count or gm.RAYS)].to(dev).contiguous()
    if option == "keyed":
        jitter = ops.KeyedJitter(gm.JITTER_KEY, gm.JITTER_FIRST + first_ray)
    flags |= (_lib.FLAG_WHITE_BKGD | _lib.FLAG_RENDER_DIFFUSE) if S % 2 else 0
    if option == "camera":
        pose = gm.camera_pose()
        camera = (gm.CAMERA_HW[0], gm.CAMERA_HW[1], gm.CAMERA_FOCAL[dims], pose.rotation, pose.translation)
        return ops.RayBatch(None, None, S, near, far, camera=camera, first_ray=first_ray, num_rays=count), flags
    hi = first_ray + (count or o.shape[0] - first_ray)
    return ops.RayBatch(o[first_ray:hi].to(dev).contiguous(), d[first_ray:hi].to(dev).contiguous(), S, near, far, t_rand=jitter), flags


def launch(grid, batch, flags, n, quantile=gm.QUANTILE, fill=float("nan")):
    """one rf_render_geometry launch on NaN-filled buffers: (N [n,3], depth [n], acc [n]) on the device"""
    dev = grid.kernel_tensors()[0].device
    normal, depth, acc = (torch.full(shape, fill, device=dev) for shape in ((n, 3), (n,), (n,)))
    ops.render_geometry_raw(grid, batch, flags, quantile, normal, depth, acc)
    return normal, depth, acc


def case_launch(dev, dims, storage, S, F, mode, option, quantile=gm.QUANTILE):
    dens, feat = gm.blob_grid(dims, F, mode)
    o, d, near, far = gm.case_rays(dims, S, option)
    grid = make_grid(dev, dens, feat, dims, storage, mode)
    if option == "occupancy":
        grid.build_occupancy()
    poison_padding(grid)
    batch, flags = batch_of(dev, dims, o, d, S, near, far, option)
    return launch(grid, batch, flags, gm.RAYS, quantile)


def test_the_case_table_meets_every_value_of_every_factor():
    cases = gm.kernel_cases()
    for col, values in ((0, gm.DIMS), (1, gm.STORAGES), (2, gm.SAMPLES), (3, gm.FEATURES), (4, gm.MODES), (5, gm.OPTIONS)):
        assert {c[col] for c in cases} == set(values), col
    assert len(set(cases)) == len(cases) == len(gm.DIMS) * len(gm.STORAGES) * len(gm.SAMPLES)


@pytest.mark.parametrize("dims,storage,S,F,mode,option", gm.kernel_cases(), ids=gm.case_id)
def test_kernel_equals_the_float64_model(hip_device, dims, storage, S, F, mode, option):
    """|acc - acc64| <= TOL on every ray; |N - N64|_inf <= bound_r on every ray whose bound is at most 1e-3; the quantile depth within
    1e-5 max(1, |z|) of the float32 ray parameter of the model's crossing sample, 0 where the model has none, on every ray whose
    crossing is not within 1e-5 of a sample's opacity.  The two sets of rays left out are the MODEL's (their sizes are capped over
    the table by tests/test_geometry_model.py: 2 % of the weighted rays, 1 % of the rays); rays that miss the box give exact zeros;
    the features keep out of it (NaN in the padding of bricked storage is never read)."""
    ref = gm.case_reference(dims, F, mode, S, option)
    normal, depth, acc = (t.cpu().numpy().astype(np.float64) for t in case_launch(hip_device, dims, storage, S, F, mode, option))
    assert np.isfinite(normal).all() and np.isfinite(depth).all() and np.isfinite(acc).all()
    err_acc = np.abs(acc - ref["acc"])
    err_n = np.abs(normal - ref["normal"]).max(-1)
    tight = ref["bound"] <= gm.BOUND_CAP
    ratio = float((err_n[tight] / ref["bound"][tight]).max())
    sure = ~ref["ambiguous"]
    err_z = np.abs(depth - ref["depth"]) / np.maximum(1.0, np.abs(ref["depth"]))
    WORST["normal"] = max(WORST["normal"], ratio)
    print(f"geometry {gm.case_id(dims)} {storage} S={S} F={F} {mode} {option}: max |acc - acc64| = {err_acc.max():.3e}, max |N - N64| / bound = {ratio:.3f} "
          f"(largest bound {ref['bound'][tight].max():.2e}; {int((~tight).sum())} rays above the cap), max depth error {err_z[sure].max():.3e} "
          f"({int((~sure).sum())} ambiguous crossings, {int((ref['istar'] >= 0).sum())} crossings); worst ratio so far {WORST['normal']:.3f}")
    assert (err_acc <= gm.TOL).all(), err_acc.max()
    assert (err_n[tight] <= ref["bound"][tight]).all(), ratio
    assert (err_z[sure] <= 1e-5).all(), err_z[sure].max()
    assert (depth[sure & (ref["istar"] < 0)] == 0).all()
    missed = ~ref["inside"].any(-1)
    assert missed.sum() >= 1 or S == 1
    assert not normal[missed].any() and not depth[missed].any() and not acc[missed].any()
    assert (np.linalg.norm(normal, axis=-1) > 0.5).any() and (depth != 0).any()  # not vacuous


@pytest.fixture(scope="module")
def property_case(hip_device):
    """one case for the exact properties: (9, 10, 17), F = 27, ReLU, S = 130, keyed jitter -- its three outputs per storage"""
    dims, S, F, mode, option = (9, 10, 17), 130, 27, "relu", "keyed"
    outs = {st: case_launch(hip_device, dims, st, S, F, mode, option) for st in gm.STORAGES}
    return dims, S, F, mode, option, outs


def test_two_runs_are_bit_identical(hip_device, property_case):
    dims, S, F, mode, option, outs = property_case
    for storage in gm.STORAGES:
        again = case_launch(hip_device, dims, storage, S, F, mode, option)
        for a, b in zip(again, outs[storage]):
            assert torch.equal(a, b)


def test_storages_agree_bit_for_bit_on_acc_and_depth(property_case):
    outs = property_case[-1]
    for storage in ("split", "bricked"):
        assert torch.equal(outs[storage][2], outs["reference"][2]) and torch.equal(outs[storage][1], outs["reference"][1])
        assert float((outs[storage][0] - outs["reference"][0]).abs().max()) <= 1e-6  # (the same formulas on the same values)


@pytest.mark.parametrize("storage,option,S", [("reference", "plain", 65), ("split", "t_rand", 130), ("bricked", "keyed", 64), ("split", "aabb", 63),
                                               ("split", "occupancy", 130)])
def test_acc_is_the_per_ray_forward_kernels_acc(hip_device, storage, option, S):
    """ray lists go to the per-ray forward kernel: its accumulated weight, bit for bit"""
    dims, F, mode = (9, 10, 17), 27, "relu"
    dens, feat = gm.blob_grid(dims, F, mode)
    o, d, near, far = gm.case_rays(dims, S, option)
    grid = make_grid(hip_device, dens, feat, dims, storage, mode)
    batch, flags = batch_of(hip_device, dims, o, d, S, near, far, option)
    if option == "occupancy":
        grid.build_occupancy()
    _, _, acc = launch(grid, batch, flags, gm.RAYS)
    with torch.no_grad():
        fwd = ops.relu_field_render(grid, batch.origins, batch.directions, S, near, far, t_rand=batch.t_rand, optimized_sampling=(option == "aabb"),
                                    use_occupancy=(option == "occupancy"))
    assert float(acc.max()) > 0.5 and torch.equal(acc, fwd[2].reshape(-1))


@pytest.mark.parametrize("jitter", [False, True])
def test_chunks_of_a_frame_equal_the_whole_frame(hip_device, jitter):
    dims, S, F, mode = (9, 10, 17), 65, 3, "relu"
    dens, feat = gm.blob_grid(dims, F, mode)
    grid = make_grid(hip_device, dens, feat, dims, "split", mode)
    _, _, near, far = gm.case_rays(dims, S, "camera")
    pose = gm.camera_pose()
    camera = (gm.CAMERA_HW[0], gm.CAMERA_HW[1], gm.CAMERA_FOCAL[dims], pose.rotation, pose.translation)
    key = ops.KeyedJitter(gm.JITTER_KEY, 0) if jitter else None

    def part(lo, count):
        return launch(grid, ops.RayBatch(None, None, S, near, far, t_rand=key, camera=camera, first_ray=lo, num_rays=count), 0, count)

    whole = part(0, gm.RAYS)
    assert float(whole[2].max()) > 0.5
    pieces = [part(0, 37), part(37, 1), part(38, 58)]
    for k in range(3):
        assert torch.equal(torch.cat([p[k] for p in pieces]), whole[k])
    # ... and the in-kernel rays are cast_rays' rays: the same frame from a ray list
    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(*camera[:3]), pose, hip_device))
    listed = launch(grid, ops.RayBatch(rays.origins.contiguous(), rays.directions.contiguous(), S, near, far, t_rand=key), 0, gm.RAYS)
    for a, b in zip(listed, whole):
        assert torch.equal(a, b)


@pytest.mark.parametrize("storage", gm.STORAGES)
def test_occupancy_mask_under_relu_changes_no_bit(hip_device, storage):
    dims, S, F, mode = (9, 10, 17), 130, 27, "relu"
    dens, feat = gm.blob_grid(dims, F, mode)
    o, d, near, far = gm.case_rays(dims, S, "plain")
    grid = make_grid(hip_device, dens, feat, dims, storage, mode)
    plain = launch(grid, *batch_of(hip_device, dims, o, d, S, near, far, "plain"), gm.RAYS)
    grid.build_occupancy(0.0)
    masked = launch(grid, *batch_of(hip_device, dims, o, d, S, near, far, "occupancy"), gm.RAYS)
    for a, b in zip(plain, masked):
        assert torch.equal(a, b)


def test_quantile_depths_are_monotone_and_leave_the_rest_alone(hip_device):
    """z(0.25) <= z(0.5) <= z(0.75) on every ray where all three are non-zero (and a crossing at a higher quantile implies one at
    every lower one); N and acc do not depend on the quantile"""
    dims, S, F, mode, option = (9, 10, 17), 130, 27, "relu", "t_rand"
    outs = [case_launch(hip_device, dims, "split", S, F, mode, option, quantile=q) for q in (0.25, 0.5, 0.75)]
    z = [o[1] for o in outs]
    all_three = (z[0] != 0) & (z[1] != 0) & (z[2] != 0)
    assert int(all_three.sum()) >= 10
    assert bool((z[0][all_three] <= z[1][all_three]).all()) and bool((z[1][all_three] <= z[2][all_three]).all())
    assert bool((z[0][all_three] < z[2][all_three]).any())  # (the case spreads its weights over several samples)
    assert bool(((z[2] != 0) <= (z[1] != 0)).all()) and bool(((z[1] != 0) <= (z[0] != 0)).all())
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[2], outs[0][2])


def test_an_opaque_first_hit_gives_one_depth_for_every_quantile(hip_device):
    dims, S, F = (9, 10, 17), 65, 3
    _, feat = gm.blob_grid(dims, F, "relu")
    grid = make_grid(hip_device, torch.full(dims + (1,), 1e4), feat, dims, "split", "relu")
    o, d, near, far = gm.case_rays(dims, S, "plain")
    batch, flags = batch_of(hip_device, dims, o, d, S, near, far, "plain")
    z = [launch(grid, batch, flags, gm.RAYS, quantile=q)[1] for q in (0.25, 0.5, 0.75)]
    acc = launch(grid, batch, flags, gm.RAYS)[2]
    hit = acc > 0
    assert int(hit.sum()) >= 48 and bool((acc[hit] == 1.0).all())
    assert torch.equal(z[0], z[1]) and torch.equal(z[1], z[2]) and bool((z[0][hit] > 0).all()) and not bool(z[0][~hit].any())


def test_single_samples_agree_with_the_point_gradient_of_grid_query(hip_device):
    """S = 1 rays whose one sample lies strictly inside a cell: where pre > 0 under ReLU, -N / |N| is parallel to the gradient of the
    activated density with respect to the point (rf_grid_query_backward_points through ops.grid_query): cosine >= 1 - 1e-5."""
    dims, F, mode = (9, 10, 17), 27, "relu"
    dens, feat = gm.blob_grid(dims, F, mode)
    grid = make_grid(hip_device, dens, feat, dims, "reference", mode)
    n = 256
    vox = np.array(gm.voxel_of(dims))
    half = np.array(dims) * vox / 2.0
    # cells around the centre of the box, where the blob is (lower node within [0, dim - 2])
    cells = np.stack([np.clip(np.floor((dims[a] - 1) / 2.0 + hash_uniform((n,), 510 + a, -2.5, 2.5).astype(np.float64)), 0, dims[a] - 2) for a in range(3)], -1)
    frac = hash_uniform((n, 3), 513, 0.2, 0.8).astype(np.float64)
    p = (cells + 0.5 + frac) * vox - half
    near = 4.0
    o_np = 4.0 * p / np.linalg.norm(p, axis=-1, keepdims=True) + hash_uniform((n, 3), 514) * 0.5
    d_np = (p - o_np) / near
    o, d = T(o_np.astype(np.float32)).to(hip_device), T(d_np.astype(np.float32)).to(hip_device)
    normal, _, acc = launch(grid, ops.RayBatch(o, d, 1, near, 6.0), 0, n)
    pts = (o + d * np.float32(near)).detach().requires_grad_(True)
    ops.grid_query(grid, pts)[:, -1].sum().backward()
    g = pts.grad
    open_gate = (acc > 0) & (g.norm(dim=-1) > 0)
    assert int(open_gate.sum()) >= 40
    cos = torch.nn.functional.cosine_similarity(-normal[open_gate].double(), g[open_gate].double(), dim=-1)
    print(f"{int(open_gate.sum())} single samples with an open gate: min cosine - 1 = {float(cos.min()) - 1.0:.2e}")
    assert float(cos.min()) >= 1.0 - 1e-5
    assert bool((acc[open_gate] == 1.0).all()) and float((normal[open_gate].norm(dim=-1) - 1.0).abs().max()) <= 1e-6


def test_error_paths_touch_no_output(hip_device):
    """every code of the contract again, with REAL device buffers behind the pointers: after the refused calls they hold their fill"""
    dims, S, F, mode = (5, 6, 7), 16, 3, "relu"
    dens, feat = gm.blob_grid(dims, F, mode)
    grid = make_grid(hip_device, dens, feat, dims, "reference", mode)
    o, d, near, far = gm.case_rays(dims, S, "plain")
    o, d = o.to(hip_device), d.to(hip_device)
    normal, depth, acc = (torch.full(shape, 7.0, device=hip_device) for shape in ((gm.RAYS, 3), (gm.RAYS,), (gm.RAYS,)))
    lib = _lib.load()
    g = grid.to_rf_grid()
    rb, keep = ops._ray_batch(o, d, S, near, far, None)
    out = _lib.RFGeometryOut()
    out.normal_dev, out.quantile_depth_dev, out.acc_dev = normal.data_ptr(), depth.data_ptr(), acc.data_ptr()
    stream = torch.cuda.current_stream(hip_device).cuda_stream
    call = lambda g_, r_, o_, flags=0, q=0.5: lib.rf_render_geometry(g_, r_, flags, q, o_, stream)  # noqa: E731
    assert call(None, C.byref(rb), C.byref(out)) == -1 and call(C.byref(g), None, C.byref(out)) == -1 and call(C.byref(g), C.byref(rb), None) == -1
    assert call(C.byref(g), C.byref(rb), C.byref(_lib.RFGeometryOut())) == -1
    assert call(C.byref(g), C.byref(rb), C.byref(out), flags=_lib.FLAG_OCCUPANCY_SKIP) == -1
    for q in (0.0, 1.0, float("nan"), float("inf"), -0.5):
        assert call(C.byref(g), C.byref(rb), C.byref(out), q=q) == -2
    rb.num_samples = 0
    assert call(C.byref(g), C.byref(rb), C.byref(out)) == -2
    rb.num_samples = S
    g.density_mode = 9
    assert call(C.byref(g), C.byref(rb), C.byref(out)) == -3
    g.density_mode, g.num_features = 0, 5
    assert call(C.byref(g), C.byref(rb), C.byref(out)) == -3
    g.num_features = F
    rb.num_rays = 0
    assert call(C.byref(g), C.byref(rb), C.byref(out)) == 0
    torch.cuda.synchronize()
    for t in (normal, depth, acc):
        assert bool((t == 7.0).all())
    # the host layer: wrong buffers raise before the call; each output alone is enough
    with pytest.raises(ValueError, match="normal"):
        ops.render_geometry_raw(grid, ops.RayBatch(o, d, S, near, far), 0, 0.5, normal[:5], None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_geometry_raw(grid, ops.RayBatch(o, d, S, near, far), 0, 0.5, None, None, acc.cpu())
    rb.num_rays = gm.RAYS
    ops.render_geometry_raw(grid, ops.RayBatch(o, d, S, near, far), 0, 0.5, None, depth, None)
    assert bool((normal == 7.0).all()) and bool((acc == 7.0).all()) and not bool((depth == 7.0).any())
    del keep


# --------------------------------------------------------------------------------------------
# the layers above
# --------------------------------------------------------------------------------------------
def blob_model(dev, storage="split", S=65, perturb=False, chunk=32768):
    dims, F, mode = (9, 10, 17), 27, "relu"
    dens, feat = gm.blob_grid(dims, F, mode)
    grid = make_grid(dev, dens, feat, dims, storage, mode)
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(2.0, 6.0), perturb_sampled_points=perturb, parallel_rays_chunk_size=chunk)
    return rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)


@pytest.mark.parametrize("storage", gm.STORAGES)
def test_model_frame_equals_render_geometry_on_cast_rays(hip_device, storage):
    model = blob_model(hip_device, storage, chunk=50)  # (the frame goes in chunks of 50 pixels)
    pose, intr = gm.camera_pose(), rf.CameraIntrinsics(11, 13, 16.0)
    out = model.render_geometry(pose, intr, quantile=0.4, optimized_sampling=True)
    assert out.colour is None and out.depth.shape == (11, 13, 1) and sorted(out.extra) == sorted([EXTRA_NORMALS, EXTRA_ACCUMULATED_WEIGHTS])
    assert out.extra[EXTRA_NORMALS].shape == (11, 13, 3) and out.extra[EXTRA_ACCUMULATED_WEIGHTS].shape == (11, 13, 1)
    assert not out.depth.requires_grad and not out.extra[EXTRA_NORMALS].requires_grad
    rays = rf.flatten_rays(rf.cast_rays(intr, pose, hip_device))
    for target in (model, model.thre3d_repr):
        flat = rf.render_geometry(target, rays, 65, rf.CameraBounds(2.0, 6.0), quantile=0.4, optimized_sampling=True)
        assert flat.colour is None and flat.depth.shape == (143, 1)
        assert torch.equal(flat.depth, out.depth.reshape(-1, 1)) and torch.equal(flat.extra[EXTRA_NORMALS], out.extra[EXTRA_NORMALS].reshape(-1, 3))
        assert torch.equal(flat.extra[EXTRA_ACCUMULATED_WEIGHTS], out.extra[EXTRA_ACCUMULATED_WEIGHTS].reshape(-1, 1))
    assert float(out.extra[EXTRA_ACCUMULATED_WEIGHTS].max()) > 0.5 and float(out.depth.max()) > 2.0
    # the accumulated weight is the ordinary render's
    ordinary = model.render(pose, intr, optimized_sampling=True)
    assert float((ordinary.extra[EXTRA_ACCUMULATED_WEIGHTS] - out.extra[EXTRA_ACCUMULATED_WEIGHTS]).abs().max()) <= 2e-5  # (two kernels, each within 1e-5 of float64)
    with pytest.raises(ValueError, match="Unknown render configuration field"):
        model.render_geometry(pose, intr, no_such_field=3)
    with pytest.raises(ValueError, match="quantile"):
        model.render_geometry(pose, intr, quantile=1.0)
    # jitter: keyed, reproducible from torch's seed, and the mask changes nothing under ReLU
    torch.manual_seed(5)
    a = model.render_geometry(pose, intr, perturb_sampled_points=True)
    torch.manual_seed(5)
    b = model.render_geometry(pose, intr, perturb_sampled_points=True, use_occupancy_mask=True, parallel_rays_chunk_size=7)
    assert torch.equal(a.depth, b.depth) and torch.equal(a.extra[EXTRA_NORMALS], b.extra[EXTRA_NORMALS])
    assert not torch.equal(a.depth, model.render_geometry(pose, intr).depth)


def test_a_foreign_grid_module_renders_its_geometry(hip_device):
    src = blob_model(hip_device, "reference").thre3d_repr

    class Foreign(torch.nn.Module):  # the reference VoxelGrid's attribute names, nothing else
        def __init__(self):
            super().__init__()
            self.densities, self.features = torch.nn.Parameter(src.densities.detach().clone()), torch.nn.Parameter(src.features.detach().clone())
            self.aabb, self._expected_density_scale = src.aabb, src.expected_density_scale
            self._density_preactivation, self._density_postactivation = torch.nn.Identity(), torch.nn.ReLU()

    rays = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(8, 8, 12.0), gm.camera_pose(), hip_device))
    a = rf.render_geometry(Foreign(), rays, 65, (2.0, 6.0))
    b = rf.render_geometry(src, rays, 65, (2.0, 6.0))
    assert torch.equal(a.depth, b.depth) and torch.equal(a.extra[EXTRA_NORMALS], b.extra[EXTRA_NORMALS]) and float(a.depth.max()) > 0


@pytest.mark.parametrize("axis,sign", [(2, 1), (2, -1), (0, 1), (1, -1)])
def test_frame_of_an_opaque_slab(hip_device, axis, sign):
    """A 24 x 24 frame of an axis-aligned opaque slab (nodes 6 .. 9 of 16 on one axis at raw density 1000, -1 elsewhere), seen from
    the +-axis side by a narrow camera: N = +-axis within 1e-4, median depth = the depth of the slab's near face (where the
    interpolated density crosses 0) within one sample spacing."""
    G, S, dist = 16, 128, 4.0
    vox = 3.0 / G
    dens = torch.full((G, G, G, 1), -1.0)
    index = [slice(None)] * 3
    index[axis] = slice(6, 10)
    dens[tuple(index)] = 1000.0
    grid = rf.VoxelGrid(dens.to(hip_device), T(hash_uniform((G, G, G, 3), 9)).to(hip_device), rf.VoxelSize(vox, vox, vox), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False, storage="split")
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(2.0, 6.0), perturb_sampled_points=False)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    # the camera looks along its -z: put the camera's z on sign * axis
    zc = np.zeros(3)
    zc[axis] = sign
    xc = np.zeros(3)
    xc[(axis + 1) % 3] = 1.0
    yc = np.cross(zc, xc)
    pose = rf.CameraPose(T(np.stack([xc, yc, zc], -1).astype(np.float32)), T((dist * zc).astype(np.float32).reshape(3, 1)))
    out = model.render_geometry(pose, rf.CameraIntrinsics(24, 24, 70.0))
    normal, depth, acc = out.extra[EXTRA_NORMALS].cpu().numpy(), out.depth.cpu().numpy()[..., 0], out.extra[EXTRA_ACCUMULATED_WEIGHTS].cpu().numpy()[..., 0]
    assert np.abs(acc - 1.0).max() <= 1e-6
    assert np.abs(normal - zc.astype(np.float32)).max() <= 1e-4, np.abs(normal - zc).max()
    # the near face: between node 9 (1000) and node 10 (-1) on the + side, between node 6 and node 5 on the - side
    node = lambda k: (k + 0.5) * vox - 1.5  # noqa: E731
    face = node(9) + vox * 1000.0 / 1001.0 if sign > 0 else node(6) - vox * 1000.0 / 1001.0
    want = dist - sign * face  # the ray parameter: the direction's component along the view axis is exactly -1
    spacing = 4.0 / (S - 1)
    assert np.abs(depth - want).max() <= spacing and (depth >= want - 1e-5).all(), (depth.min(), depth.max(), want)


@pytest.fixture(scope="module")
def sphere_model(hip_device):
    """32^3 ReLU field D = 30 (R - |p|), R = 0.9: a ball whose surface is opaque within a fraction of a voxel"""
    G, R = 32, 0.9
    vox = 3.0 / G
    ax = (np.arange(G) + 0.5) * vox - 1.5
    dist = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    dens = T((30.0 * (R - dist)).astype(np.float32)[..., None])
    grid = rf.VoxelGrid(dens.to(hip_device), T(hash_uniform((G, G, G, 3), 11)).to(hip_device), rf.VoxelSize(vox, vox, vox), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False, storage="split")
    cfg = rf.SHVoxGridRenderConfig(256, rf.CameraBounds(2.0, 6.0), perturb_sampled_points=False)
    return rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device), R, vox


def test_back_projected_points_lie_on_the_sphere(hip_device, sphere_model):
    model, R, vox = sphere_model
    poses = [rf.pose_spherical(yaw, pitch, 4.0) for yaw, pitch in ((0.0, -30.0), (120.0, -60.0), (240.0, 20.0))]
    intr = rf.CameraIntrinsics(32, 32, 40.0)
    points, normals, colours = rf.back_project_points(model, poses, intr)
    assert points.shape == normals.shape == colours.shape and points.shape[1] == 3 and points.shape[0] > 600
    radius = points.norm(dim=-1)
    assert float((radius - R).abs().max()) <= vox, (float(radius.min()), float(radius.max()))
    assert float((normals.norm(dim=-1) - 1.0).abs().max()) <= 1e-5
    cos = (normals * points / radius[:, None]).sum(-1)
    assert float(cos.min()) >= np.cos(np.deg2rad(15.0)), float(cos.min())
    assert float(colours.min()) >= 0.0 and float(colours.max()) <= 1.0
    # the selection rule: non-zero quantile depth and acc >= min_acc, view by view; a stride thins the pixels
    geo = model.render_geometry(poses[0], intr)
    keep = (geo.depth[..., 0] != 0) & (geo.extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0] >= 0.5)
    one = rf.back_project_points(model, poses[:1], intr)
    assert one[0].shape[0] == int(keep.sum()) and torch.equal(one[0], points[: one[0].shape[0]])
    thin = rf.back_project_points(model, poses[:1], intr, stride=3)
    assert thin[0].shape[0] == int(keep[::3, ::3].sum())
    assert rf.back_project_points(model, poses[:1], intr, min_acc=2.0)[0].shape == (0, 3)


def _run(args, timeout=600):
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def checkpoint(hip_device, tmp_path_factory):
    """a 16^3 ball with the extra info the scripts read"""
    G, R = 16, 0.9
    vox = 3.0 / G
    ax = (np.arange(G) + 0.5) * vox - 1.5
    dist = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    grid = rf.VoxelGrid(T((30.0 * (R - dist)).astype(np.float32)[..., None]).to(hip_device), T(hash_uniform((G, G, G, 3), 12)).to(hip_device), rf.VoxelSize(vox, vox, vox),
                        density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False)
    cfg = rf.SHVoxGridRenderConfig(32, rf.CameraBounds(2.0, 6.0), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    path = tmp_path_factory.mktemp("geometry") / "model.pth"
    torch.save(model.get_save_info(extra_info={"hemispherical_radius": 4.0, "camera_intrinsics": rf.CameraIntrinsics(16, 16, 20.0)}), path)
    return path


def test_render_script_writes_the_geometry_only_with_its_flags(checkpoint, tmp_path):
    common = ["scripts/render_sh_based_voxel_grid.py", "-i", str(checkpoint), "--overridden_num_samples_per_ray", "32", "--render_scale_factor", "1.0", "--num_frames", "3"]  # (a turn-table of num_frames - 1 poses)
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    for out, extra in ((plain, []), (flagged, ["--normals", "--median_depth"])):
        r = _run(common + ["-o", str(out)] + extra)
        assert r.returncode == 0, r.stderr[-2000:]
    frames = sorted(os.listdir(plain))
    assert len(frames) == 2 and all(name.startswith("frame_") for name in frames)
    for name in frames:
        assert (plain / name).read_bytes() == (flagged / name).read_bytes()
    extras = sorted(set(os.listdir(flagged)) - set(frames))
    assert [e.split(".")[0] for e in extras] == ["median_depth_0000", "median_depth_0001", "normal_0000", "normal_0001"]
    depth = np.load(flagged / "median_depth_0000.npy")
    assert depth.shape == (16, 16) and depth.dtype == np.float32 and (depth > 2.0).any() and (depth == 0).any()
    normal = [e for e in extras if e.startswith("normal_0000")][0]
    if normal.endswith(".png"):
        from PIL import Image

        image = np.asarray(Image.open(flagged / normal))
    else:
        image = np.load(flagged / normal)
    assert image.shape == (16, 16, 3) and image.dtype == np.uint8
    assert (image[depth == 0] == 255).all() and (image[8, 8] != 255).any()  # white background outside the ball


def test_export_script_writes_a_point_cloud_without_faces(hip_device, checkpoint, tmp_path):
    cloud = tmp_path / "out" / "cloud.ply"
    r = _run(["scripts/export_point_cloud_from_sh_based_voxel_grid.py", "-i", str(checkpoint), "-o", str(cloud), "--num_views", "2", "--camera_pitch", "40"])
    assert r.returncode == 0, r.stderr[-2000:]
    model, extra = rf.create_volumetric_model_from_saved_model(checkpoint, lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split"), device=hip_device)
    poses = rf.get_thre360_animation_poses(extra["hemispherical_radius"], 40.0, 3)  # (num_poses - 1 yaws)
    points, normals, _ = rf.back_project_points(model, poses, extra["camera_intrinsics"])
    data = cloud.read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii")
    assert f"element vertex {points.shape[0]}\n" in header and "element face" not in header and points.shape[0] > 50
    vdt = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    assert len(data) - end == points.shape[0] * vdt.itemsize
    vert = np.frombuffer(data, vdt, count=points.shape[0], offset=end)
    assert np.array_equal(vert["p"], points.cpu().numpy()) and np.array_equal(vert["n"], normals.cpu().numpy())
    assert f"{points.shape[0]} points" in r.stdout
