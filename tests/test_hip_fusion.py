"""GPU: rf_fuse_depth_views, rf.fuse_depth_views, rf.fuse_field_views and FusedVolume against tests/fusion_model.py on the smallest
inputs at which they can go wrong: slabs whose every quantity is exact in float32 (bit for bit against values written out by hand);
an analytic sphere seen by 8 cameras on lattices of one node, of partial 4 x 4 x 4 blocks and of z columns that cross a wavefront and
a workgroup; 0, 1, 2, 16 and 17 views; images from 1 x 1 pixel upwards; with and without alphas, images and
carving; a camera inside the box, a view with everything behind ``near``, depth images holding 0, NaN and +inf.  Counts are equal and
sums within the bound of docs/fusion_errors.md at every node outside the model's undecidable set.  Then the chain: the depth of
``render_mesh`` of a closed mesh fused and extracted gives a closed mesh that renders the depth it was made from, ``to_voxel_grid``
returns the tsdf at the node centres, and on a field of an opaque ball plus a faint detached blob the fused mesh has one component
where the density's mesh has two and scores the higher mask IoU.

Measured on an MI355X: see docs/fusion_errors.md for the worst ratios of error to bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import fusion_model as fm
from tests import mesh_oracle
from thr3ed_atom_amd import _lib, _marshal

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rf_cameras(cameras, H, W):
    return [_marshal.camera_struct(H, W, cam.focal, cam.rotation, cam.translation) for cam in cameras]


def poses_of(cameras):
    return [rf.CameraPose(torch.from_numpy(np.asarray(cam.rotation, np.float32)), torch.from_numpy(np.asarray(cam.translation, np.float32)).reshape(3, 1)) for cam in cameras]


def on(device, array):
    return None if array is None else torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(device)


def raw_fuse(device, lo, hi, dims, cameras, H, W, depths, alphas=None, images=None, near=0.0, truncation=1.0, min_alpha=0.5, carve=True, state=None):
    """one rf_fuse_depth_views call on fresh (or the given) accumulators: (tsdf_sum [X, Y, Z], counts [X, Y, Z, 2], colour_sum [X, Y, Z, 4] or None)"""
    lib = _lib.load()
    dims = tuple(int(d) for d in dims)
    if state is None:
        state = (torch.zeros(dims, device=device), torch.zeros(dims + (2,), dtype=torch.int32, device=device),
                 torch.zeros(dims + (4,), device=device) if images is not None else None)
    tsdf_sum, counts, colour = state
    cams = rf_cameras(cameras, H, W)
    d, a, im = on(device, depths), on(device, alphas), on(device, images)
    rc = lib.rf_fuse_depth_views(_lib.float3(lo), _lib.float3(hi), (C.c_int32 * 3)(*dims), len(cams), (_lib.RFCamera * max(len(cams), 1))(*cams), _marshal.ptr(d), _marshal.ptr(a),
                                 _marshal.ptr(im), near, truncation, min_alpha, _lib.FUSE_CARVE if carve else 0, tsdf_sum.data_ptr(), counts.data_ptr(), _marshal.ptr(colour),
                                 _marshal.stream(device))
    _lib.check(rc, "rf_fuse_depth_views")
    torch.cuda.synchronize()
    return tsdf_sum, counts, colour


def against_model(model, tsdf_sum, counts, colour, what):
    """counts equal and sums within the bound at every node outside the undecidable set; the worst ratio of error to bound"""
    ok = ~fm.undecidable(model)
    counts = counts.cpu().numpy()
    assert (counts[..., 0][ok] == model.observed[ok]).all() and (counts[..., 1][ok] == model.hidden[ok]).all(), what
    err = np.abs(tsdf_sum.cpu().numpy().astype(np.float64) - model.tsdf_sum)
    assert (err[ok] <= model.bound[ok]).all(), (what, float((err - model.bound)[ok].max()))
    worst = float((err[ok & (model.bound > 0)] / model.bound[ok & (model.bound > 0)]).max()) if (ok & (model.bound > 0)).any() else 0.0
    if model.colour_sum is not None:
        got = colour.cpu().numpy().astype(np.float64)
        assert (got[..., 3][ok] == model.colour_sum[..., 3][ok]).all(), what
        assert (np.abs(got - model.colour_sum).max(-1)[ok] <= model.colour_bound[ok]).all(), what
    else:
        assert colour is None or not bool(colour.any())
    return worst, int((~ok).sum())


# ------------------------------------------------------------------------------------------------------------------- exactness

@pytest.mark.parametrize("axis", [2, 0, 1])
def test_exact_cases_bit_for_bit(hip_device, axis):
    lo, hi, dims, cams, H, W, depths, images, trunc, _ = fm.exact_case(axis)
    for carve, sums, observed, tsdf in ((True, fm.EXACT_SUM_CARVE, fm.EXACT_OBSERVED_CARVE, fm.EXACT_TSDF_CARVE), (False, fm.EXACT_SUM_PLAIN, fm.EXACT_OBSERVED_PLAIN, fm.EXACT_TSDF_PLAIN)):
        tsdf_sum, counts, colour = raw_fuse(hip_device, lo, hi, dims, cams, H, W, depths, None, images, 0.0, trunc, 0.5, carve)
        assert np.array_equal(tsdf_sum.cpu().numpy(), fm.exact_expected(axis, sums).astype(np.float32))
        assert np.array_equal(counts[..., 0].cpu().numpy(), fm.exact_expected(axis, observed)) and np.array_equal(counts[..., 1].cpu().numpy(), fm.exact_expected(axis, fm.EXACT_HIDDEN))
        got = colour.cpu().numpy()
        count = fm.exact_expected(axis, fm.EXACT_COLOUR_COUNT)
        assert np.array_equal(got[..., 3], count.astype(np.float32))
        assert (got[..., :3][count > 0] == np.array(fm.EXACT_COLOUR_SUM, np.float32)).all() and (got[..., :3][count == 0] == 0).all()
        volume = rf.fuse_depth_views(on(hip_device, depths), poses_of(cams), rf.CameraIntrinsics(H, W, 16.0), lo, hi, dims, truncation=trunc, images=on(hip_device, images), carve=carve)
        want_sum, want_seen = fm.exact_expected(axis, sums).astype(np.float32), fm.exact_expected(axis, observed)
        assert np.array_equal(volume.tsdf.cpu().numpy(), np.where(want_seen > 0, want_sum / np.maximum(want_seen, 1).astype(np.float32), np.float32(-1.0)))  # (float32 division)
        np.testing.assert_allclose(volume.tsdf.cpu().numpy(), fm.exact_expected(axis, tsdf), rtol=0, atol=2.0 ** -24)
        assert np.array_equal(volume.observed.cpu().numpy(), fm.exact_expected(axis, observed)) and np.array_equal(volume.hidden.cpu().numpy(), fm.exact_expected(axis, fm.EXACT_HIDDEN))
        assert np.array_equal(volume.colour_count.cpu().numpy(), count) and volume.colour.shape == tuple(dims) + (3,)
        assert (volume.colour.cpu().numpy()[count > 0] == np.float32(0.5)).all() and (volume.colour.cpu().numpy()[count == 0] == 0).all()
        assert volume.truncation == trunc and volume.aabb_min == lo and volume.aabb_max == hi


# ------------------------------------------------------------------------------------------------- the sphere against the model

DIMS = [fm.SPHERE_DIMS, (1, 1, 1), (2, 3, 5), (3, 2, 65), (1, 1, 257), (5, 4, 4)]
OPTIONS = [dict(alphas=True, images=True, carve=True), dict(alphas=False, images=False, carve=True), dict(alphas=True, images=False, carve=False),
           dict(alphas=False, images=True, carve=False)]


def run_both_ways(device, case, alphas=True, images=True, carve=True, near=0.0, min_alpha=0.5):
    """the raw entry point and rf.fuse_depth_views (the same sums, finalised), against the model"""
    lo, hi, dims, cams, H, W, depths, al, im, trunc = case
    al, im = (al if alphas else None), (im if images else None)
    model = fm.fuse(lo, hi, dims, cams, H, W, depths, al, im, near, trunc, min_alpha, carve)
    state = None
    for first in range(0, max(len(cams), 1), 16):  # (the entry point takes 16 views)
        chunk = slice(first, first + 16)
        state = raw_fuse(device, lo, hi, dims, cams[chunk], H, W, depths[chunk], None if al is None else al[chunk], None if im is None else im[chunk], near, trunc, min_alpha,
                         carve, state=state)
    s0, c0, k0 = state
    worst, skipped = against_model(model, s0, c0, k0, (dims, H, W, alphas, images, carve))
    focal = cams[0].focal if cams else 10.0
    volume = rf.fuse_depth_views(on(device, depths), poses_of(cams), rf.CameraIntrinsics(H, W, focal), lo, hi, dims, truncation=trunc, alphas=on(device, al), images=on(device, im),
                                 min_alpha=min_alpha, near=near, carve=carve)
    assert torch.equal(volume.observed, c0[..., 0]) and torch.equal(volume.hidden, c0[..., 1]) and volume.tsdf.shape == tuple(dims) and volume.tsdf.dtype == torch.float32
    seen = c0[..., 0] > 0
    assert torch.equal(volume.tsdf[seen], (s0 / c0[..., 0].clamp(min=1))[seen])
    assert bool((volume.tsdf[~seen & (c0[..., 1] > 0)] == -1.0).all()) and bool((volume.tsdf[~seen & (c0[..., 1] == 0)] == 1.0).all())
    assert float(volume.tsdf.abs().max()) <= 1.0
    assert (volume.colour is None) == (im is None)
    if im is not None:
        assert torch.equal(volume.colour_count, k0[..., 3].to(torch.int32))
        has = k0[..., 3] > 0
        assert torch.equal(volume.colour[has], (k0[..., :3] / k0[..., 3:].clamp(min=1.0))[has]) and not bool(volume.colour[~has].any())
    return worst, skipped, model


@pytest.mark.parametrize("dims", DIMS)
def test_sphere_on_every_lattice_shape(hip_device, dims):
    case = fm.sphere_case(dims=dims)
    for options in OPTIONS:
        worst, skipped, model = run_both_ways(hip_device, case, **options)
        print(f"fusion {dims} {options}: worst tsdf_sum error / bound {worst:.4f}, {skipped} of {model.observed.size} nodes undecidable")
    if dims == fm.SPHERE_DIMS:
        assert int(model.observed.sum()) > 0 and int(model.hidden.sum()) > 0


@pytest.mark.parametrize("views", [0, 1, 2, 16, 17])
def test_view_counts_and_chunks(hip_device, views):
    case = fm.sphere_case(dims=(7, 6, 5), views=views)
    lo, hi, dims, cams, H, W, depths, al, im, trunc = case
    worst, skipped, model = run_both_ways(hip_device, case)
    if views == 0:
        assert not model.observed.any()
        empty = raw_fuse(hip_device, lo, hi, dims, [], H, W, None, None, None, 0.0, trunc)
        assert not bool(empty[0].any()) and not bool(empty[1].any())
    if views == 17:
        # 17 views through the Python layer (16 + 1) = the raw entry point on 16 views, then on 1 more over the same accumulators
        state = raw_fuse(hip_device, lo, hi, dims, cams[:16], H, W, depths[:16], al[:16], im[:16], 0.0, trunc)
        state = raw_fuse(hip_device, lo, hi, dims, cams[16:], H, W, depths[16:], al[16:], im[16:], 0.0, trunc, state=state)
        volume = rf.fuse_depth_views(on(hip_device, depths), poses_of(cams), rf.CameraIntrinsics(H, W, cams[0].focal), lo, hi, dims, truncation=trunc, alphas=on(hip_device, al),
                                     images=on(hip_device, im))
        seen = state[1][..., 0] > 0
        assert torch.equal(volume.observed, state[1][..., 0]) and torch.equal(volume.hidden, state[1][..., 1])
        assert torch.equal(volume.tsdf[seen], (state[0] / state[1][..., 0].clamp(min=1))[seen]) and torch.equal(volume.colour_count, state[2][..., 3].to(torch.int32))
        against_model(model, *state, "16 + 1")
        with pytest.raises(RuntimeError, match="rf_fuse_depth_views"):  # the entry point itself takes 16
            raw_fuse(hip_device, lo, hi, dims, cams, H, W, depths, al, im, 0.0, trunc)


@pytest.mark.parametrize("image", [(1, 1, 0.4), (1, 7, 3.0), (5, 1, 2.0), (2, 2, 1.0), (33, 29, 30.0)])
def test_image_sizes(hip_device, image):
    worst, skipped, model = run_both_ways(hip_device, fm.sphere_case(dims=(6, 5, 9), image=image, views=3))
    assert int(model.observed.sum()) > 0
    print(f"fusion image {image}: worst tsdf_sum error / bound {worst:.4f}, {skipped} nodes undecidable")


def test_degenerate_views(hip_device):
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case(dims=(8, 7, 6), views=4)
    # a camera inside the box (nodes behind it, nodes at its own depth 0 and nodes that project far outside the image)
    inside = fm.look_at((0.05, -0.1, 0.02), target=(1.0, 0.3, 0.2))._replace(focal=cams[0].focal)
    cams = [inside] + cams[1:]
    depths = depths.copy()
    depths[0] = 0.7
    depths[1, ::2, ::3], depths[1, 1::2, 1::3], depths[2, :, ::2] = np.nan, np.inf, 0.0  # no information, no information, a miss
    depths[3, ::3] = -np.inf
    case = (lo, hi, dims, cams, H, W, depths, al, im, trunc)
    for options in OPTIONS:
        worst, skipped, model = run_both_ways(hip_device, case, **options)
    # everything behind near: nothing is counted, nothing is written but what was loaded
    far = run_both_ways(hip_device, case, near=10.0)[2]
    assert not far.observed.any() and not far.hidden.any()
    state = (torch.full(dims, 0.25, device=hip_device), torch.full(dims + (2,), 3, dtype=torch.int32, device=hip_device), torch.full(dims + (4,), 2.0, device=hip_device))
    out = raw_fuse(hip_device, lo, hi, dims, cams, H, W, depths, al, im, 10.0, trunc, state=state)
    assert bool((out[0] == 0.25).all()) and bool((out[1] == 3).all()) and bool((out[2] == 2.0).all())
    # alphas on the threshold: A < min_alpha is the miss, A == min_alpha the hit
    edge = np.full_like(al, 0.5)
    run_both_ways(hip_device, (lo, hi, dims, cams, H, W, depths, edge, im, trunc), min_alpha=0.5)
    run_both_ways(hip_device, (lo, hi, dims, cams, H, W, depths, edge, im, trunc), min_alpha=0.75)


def test_two_calls_give_identical_bits(hip_device):
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case()
    first = raw_fuse(hip_device, lo, hi, dims, cams, H, W, depths, al, im, 0.0, trunc)
    second = raw_fuse(hip_device, lo, hi, dims, cams, H, W, depths, al, im, 0.0, trunc)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    args = (on(hip_device, depths), poses_of(cams), rf.CameraIntrinsics(H, W, cams[0].focal), lo, hi, dims)
    one, two = rf.fuse_depth_views(*args, alphas=on(hip_device, al), images=on(hip_device, im)), rf.fuse_depth_views(*args, alphas=on(hip_device, al), images=on(hip_device, im))
    assert torch.equal(one.tsdf, two.tsdf) and torch.equal(one.colour, two.colour) and torch.equal(one.observed, two.observed)
    # the default truncation: 3 x the longest voxel edge
    assert one.truncation == float(np.float32(trunc))


def test_argument_errors(hip_device):
    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case(dims=(4, 4, 4), views=2)
    d, a, i, poses, intr = on(hip_device, depths), on(hip_device, al), on(hip_device, im), poses_of(cams), rf.CameraIntrinsics(H, W, 36.0)
    assert rf.fuse_depth_views([d[0], d[1]], poses, intr, lo, hi, dims, alphas=a[..., None], images=[i[0], i[1]]).tsdf.shape == (4, 4, 4)  # lists and [H, W, 1] are taken
    for kwargs in (dict(truncation=0.0), dict(truncation=float("nan")), dict(truncation=-1.0), dict(min_alpha=1.5), dict(min_alpha=-0.1), dict(near=-1.0), dict(near=float("inf"))):
        with pytest.raises(ValueError):
            rf.fuse_depth_views(d, poses, intr, lo, hi, dims, **kwargs)
    for bad_lo, bad_hi, bad_dims in ((hi, lo, dims), ((float("nan"), 0, 0), hi, dims), (lo, hi, (0, 4, 4)), (lo, hi, (4, 4, 4097)), (lo, hi, (4, 4)), (lo, hi, (4, 4, 2.5)), (lo, hi, (2048, 2048, 512)),
                                     ((-1, -1), hi, dims), ((-1.0, 1.0, -1.0), (1.0, 1.0, 1.0), dims)):
        with pytest.raises(ValueError):
            rf.fuse_depth_views(d, poses, intr, bad_lo, bad_hi, bad_dims)
    for dd, aa, ii, pp in ((d[:1], None, None, poses), (d, a[:1], None, poses), (d, None, i[:1], poses), (d, None, None, poses[:1]), (d[:, :-1], None, None, poses), (d, a[:, :, :-1], None, poses),
                           (d, None, i[..., :2], poses)):
        with pytest.raises(ValueError):
            rf.fuse_depth_views(dd, pp, intr, lo, hi, dims, alphas=aa, images=ii)
    with pytest.raises(ValueError):
        rf.fuse_depth_views(d, poses, rf.CameraIntrinsics(H, W, 0.0), lo, hi, dims)
    with pytest.raises(RuntimeError, match="HIP device"):
        rf.fuse_depth_views(d.cpu(), poses, intr, lo, hi, dims)
    with pytest.raises(RuntimeError, match="HIP device"):
        rf.fuse_depth_views(d, poses, intr, lo, hi, dims, alphas=a, images=i.cpu())
    volume = rf.fuse_depth_views(d, poses, intr, lo, hi, dims)
    with pytest.raises(ValueError):
        volume.to_voxel_grid(fill_colour=1.5)


# ----------------------------------------------------------------------------------------------------------------- the chain

def components_of(faces, num_vertices):
    """connected components of a mesh's vertices that faces use (numpy union-find by repeated minimum propagation)"""
    f = np.asarray(faces, np.int64)
    label = np.arange(num_vertices)
    while True:
        low = label[f].min(axis=1)
        new = label.copy()
        for c in range(3):
            np.minimum.at(new, f[:, c], low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return len(np.unique(label[np.unique(f)]))


def ball_grid(device, G=16, radius=0.6, scale=400.0):
    ax = (np.arange(G, dtype=np.float32) + 0.5) / G * 2.0 - 1.0
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    feat = torch.from_numpy(np.stack([4.0 * np.sin(5.0 * x + 1.0), 4.0 * np.cos(4.0 * y - z), 4.0 * np.sin(3.0 * z + 2.0 * x * y)], axis=-1).astype(np.float32))
    return rf.VoxelGrid(torch.from_numpy((radius - r).astype(np.float32)[..., None]).to(device), feat.to(device), rf.VoxelSize(2.0 / G, 2.0 / G, 2.0 / G),
                        density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=scale, storage="split")


def all_round_poses(radius=3.0, turn=0.0):
    """8 cameras that look at the origin from every side: 3 above, 3 below, one near each pole (``rf.pose_spherical`` stays in the upper
    hemisphere, and what no view sees from its free side stays solid: the rule's answer to the underside of an object on a table)"""
    positions = fm.ring(3, radius, 0.6, phase=turn) + fm.ring(3, radius, -0.6, phase=turn + np.pi / 3) + [(0.1 * radius, 0.07 * radius, 0.99 * radius), (-0.07 * radius, 0.1 * radius, -0.99 * radius)]
    return poses_of([fm.look_at(position) for position in positions])


def test_round_trip_through_render_mesh(hip_device):
    """a closed mesh -> its depth from 8 views -> fused -> extracted: closed again, and it renders the depth it was made from.  The
    bounds are those of docs/fusion_errors.md ("The round trip"): a surface within one voxel edge h of the original moves the depth of
    a ball by h / cos(incidence), whose mean over the ball's disc is 2 h; the silhouettes agree to within a ring one voxel edge plus one
    pixel footprint wide."""
    G, dims = 16, (24, 24, 24)
    h = 2.0 / dims[0]
    mesh = rf.extract_mesh(ball_grid(hip_device, G), 40.0, subdivisions=2)  # sigma = 400 (0.6 - r) = 40 at r = 0.5
    assert mesh_oracle.manifold_report(mesh.faces.cpu().numpy(), len(mesh.vertices))[0]
    intr = rf.CameraIntrinsics(48, 56, 70.0)
    poses = all_round_poses()
    renders = [rf.render_mesh(mesh, pose, intr) for pose in poses]
    depths = torch.stack([r.depth[..., 0] for r in renders])
    volume = rf.fuse_depth_views(depths, poses, intr, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), dims, images=torch.stack([r.colour for r in renders]))
    fused = volume.extract_mesh()
    assert fused.faces.shape[0] > 500 and fused.colours is not None
    closed, oriented, euler = mesh_oracle.manifold_report(fused.faces.cpu().numpy(), len(fused.vertices))
    assert closed and oriented and euler == 2  # every edge in exactly two faces, once per direction; one sphere
    radius = fused.vertices.norm(dim=1)
    print(f"fusion round trip: {fused.faces.shape[0]} faces, vertex radius {float(radius.min()):.4f} .. {float(radius.max()):.4f} (the ball: 0.5; voxel edge {h:.4f})")
    assert float((radius - 0.5).abs().max()) <= h + 3.0 / 70.0  # one voxel edge + one pixel footprint at the camera's distance
    worst_mean, worst_iou = 0.0, 1.0
    for pose, render in zip(poses, renders):
        mine = rf.render_mesh(fused, pose, intr)
        both = mine.mask & render.mask
        union = mine.mask | render.mask
        worst_mean = max(worst_mean, float((mine.depth - render.depth)[..., 0].abs()[both].mean()))
        worst_iou = min(worst_iou, float(both.sum()) / float(union.sum()))
        ring = 2.0 * np.pi * 0.5 * (h + 3.0 / 70.0) * (70.0 / 3.0) ** 2  # pixels in a ring of that width round the silhouette (radius 0.5 at distance 3)
        assert int((mine.mask ^ render.mask).sum()) <= ring
    print(f"fusion round trip: worst mean |depth - input depth| over a view {worst_mean:.5f} ({worst_mean / h:.3f} voxel edges), worst mask IoU {worst_iou:.4f}")
    assert worst_mean <= 2.0 * h


def test_to_voxel_grid_returns_the_tsdf_at_the_node_centres(hip_device):
    from thr3ed_atom_amd.ops import grid_query

    lo, hi, dims, cams, H, W, depths, al, im, trunc = fm.sphere_case()
    volume = rf.fuse_depth_views(on(hip_device, depths), poses_of(cams), rf.CameraIntrinsics(H, W, cams[0].focal), lo, hi, dims, alphas=on(hip_device, al), images=on(hip_device, im))
    nodes = torch.from_numpy(fm.node_positions(lo, hi, dims).reshape(-1, 3)).to(hip_device)
    for storage in ("reference", "split"):
        grid = volume.to_voxel_grid(storage=storage)
        assert grid.density_mode == "identity" and tuple(grid.grid_dims) == tuple(dims) and grid.num_features == 3
        assert torch.equal(grid.densities[..., 0], -volume.tsdf)
        assert [tuple(float(np.float32(v)) for v in r) for r in grid.aabb] == [(float(np.float32(a)), float(np.float32(b))) for a, b in zip(lo, hi)]
        out = grid_query(grid, nodes)
        # docs/fusion_errors.md ("The grid"): at a node centre the trilinear weights are (1, 0) up to the rounding of the index
        # coordinate, at most 8 u dim per axis, against neighbours that differ by at most 2
        bound = 3 * 2 * 8 * 2.0 ** -24 * max(dims) + 2.0 ** -23
        error = float((out[:, -1] + volume.tsdf.reshape(-1)).abs().max())
        print(f"fusion to_voxel_grid ({storage}): largest |query + tsdf| at the node centres {error:.3e} (bound {bound:.3e})")
        assert error <= bound
        colour = torch.sigmoid(out[:, :3] * 0.28209479177387814).reshape(tuple(dims) + (3,))
        expect = torch.where((volume.colour_count > 0)[..., None], volume.colour, torch.full_like(volume.colour, 0.5)).clamp(1 / 512, 1 - 1 / 512)
        assert float((colour - expect).abs().max()) <= 1e-4
    mesh = volume.extract_mesh()
    again = rf.extract_mesh(volume.to_voxel_grid(), 0.0, 1)
    assert torch.equal(mesh.vertices, again.vertices) and torch.equal(mesh.faces, again.faces)
    assert float((mesh.vertices.norm(dim=1) - fm.SPHERE_RADIUS).abs().max()) <= 0.103125  # the sphere chain of tests/test_fusion_model.py, on the device


def test_a_faint_detached_blob_leaves_no_shell(hip_device):
    """The point of the feature.  An opaque ball (sigma = 200 (0.45 - r), capped at 60) and a detached blob of density 1.3 and diameter
    0.3: above the iso level 1, but 1.3 x 0.3 = 0.39 <= 0.4, so no ray accumulates 1/2 in it (1 - exp(-0.39) = 0.32).  The density's
    mesh has two components, the fused one has one, and it scores the higher mask IoU against the field on poses that were not fused:
    a comparison with the density route by construction, not a tuned number."""
    G = 32
    ax = (np.arange(G, dtype=np.float32) + 0.5) / G * 2.0 - 1.0
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    ball = np.minimum(200.0 * (0.45 - np.sqrt(x * x + y * y + z * z)), 60.0)
    blob = np.where(np.sqrt((x - 0.72) ** 2 + y * y + (z - 0.1) ** 2) < 0.15, 1.3, 0.0)
    dens = np.maximum(ball, blob).astype(np.float32)
    feat = np.stack([2.0 * np.sin(3.0 * x), 2.0 * np.cos(2.0 * y), 2.0 * np.sin(z + x)], axis=-1).astype(np.float32)
    grid = rf.VoxelGrid(torch.from_numpy(dens[..., None]).to(hip_device), torch.from_numpy(feat).to(hip_device), rf.VoxelSize(2.0 / G, 2.0 / G, 2.0 / G),
                        density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=1.0, storage="split")
    cfg = rf.SHVoxGridRenderConfig(num_samples_per_ray=256, camera_bounds=rf.CameraBounds(0.5, 5.0), perturb_sampled_points=False, render_num_samples_per_ray=256)
    vol_mod = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    intr = rf.CameraIntrinsics(64, 64, 80.0)
    fuse_poses, held_out = all_round_poses(), all_round_poses(turn=0.5)[:6:2] + all_round_poses(turn=0.5)[7:]
    from_density = rf.extract_mesh(grid, 1.0, subdivisions=1)
    volume = rf.fuse_field_views(vol_mod, fuse_poses, intr)
    assert volume.tsdf.shape == (G, G, G) and volume.colour is not None and volume.aabb_min == (-1.0, -1.0, -1.0)
    fused = volume.extract_mesh()
    assert mesh_oracle.manifold_report(fused.faces.cpu().numpy(), len(fused.vertices))[0]
    parts = components_of(from_density.faces.cpu().numpy(), len(from_density.vertices)), components_of(fused.faces.cpu().numpy(), len(fused.vertices))
    scores = [rf.evaluate_mesh_against_field(m, None, vol_mod, held_out, intr) for m in (from_density, fused)]
    print(f"fusion against the density's mesh: components {parts[0]} -> {parts[1]}, held-out mask IoU {scores[0]['mask_iou']:.4f} -> {scores[1]['mask_iou']:.4f}, "
          f"depth L1 {scores[0]['depth_l1']:.5f} -> {scores[1]['depth_l1']:.5f}")
    assert parts == (2, 1)
    assert scores[1]["mask_iou"] > scores[0]["mask_iou"]
    # without the colour renders and on another lattice
    coarse = rf.fuse_field_views(vol_mod, fuse_poses[:3], intr, (20, 18, 16), images=False, truncation=0.3)
    assert coarse.tsdf.shape == (20, 18, 16) and coarse.colour is None and coarse.truncation == float(np.float32(0.3))


# --------------------------------------------------------------------------------------------------------------- the scripts

def test_the_scripts_end_to_end(hip_device, tmp_path):
    """one run of scripts/fuse_mesh.py and one of scripts/extract_mesh_from_sh_based_voxel_grid.py --fuse_views on the reference
    checkpoint fixture, each in a fresh process under its own time limit"""
    from thr3ed_atom_amd.mesh import read_ply

    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    checkpoint = os.path.join(REPO_ROOT, "tests", "golden", "reference_checkpoint.pth")
    fused = tmp_path / "fused.ply"
    r = subprocess.run([sys.executable, "scripts/fuse_mesh.py", "-i", checkpoint, "-o", str(fused), "--views", "5", "--grid_dims", "20", "18", "16", "--truncation_voxels", "2.5",
                        "--keep_largest", "1", "--simplify_voxels", "2"], cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "fused 5 views of " in r.stdout and "into (20, 18, 16) nodes" in r.stdout and "connected components inside the fused surface: " in r.stdout and fused.exists()
    vertices, _, _, faces = read_ply(str(fused))
    assert faces.size == 0 or faces.max() < len(vertices)
    other = tmp_path / "other.ply"
    r = subprocess.run([sys.executable, "scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", checkpoint, "-o", str(other), "--fuse_views", "4", "--fuse_truncation_voxels", "2",
                        "--subdivisions", "1", "--simplify_voxels", "2"], cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "fused 4 views of " in r.stdout and "iso_level 0" in r.stdout and other.exists()
