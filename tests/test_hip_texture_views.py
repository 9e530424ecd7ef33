"""GPU: rf.bake_texture_from_views / rf_texture_project_views (csrc/texture_views_kernels.hip) against the float64 model of
tests/texture_views_model.py within the per-texel bound of docs/texture_views_errors.md, on the smallest inputs at which it can go
wrong (tests/texture_views_model.py SPECS: T = 1, 2, 3 and an odd T, patch 2, 3, 4 and 8, images of 1 x 1 to 48 x 64, 1, 2, 16 and 17
views, a view behind the mesh and one that looks past it, a zero-area face, a flipped face with and without the two-sided flag, with
and without alphas, backgrounds 0 and 1, cos_power 0, 2 and 8) and bit for bit on the crafted exact cases; chunking, determinism,
bad faces, argument errors, the empty mesh, zero views; and the export chain end to end on a ball of one colour.

Measured on an MI355X: see docs/texture_views_errors.md for the worst ratio of error to bound over these cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_raster_model as mrm
from tests import texture_views_model as tvm
from thr3ed_atom_amd import _lib, mesh_raster
from thr3ed_atom_amd import texture as tx

pytestmark = pytest.mark.gpu

ALL_CASES = tvm.CASES + list(tvm.EXACT_CASES)


def made_of(name):
    return tvm.make_exact(name) if name in tvm.EXACT_CASES else tvm.make_case(name)


def reference_of(name):
    """(model result, model depths [n, H, W]) of a randomised or an exact case"""
    if name not in tvm.EXACT_CASES:
        return tvm.reference(name)
    made = made_of(name)
    view = made["views"][0]
    raster = mrm.rasterise(made["vertices"], made["faces"], 16, 16, 16.0, view["R"], view["t"])
    depths = np.where(raster["mask"], raster["depth"], np.inf)[None]
    return tvm.project_case(made, depths), depths


def mesh_of(made, device, faces=None):
    return rf.Mesh(torch.from_numpy(made["vertices"]).to(device), torch.from_numpy(made["faces"] if faces is None else faces).to(device), None, None)


def poses_of(made):
    return [rf.CameraPose(v["R"], v["t"].reshape(3, 1)) for v in made["views"]]


def intrinsics_of(made):
    return [rf.CameraIntrinsics(v["H"], v["W"], v["focal"]) for v in made["views"]]


def flags_of(made):
    return _lib.TEXTURE_VIEWS_TWO_SIDED if made["two_sided"] else 0


def raw_project(made, mesh, keys, accum, count, status, first=0, last=None):
    """rf_texture_project_views over the views first .. last of a case, with ``keys`` [n, H, W] int64 as its visibility"""
    last = len(made["views"]) if last is None else last
    n, dev = last - first, mesh.vertices.device
    cams = (_lib.RFCamera * n)(*[mesh_raster._camera(p, i) for p, i in zip(poses_of(made)[first:last], intrinsics_of(made)[first:last])])
    images = torch.from_numpy(made["images"][first:last]).to(dev).contiguous()
    alphas = None if made["alphas"] is None else torch.from_numpy(made["alphas"][first:last]).to(dev).contiguous()
    lay = tx.atlas_layout(len(made["faces"]), made["patch"])
    rc = _lib.load().rf_texture_project_views(mesh.vertices.data_ptr(), mesh.vertices.shape[0], mesh.faces.data_ptr(), mesh.faces.shape[0], lay.patch, lay.cols, lay.rows,
                                              n, cams, images.data_ptr(), keys.data_ptr(), None if alphas is None else alphas.data_ptr(), made["near"],
                                              made["depth_bias"], made["min_cos"], made["cos_power"], made["background"], flags_of(made), accum.data_ptr(),
                                              None if count is None else count.data_ptr(), status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    return lay


def buffers(made, device, fill=0.0):
    lay = tx.atlas_layout(len(made["faces"]), made["patch"])
    return (torch.full((lay.height, lay.width, 4), fill, dtype=torch.float32, device=device), torch.zeros((lay.height, lay.width), dtype=torch.int32, device=device),
            torch.zeros(1, dtype=torch.int32, device=device))


def fallback_of(made, device):
    return None if made["fallback"] is None else torch.from_numpy(made["fallback"]).to(device)


def fallback_bake(made, device):
    if made["fallback"] is None:
        return None
    lay = tx.atlas_layout(len(made["faces"]), made["patch"])
    return rf.TextureBake(fallback_of(made, device), None, torch.from_numpy(tx.corner_uvs(lay, len(made["faces"]))).to(device), lay.patch, lay.block, lay.cols, lay.rows)


def bake_kwargs(made, device):
    return dict(alphas=None if made["alphas"] is None else torch.from_numpy(made["alphas"]), background=made["background"], fallback=fallback_bake(made, device),
                near=made["near"], depth_bias=None if made["default_bias"] else made["depth_bias"], min_cos=made["min_cos"], cos_power=made["cos_power"],
                two_sided=made["two_sided"], min_weight=made["min_weight"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_kernel_matches_the_model_on_the_models_depth(hip_device, name):
    made = made_of(name)
    ref, depths = reference_of(name)
    mesh = mesh_of(made, hip_device)
    keys = torch.from_numpy(tvm.depth_keys(depths)).to(hip_device)
    n = len(made["views"])
    accum, count, status = buffers(made, hip_device)
    for lo in range(0, n, 16):  # (the entry point takes at most 16 views)
        raw_project(made, mesh, keys[lo:lo + 16].contiguous(), accum, count, status, lo, min(lo + 16, n))
    again = buffers(made, hip_device)
    for lo in range(0, n, 16):
        raw_project(made, mesh, keys[lo:lo + 16].contiguous(), again[0], again[1], again[2], lo, min(lo + 16, n))
    assert torch.equal(accum, again[0]) and torch.equal(count, again[1]) and int(status.item()) == 0  # bitwise
    texture, weight = tx.finalise_views(accum, fallback_of(made, hip_device), made["min_weight"])
    ratio = tvm.compare(ref, texture.cpu().numpy(), weight.cpu().numpy(), count.cpu().numpy(), exact=name in tvm.EXACT_CASES)
    owned = ref["owned"]
    skipped = 0.0 if name in tvm.EXACT_CASES else 100 * ref["ambiguous"][owned].mean()
    print(f"texture views (kernel) {name}: worst error / bound {ratio:.4f}, {skipped:.2f} % skipped, "
          f"{100 * (ref['views'][owned] > 0).mean():.1f} % seen")
    assert (accum.cpu().numpy()[~owned] == 0).all()  # unowned texels are not touched


@pytest.mark.parametrize("name", ALL_CASES)
def test_python_layer_matches_the_model(hip_device, name):
    made = made_of(name)
    ref, _ = reference_of(name)
    mesh = mesh_of(made, hip_device)
    images = torch.from_numpy(made["images"])  # (on the CPU: uploaded chunk by chunk)
    out = rf.bake_texture_from_views(mesh, images, poses_of(made), intrinsics_of(made), made["patch"], **bake_kwargs(made, hip_device))
    again = rf.bake_texture_from_views(mesh, [im.to(hip_device) for im in images], poses_of(made), intrinsics_of(made), made["patch"], **bake_kwargs(made, hip_device))
    assert torch.equal(out.bake.texture, again.bake.texture) and torch.equal(out.weight, again.weight) and torch.equal(out.views, again.views)
    lay = ref["layout"]
    assert (out.bake.patch, out.bake.block, out.bake.cols, out.bake.rows) == (lay["patch"], lay["block"], lay["cols"], lay["rows"])
    assert out.bake.texture.shape == (lay["height"], lay["width"], 3) and out.bake.texture.dtype == torch.float32 and out.bake.opacity is None
    assert out.weight.shape == (lay["height"], lay["width"]) and out.views.dtype == torch.int32 and out.bake.texture.device.type == "cuda"
    assert np.array_equal(out.bake.uvs.cpu().numpy(), tx.corner_uvs(tx.atlas_layout(len(made["faces"]), made["patch"]), len(made["faces"])))
    ratio = tvm.compare(ref, out.bake.texture.cpu().numpy(), out.weight.cpu().numpy(), out.views.cpu().numpy(), exact=name in tvm.EXACT_CASES)
    print(f"texture views (python) {name}: worst error / bound {ratio:.4f}")


def test_chunks_of_views_equal_single_view_calls(hip_device):
    """17 views through the Python layer (chunks of 16 + 1) against 17 raw calls of one view each on the rasteriser's own visibility"""
    made = made_of("oct31-P4-40x40-v17")
    mesh = mesh_of(made, hip_device)
    out = rf.bake_texture_from_views(mesh, torch.from_numpy(made["images"]), poses_of(made), intrinsics_of(made), made["patch"], **bake_kwargs(made, hip_device))
    accum, count, status = buffers(made, hip_device)
    H, W = made["views"][0]["H"], made["views"][0]["W"]
    for k in range(17):
        cam = mesh_raster._camera(poses_of(made)[k], intrinsics_of(made)[k])
        vis = torch.full((1, H, W), -1, dtype=torch.int64, device=hip_device)
        rc = _lib.load().rf_mesh_raster_visibility(C.byref(cam), mesh.vertices.data_ptr(), mesh.vertices.shape[0], mesh.faces.data_ptr(), mesh.faces.shape[0],
                                                   made["near"], 0, vis.data_ptr(), status.data_ptr(), torch.cuda.current_stream(hip_device).cuda_stream)
        assert rc == 0
        raw_project(made, mesh, vis, accum, count, status, k, k + 1)
    texture, weight = tx.finalise_views(accum, fallback_of(made, hip_device), made["min_weight"])
    assert torch.equal(texture, out.bake.texture) and torch.equal(weight, out.weight) and torch.equal(count, out.views)  # bitwise
    assert int(out.views.max()) >= 3 and int(status.item()) == 0


def test_bad_faces(hip_device):
    made = made_of("oct32-P4-40x40-v3")
    mesh = mesh_of(made, hip_device)
    V, victim = mesh.vertices.shape[0], 5
    images = torch.from_numpy(made["images"]).to(hip_device)
    for bad_index in (V, -1, 2**40):
        faces = mesh.faces.clone()
        faces[victim, 2] = bad_index
        with pytest.raises(ValueError, match="faces index outside"):
            rf.bake_texture_from_views(mesh._replace(faces=faces), images, poses_of(made), intrinsics_of(made), made["patch"])
    # the raw call: status 1, the victim's texels untouched, every other face's texels the bits they have without the victim -- the keys
    # are those of the mesh whose victim is a zero-area face (never drawn, like the skipped bad face)
    hidden = made["faces"].copy()
    hidden[victim] = hidden[victim, 0]
    depths = tvm.depth_buffers(dict(made, faces=hidden))[0]
    keys = torch.from_numpy(tvm.depth_keys(depths)).to(hip_device)
    good, _, good_status = buffers(made, hip_device, fill=7.0)
    raw_project(made, mesh_of(made, hip_device, hidden), keys, good, None, good_status)
    for bad_index in (V, -1, 2**40):
        faces = mesh.faces.clone()
        faces[victim, 2] = bad_index
        accum, count, status = buffers(made, hip_device, fill=7.0)
        count.fill_(3)
        raw_project(made, mesh._replace(faces=faces), keys, accum, count, status)
        face = torch.from_numpy(tvm.tm.texel_table(32, made["patch"])["face"]).to(hip_device)
        assert int(status.item()) == 1 and int(good_status.item()) == 0
        assert (accum[face == victim] == 7.0).all() and (count[face == victim] == 3).all() and (accum[face == -1] == 7.0).all()
        others = (face >= 0) & (face != victim)
        assert torch.equal(accum[others], good[others]) and bool((accum[others] != 7.0).any()) and bool(torch.isfinite(accum).all())


def test_argument_errors_the_empty_mesh_and_zero_views(hip_device):
    made = made_of("oct32-P4-40x40-v3")
    mesh = mesh_of(made, hip_device)
    images, poses, intr = torch.from_numpy(made["images"]).to(hip_device), poses_of(made), intrinsics_of(made)[0]
    good = rf.bake_texture_from_views(mesh, images, poses, intr, 4)
    assert int(good.views.max()) >= 1
    for kwargs in (dict(patch=1), dict(patch=65), dict(cols=0), dict(near=-0.1), dict(near=float("nan")), dict(depth_bias=-1.0), dict(depth_bias=float("inf")),
                   dict(min_cos=-0.1), dict(min_cos=1.0), dict(cos_power=-1), dict(cos_power=9), dict(cos_power=1.5), dict(background=float("nan")),
                   dict(background=-1.0), dict(min_weight=-1.0), dict(min_weight=float("nan"))):
        with pytest.raises(ValueError):
            rf.bake_texture_from_views(mesh, images, poses, intr, **{"patch": 4, **kwargs})
    # counts and sizes of images, poses and alphas
    alphas = torch.ones(images.shape[:3], device=hip_device)
    for args, kwargs in (((images[:2], poses), {}), ((images, poses[:2]), {}), ((images, poses), dict(alphas=alphas[:2])), ((images[:, :-1], poses), {}),
                         ((images[..., :2], poses), {}), ((images, poses), dict(alphas=alphas[:, :, :-1])), (([images[0], images[1], images[2, :-1]], poses), {})):
        with pytest.raises(ValueError):
            rf.bake_texture_from_views(mesh, args[0], args[1], intr, 4, **kwargs)
    with pytest.raises(ValueError):
        rf.bake_texture_from_views(mesh, images, poses, [intr, intr], 4)
    with pytest.raises(ValueError):
        rf.bake_texture_from_views(mesh, images, poses, [intr, intr, rf.CameraIntrinsics(intr.height + 1, intr.width, intr.focal)], 4)
    for bad_intr in ((0, 40, 30.0), (40, 16385, 30.0), (40, 40, 0.0), (40, 40, float("nan"))):
        with pytest.raises(ValueError):
            rf.bake_texture_from_views(mesh, images, poses, rf.CameraIntrinsics(*bad_intr), 4)
    with pytest.raises(ValueError, match="pose"):
        rf.bake_texture_from_views(mesh, images, [poses[0], poses[1], rf.CameraPose(made["views"][2]["R"], np.full((3, 1), np.inf, np.float32))], intr, 4)
    with pytest.raises(ValueError, match="not finite"):
        rf.bake_texture_from_views(mesh._replace(vertices=mesh.vertices.clone().index_fill_(0, torch.tensor([0], device=hip_device), float("inf"))), images, poses, intr, 4)
    with pytest.raises(ValueError, match="HIP device"):
        rf.bake_texture_from_views(rf.Mesh(mesh.vertices.cpu(), mesh.faces.cpu(), None, None), images, poses, intr, 4)
    # a fallback of another layout
    lay3 = tx.atlas_layout(32, 3)
    other = rf.TextureBake(torch.zeros((lay3.height, lay3.width, 3), device=hip_device), None, good.bake.uvs, 3, lay3.block, lay3.cols, lay3.rows)
    with pytest.raises(ValueError, match="layout"):
        rf.bake_texture_from_views(mesh, images, poses, intr, 4, fallback=other)
    # zero views: the fallback, or zeros
    none = rf.bake_texture_from_views(mesh, images[:0], [], intr, 4)
    assert none.bake.texture.shape == good.bake.texture.shape and not bool(none.bake.texture.any()) and not bool(none.weight.any()) and not bool(none.views.any())
    sentinel = good.bake._replace(texture=torch.full_like(good.bake.texture, 0.25))
    kept = rf.bake_texture_from_views(mesh, [], [], intr, 4, fallback=sentinel)
    assert torch.equal(kept.bake.texture, sentinel.texture) and torch.equal(kept.bake.uvs, good.bake.uvs)
    # the empty mesh: 0 x 0 without a launch
    empty = rf.bake_texture_from_views(rf.Mesh(mesh.vertices, mesh.faces[:0], None, None), images, poses, intr, 8)
    assert empty.bake.texture.shape == (0, 0, 3) and empty.weight.shape == (0, 0) and empty.views.shape == (0, 0) and empty.bake.uvs.shape == (0, 3, 2)
    assert (empty.bake.cols, empty.bake.rows) == (0, 0)
    # the default depth bias is the mean edge length
    corners = made["vertices"].astype(np.float64)[made["faces"]]
    bias = float(np.float32(np.linalg.norm(corners - np.roll(corners, 1, axis=1), axis=-1).mean()))
    explicit = rf.bake_texture_from_views(mesh, images, poses, intr, 4, depth_bias=bias)
    assert torch.equal(explicit.bake.texture, good.bake.texture) and torch.equal(explicit.views, good.views)


def test_export_chain_on_a_ball_of_one_colour(hip_device, tmp_path):
    """the 16^3 one-colour ball of tests/test_hip_texture.py: extract_mesh -> simplify_mesh -> bake_texture_from_field_views from 6 poses
    around it -> write_obj -> read_obj -> render_mesh"""
    G = 16
    ax = (np.arange(G, dtype=np.float32) + 0.5) / G * 2.0 - 1.0
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    dens = torch.from_numpy((0.6 - r).astype(np.float32)[..., None])
    coeff = np.array([1.2, -0.4, 0.3], np.float32)
    feat = torch.from_numpy(np.broadcast_to(coeff, (G, G, G, 3)).copy())
    voxel = 2.0 / G
    grid = rf.VoxelGrid(dens.to(hip_device), feat.to(hip_device), rf.VoxelSize(voxel, voxel, voxel), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=20.0, storage="split")
    mesh = rf.simplify_mesh(rf.extract_mesh(grid, 1.0, subdivisions=2), 2 * voxel)
    T = mesh.faces.shape[0]
    assert T > 50
    cfg = rf.SHVoxGridRenderConfig(num_samples_per_ray=128, camera_bounds=rf.CameraBounds(0.5, 5.0), perturb_sampled_points=False, render_num_samples_per_ray=128)
    vol_mod = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    intr = rf.CameraIntrinsics(64, 64, 80.0)
    poses = [rf.pose_spherical(yaw, pitch, 3.0) for yaw, pitch in ((0.0, -20.0), (90.0, 25.0), (180.0, -30.0), (270.0, 20.0), (45.0, -80.0), (200.0, 75.0))]
    fallback = rf.bake_texture(mesh, grid, 4, reach=0.5 * voxel, samples=4)  # (the reach of the two other ball tests)
    out = rf.bake_texture_from_field_views(mesh, vol_mod, poses, intr, 4, fallback=fallback)
    want = 1.0 / (1.0 + np.exp(-0.28209479177387814 * coeff.astype(np.float64)))
    owned = tvm.tm.texel_table(T, 4)["face"] >= 0
    texture, views = out.bake.texture.cpu().numpy().astype(np.float64), out.views.cpu().numpy()
    seen = views >= 1
    # every seen texel: within one 8-bit step, the tolerance the two other ball tests apply -- at the silhouette too, where the pixel
    # is a * colour exactly and the alpha rule divides the a out again
    assert not seen[~owned].any() and seen[owned].mean() > 0.5, seen[owned].mean()
    assert np.abs(255.0 * (texture[seen] - want)).max() <= 1.0, np.abs(255.0 * (texture[seen] - want)).max()
    print(f"ball: {100 * seen[owned].mean():.1f} % of the owned texels seen, worst error {np.abs(255.0 * (texture[seen] - want)).max():.3f} 8-bit steps")
    default = rf.bake_texture_from_field_views(mesh, vol_mod, poses[:2], intr, 4)  # the default fallback: bake_texture(mesh, vol_mod, patch)
    assert default.bake.texture.shape == out.bake.texture.shape and bool((default.bake.texture[torch.from_numpy(owned).to(hip_device)] > 0).all())
    stem = str(tmp_path / "ball_views")
    rf.write_obj(mesh, out.bake, stem)
    mesh2, bake2 = rf.read_obj(stem, device=hip_device)
    assert torch.equal(mesh2.faces, mesh.faces) and torch.equal(bake2.uvs, out.bake.uvs)
    render = rf.render_mesh(mesh2, poses[0], intr, bake2, cull_backfaces=True)
    colour, mask = render.colour.cpu().numpy().astype(np.float64), render.mask.cpu().numpy()
    assert mask.sum() > 100 and np.abs(255.0 * (colour[mask] - want)).max() <= 2.0  # (one step of the bake, one of the 8-bit file)
