"""GPU: rf.render_mesh (csrc/mesh_raster_kernels.hip) against the float64 model of tests/mesh_raster_model.py within the per-pixel
bounds of docs/mesh_raster_errors.md, on the smallest inputs at which it can go wrong (tests/mesh_raster_model.py CASES: images of
1 x 1, 24 x 40, 37 x 53 and 64 x 64 pixels; one triangle over the whole image (the wave path), triangles over every edge and corner,
1, 63, 64, 65 and 2000 sub-pixel triangles (the lane path), both in one launch, interpenetrating triangles, triangles behind the camera
and nearer than ``near``, zero-area faces, culling on and off for both windings, both backgrounds, texture colour for patch 2, 3 and 8,
vertex colours, barycentrics, a literal duplicate face; and the crafted exact cases, where EVERY pixel is compared); bad faces,
argument errors, the empty mesh; and the export chain end to end on a ball of one colour.

Measured on an MI355X: see docs/mesh_raster_errors.md for the worst ratio of error to bound over these cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_raster_model as rm

pytestmark = pytest.mark.gpu


def render_case(case, device, **overrides):
    mesh = rf.Mesh(torch.from_numpy(case["vertices"]).to(device), torch.from_numpy(case["faces"]).to(device),
                   None if case["colours"] is None else torch.from_numpy(case["colours"]).to(device), None)
    bake = None
    if case["texture"] is not None:
        lay = rf.texture.atlas_layout(len(case["faces"]), case["patch"])
        bake = rf.TextureBake(torch.from_numpy(case["texture"]).to(device), None, torch.from_numpy(case["uvs"]).to(device), lay.patch, lay.block, lay.cols, lay.rows)
    pose = rf.CameraPose(case["R"], case["t"].reshape(3, 1))
    kwargs = dict(near=case["near"], white_bkgd=case["white"], cull_backfaces=case["cull"], barycentrics=case["bary"])
    kwargs.update(overrides)
    return rf.render_mesh(mesh, pose, rf.CameraIntrinsics(case["H"], case["W"], case["focal"]), bake, **kwargs), mesh, bake, pose


def as_numpy(out):
    return dict(face_ids=out.face_ids.cpu().numpy(), mask=out.mask.cpu().numpy(), depth=out.depth[..., 0].cpu().numpy(),
                bary=None if out.barycentrics is None else out.barycentrics.cpu().numpy(), colour=None if out.colour is None else out.colour.cpu().numpy())


@pytest.mark.parametrize("name", rm.CASES)
def test_matches_the_model(hip_device, name):
    case, ref = rm.make_case(name), rm.reference(name)
    if case["exact"]:
        rm.assert_exact_in_float32(case)
    out, _, _, _ = render_case(case, hip_device)
    again, _, _, _ = render_case(case, hip_device)
    H, W = case["H"], case["W"]
    assert out.depth.shape == (H, W, 1) and out.mask.shape == (H, W) and out.face_ids.shape == (H, W)
    assert out.depth.dtype == torch.float32 and out.face_ids.dtype == torch.int32 and out.mask.dtype == torch.bool and out.depth.device.type == "cuda"
    assert (out.barycentrics is not None) == case["bary"] and (out.colour is None) == (case["texture"] is None and case["colours"] is None)
    for a, b in zip(out, again):  # bitwise
        assert (a is None and b is None) or torch.equal(a, b)
    got = as_numpy(out)
    assert np.array_equal(got["mask"], got["face_ids"] >= 0)
    assert (got["depth"][~got["mask"]] == 0).all()
    if got["bary"] is not None:
        assert (got["bary"][~got["mask"]] == 0).all()
    if got["colour"] is not None:
        assert (got["colour"][~got["mask"]] == (1.0 if case["white"] else 0.0)).all()
    ratio = rm.compare(ref, got, exact=case["exact"])
    print(f"mesh raster {name}: {ref['mask'].sum()} pixels covered, {0 if case['exact'] else ref['ambiguous'].sum()} skipped, worst error / bound {ratio:.4f}")
    assert not case["exact"] or ref["mask"].sum() > 60
    if not case["bary"]:  # the barycentrics are an output only: asking for them changes no other bit
        more, _, _, _ = render_case(case, hip_device, barycentrics=True)
        assert torch.equal(more.depth, out.depth) and torch.equal(more.face_ids, out.face_ids) and (out.colour is None or torch.equal(more.colour, out.colour))
        rm.compare(ref, as_numpy(more), exact=case["exact"])


def test_bad_faces_argument_errors_and_the_empty_mesh(hip_device):
    case = rm.make_case("interpenetrating")
    good, mesh, _, pose = render_case(case, hip_device)
    intr = rf.CameraIntrinsics(case["H"], case["W"], case["focal"])
    V, T = mesh.vertices.shape[0], mesh.faces.shape[0]
    victim = int(torch.mode(good.face_ids[good.face_ids > 0]).values)  # a face that owns pixels (not face 0: its twin below must lose ties)
    for bad_index in (V, -1, 2**40):
        faces = mesh.faces.clone()
        faces[victim, 2] = bad_index
        with pytest.raises(ValueError, match="faces index outside"):
            rf.render_mesh(mesh._replace(faces=faces), pose, intr)
    # the raw call: the status word says so, the bad face is skipped, and the pixels the other faces own are what they were
    from thr3ed_atom_amd import _lib, mesh_raster
    faces = mesh.faces.clone()
    faces[victim, 2] = V
    cam = mesh_raster._camera(pose, intr)
    vis = torch.full((case["H"], case["W"]), -1, dtype=torch.int64, device=hip_device)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    stream = torch.cuda.current_stream(hip_device).cuda_stream
    lib = _lib.load()
    assert lib.rf_mesh_raster_visibility(C.byref(cam), mesh.vertices.data_ptr(), V, faces.data_ptr(), T, 0.0, 0, vis.data_ptr(), status.data_ptr(), stream) == 0
    depth = torch.full((case["H"], case["W"]), 7.0, device=hip_device)
    ids = torch.full((case["H"], case["W"]), 7, dtype=torch.int32, device=hip_device)
    colour = torch.full((case["H"], case["W"], 3), 7.0, device=hip_device)
    assert lib.rf_mesh_raster_shade(C.byref(cam), mesh.vertices.data_ptr(), V, faces.data_ptr(), T, vis.data_ptr(), None, None, 0, 0, mesh.colours.data_ptr(), 0,
                                    colour.data_ptr(), depth.data_ptr(), ids.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 1 and not bool((ids == victim).any()) and bool((good.face_ids == victim).any())
    hidden = mesh.faces.clone()
    hidden[victim] = hidden[0]  # the face hidden behind a twin of face 0, which wins every tie
    without = rf.render_mesh(mesh._replace(faces=hidden), pose, intr)
    assert torch.equal(ids, without.face_ids) and torch.equal(depth, without.depth[..., 0]) and torch.equal(colour, without.colour)
    untouched = good.face_ids == without.face_ids
    assert bool(untouched.any()) and torch.equal(colour[untouched], good.colour[untouched]) and torch.isfinite(colour).all()
    # argument errors of the Python layer
    for bad_intr in ((0, 40, 30.0), (24, 16385, 30.0), (24, 40, 0.0), (24, 40, float("nan")), (24, 40, -1.0)):
        with pytest.raises(ValueError):
            rf.render_mesh(mesh, pose, rf.CameraIntrinsics(*bad_intr))
    for near in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="near"):
            rf.render_mesh(mesh, pose, intr, near=near)
    with pytest.raises(ValueError, match="pose"):
        rf.render_mesh(mesh, rf.CameraPose(case["R"], np.array([[0.0], [float("nan")], [0.0]], np.float32)), intr)
    with pytest.raises(ValueError, match="not finite"):
        rf.render_mesh(mesh._replace(vertices=mesh.vertices.clone().index_fill_(0, torch.tensor([0], device=hip_device), float("inf"))), pose, intr)
    with pytest.raises(ValueError, match="HIP device"):
        rf.render_mesh(rf.Mesh(mesh.vertices.cpu(), mesh.faces.cpu(), None, None), pose, intr)
    with pytest.raises(ValueError, match="faces on"):
        rf.render_mesh(rf.Mesh(mesh.vertices, mesh.faces.cpu(), None, None), pose, intr)
    lay = rf.texture.atlas_layout(T, 3)
    uvs = torch.from_numpy(rf.texture.corner_uvs(lay, T)).to(hip_device)
    texture = torch.rand((lay.height, lay.width, 3), device=hip_device)
    with pytest.raises(ValueError, match="UVs"):
        rf.render_mesh(mesh, pose, intr, rf.TextureBake(texture, None, uvs[:-1], 3, lay.block, lay.cols, lay.rows))
    with pytest.raises(ValueError, match="the bake is not"):
        rf.render_mesh(mesh, pose, intr, rf.TextureBake(texture.cpu(), None, uvs, 3, lay.block, lay.cols, lay.rows))
    # the empty mesh: the background, without a launch
    for white in (False, True):
        empty = rf.render_mesh(mesh._replace(faces=mesh.faces[:0]), pose, intr, white_bkgd=white, barycentrics=True)
        assert empty.colour.shape == (case["H"], case["W"], 3) and (empty.colour == float(white)).all() and not empty.mask.any()
        assert (empty.depth == 0).all() and (empty.face_ids == -1).all() and (empty.barycentrics == 0).all()
    bare = rf.render_mesh(rf.Mesh(mesh.vertices, mesh.faces[:0], None, None), pose, intr)
    assert bare.colour is None and bare.barycentrics is None


def test_export_chain_on_a_ball_of_one_colour(hip_device, tmp_path):
    """the 16^3 one-colour ball of tests/test_hip_texture.py carried through extract_mesh -> simplify_mesh -> bake_texture -> write_obj ->
    read_obj -> render_mesh from two poses, and evaluate_mesh_against_field on the same views"""
    G = 16
    ax = (np.arange(G, dtype=np.float32) + 0.5) / G * 2.0 - 1.0
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    dens = torch.from_numpy((0.6 - r).astype(np.float32)[..., None])
    coeff = np.array([1.2, -0.4, 0.3], np.float32)
    feat = torch.from_numpy(np.broadcast_to(coeff, (G, G, G, 3)).copy())
    voxel = 2.0 / G
    grid = rf.VoxelGrid(dens.to(hip_device), feat.to(hip_device), rf.VoxelSize(voxel, voxel, voxel), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=20.0, storage="split")
    cell = 2 * voxel
    mesh = rf.simplify_mesh(rf.extract_mesh(grid, 1.0, subdivisions=2), cell)
    T = mesh.faces.shape[0]
    assert T > 50
    bake = rf.bake_texture(mesh, grid, 4, reach=0.5 * voxel, samples=4)
    stem = str(tmp_path / "ball")
    rf.write_obj(mesh, bake, stem)
    mesh2, bake2 = rf.read_obj(stem, device=hip_device)
    # read_obj returns what was written: faces and UVs exactly, vertices to the 9 printed digits, the texture as its 8 bits
    assert torch.equal(mesh2.faces, mesh.faces) and torch.equal(bake2.uvs, bake.uvs)
    assert torch.equal(mesh2.vertices, mesh.vertices)  # (9 significant digits round-trip a float32)
    assert (bake2.patch, bake2.block, bake2.cols, bake2.rows) == (bake.patch, bake.block, bake.cols, bake.rows)
    assert torch.equal((bake2.texture * 255.0).round().to(torch.uint8), torch.from_numpy(rf.mesh.to8b(bake.texture.cpu().numpy())).to(hip_device))
    assert (mesh2.normals is None) == (mesh.normals is None) and (mesh.normals is None or torch.equal(mesh2.normals, mesh.normals))
    assert mesh2.colours is None and bake2.opacity is None
    # the surface {sigma > 1}: 20 (0.6 - r) = 1 at r = 0.55; h = one simplification cell plus one voxel
    radius, h = 0.55, cell + voxel
    want = 1.0 / (1.0 + np.exp(-0.28209479177387814 * coeff.astype(np.float64)))
    H = W = 64
    intr = rf.CameraIntrinsics(H, W, 80.0)
    poses = [rf.pose_spherical(30.0, -25.0, 3.0), rf.pose_spherical(200.0, 40.0, 2.5)]
    for pose in poses:
        out = rf.render_mesh(mesh2, pose, intr, bake2, cull_backfaces=True)
        colour, mask = out.colour.cpu().numpy().astype(np.float64), out.mask.cpu().numpy()
        # every covered pixel's colour: within one 8-bit step, the tolerance tests/test_hip_texture.py applies to the atlas of this ball
        assert mask.sum() > 100 and np.abs(255.0 * (colour[mask] - want)).max() <= 1.0 and (colour[~mask] == 0).all()
        # the silhouette against the analytic sphere: the distance of every pixel's ray from the centre
        rays = rf.cast_rays(intr, pose, hip_device)
        o, d = rays.origins.reshape(-1, 3).cpu().numpy().astype(np.float64), rays.directions.reshape(-1, 3).cpu().numpy().astype(np.float64)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        closest = np.linalg.norm(np.cross(-o, d), axis=-1).reshape(H, W)
        ahead = (np.einsum("ij,ij->i", -o, d) > 0).reshape(H, W)
        assert (ahead & (closest < radius - h)).sum() > 50 and (closest > radius + h).sum() > 50
        assert mask[ahead & (closest < radius - h)].all() and not mask[closest > radius + h].any()
        depth = out.depth[..., 0].cpu().numpy()
        centre_distance = np.linalg.norm(o[0])
        assert (np.abs(depth[mask] - centre_distance) < radius + h).all()
        both = rf.render_mesh(mesh2, pose, intr, bake2)  # a closed surface seen from outside: culling hides nothing
        assert torch.equal(both.face_ids, out.face_ids)
    cfg = rf.SHVoxGridRenderConfig(num_samples_per_ray=128, camera_bounds=rf.CameraBounds(0.5, 5.0), perturb_sampled_points=False, render_num_samples_per_ray=128)
    vol_mod = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    metrics = rf.evaluate_mesh_against_field(mesh2, bake2, vol_mod, poses, intr)
    assert set(metrics) == {"psnr", "ssim", "depth_l1", "mask_iou", "per_image"} and len(metrics["per_image"]) == 2
    for row in metrics["per_image"] + [metrics]:
        assert all(np.isfinite(row[k]) for k in ("psnr", "ssim", "depth_l1", "mask_iou"))
        # both masks hold the disc of radius r - h and stay inside the one of radius r + h (the field's > 1/2 mask: the ray has to
        # cross at least the opaque core), so their IoU is at least the ratio of the two discs' areas, less the pixels on the rims
        assert ((radius - h) / (radius + h)) ** 2 * 0.8 <= row["mask_iou"] <= 1.0
    print(f"ball: {metrics}")
