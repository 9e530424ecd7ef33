#!/usr/bin/env python
"""Time of the mesh rasteriser (thr3ed_atom_amd.render_mesh: rf_mesh_raster_visibility + rf_mesh_raster_shade) on the meshes of DESIGN.md
section 10's scene -- the 256^3 sparse scene of tests.helpers.sparse_scene_grid at level 5 -- for one 800 x 800 frame of the camera
tools/frame_time.py uses: the textured simplified mesh (subdivisions 2, cells of 2 voxels, patch 8, diffuse bake) and the raw
subdivisions = 1 mesh with its vertex colours.  HIP events, two warm-up runs, median of N timed runs, in a fresh process:

    whole        rf.render_mesh as a user calls it (checks, allocation, the fill of the visibility buffer, both launches, the status read)
    visibility   rf_mesh_raster_visibility alone into a freshly filled buffer (the fill is outside the events)
    shade        rf_mesh_raster_shade alone
    field        the field's own frame of the same camera on the same grid (VolumetricModel.render, 512 samples, occupancy mask)
    torch        a restatement of the same rule with torch ops, a brute force over all triangles per pixel in chunks; for the raw mesh
                 on a 100 x 100 frame of the same field of view (its time is linear in the pixels)

and the share of triangles whose pixel box is larger than 8 x 8 (the wave path), counted with torch from the same projection.
Writes profiles/mesh_raster_time.json.

    python tools/mesh_raster_time.py [timed runs] [output json] [--no-torch]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import _lib, mesh_raster  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else os.path.join(ROOT, "profiles", "mesh_raster_time.json")
with_torch = "--no-torch" not in sys.argv[1:]
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, DEGREE = 256, 5.0, 2
VOXEL = 3.0 / G
NEAR, FAR, RADIUS = float(np.float32(2.0) * 0.9), float(np.float32(6.0) * 1.1), 4.0311


def timed(fn, runs, warm=2, before=None):
    times = []
    for k in range(warm + runs):
        if before is not None:
            before()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = fn()
        stop.record()
        stop.synchronize()
        if k >= warm:
            times.append(start.elapsed_time(stop))
    times.sort()
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)], result


def camera_rays(pose, intr):
    rays = rf.cast_rays(intr, pose, dev)
    return rays.origins.reshape(-1, 3)[0].clone(), rays.directions.reshape(-1, 3).contiguous()


def torch_restatement(mesh, pose, intr, chunk=512):
    """face ids [H, W] by brute force: every triangle against every pixel, in chunks of triangles.  Unlike the kernel it has no pixel
    box: a zero-area sliver whose edge values are rounding noise can pass the sign test on every pixel of the frame (the raw mesh of
    the timed scene has one: DESIGN.md section 22), so on such a mesh its face ids are not the kernel's and only its time is of use."""
    o, d = camera_rays(pose, intr)
    R = torch.as_tensor(np.asarray(pose.rotation, np.float32), device=dev).reshape(3, 3)
    P = d.shape[0]
    best_z = torch.full((P,), float("inf"), device=dev)
    best_id = torch.full((P,), -1, dtype=torch.int64, device=dev)
    for lo in range(0, mesh.faces.shape[0], chunk):
        p = mesh.vertices[mesh.faces[lo:lo + chunk]] - o  # [Tc, 3, 3]
        zk = -(p @ R[:, 2])                                # [Tc, 3]
        e = []
        for k in range(3):  # (plain float32 products and sums: a matrix product may round differently)
            c = torch.linalg.cross(p[:, (k + 1) % 3], p[:, (k + 2) % 3])
            e.append((c[:, None, 0] * d[None, :, 0] + c[:, None, 1] * d[None, :, 1]) + c[:, None, 2] * d[None, :, 2])
        e = torch.stack(e, dim=-1)  # [Tc, P, 3]
        s = e.sum(-1)
        hit = ((e >= 0).all(-1) | (e <= 0).all(-1)) & (s != 0) & (zk >= 0).all(-1)[:, None]
        w = e / s[..., None]
        z = zk[:, None, 0] + (w[..., 1] * (zk[:, 1] - zk[:, 0])[:, None] + w[..., 2] * (zk[:, 2] - zk[:, 0])[:, None])
        z = torch.where(hit, z, torch.full_like(z, float("inf")))
        cz, row = z.min(dim=0)
        better = cz < best_z
        best_z = torch.where(better, cz, best_z)
        best_id = torch.where(better, row + lo, best_id)
    return best_id.reshape(int(intr.height), int(intr.width))


def wave_share(mesh, pose, intr):
    """share of the faces whose clipped pixel box (projected corners widened by one pixel) is larger than 8 x 8, and of those with a box at all"""
    o, _ = camera_rays(pose, intr)
    R = torch.as_tensor(np.asarray(pose.rotation, np.float32), device=dev).reshape(3, 3)
    cam = (mesh.vertices - o) @ R  # [V, 3]: x, y, -depth
    depth = -cam[:, 2]
    x = intr.focal * cam[:, 0] / depth + intr.width / 2 - 0.5
    y = intr.height / 2 - 0.5 - intr.focal * cam[:, 1] / depth
    fx, fy, fz = x[mesh.faces], y[mesh.faces], depth[mesh.faces]
    front = (fz > 0).all(-1)
    j0, j1 = torch.ceil(fx.amin(-1) - 1).clamp(0, intr.width), torch.floor(fx.amax(-1) + 1).clamp(-1, intr.width - 1)
    i0, i1 = torch.ceil(fy.amin(-1) - 1).clamp(0, intr.height), torch.floor(fy.amax(-1) + 1).clamp(-1, intr.height - 1)
    boxed = front & (j0 <= j1) & (i0 <= i1)
    wave = boxed & ((j1 - j0 >= _lib.RASTER_LANE_BOX) | (i1 - i0 >= _lib.RASTER_LANE_BOX))
    return float(wave.sum()) / max(int(boxed.sum()), 1), float(boxed.sum()) / len(mesh.faces)


def measure(name, mesh, bake, pose, intr, small_intr):
    lib = _lib.load()
    cam = mesh_raster._camera(pose, intr)
    H, W, V, T = intr.height, intr.width, mesh.vertices.shape[0], mesh.faces.shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    vis = torch.empty((H, W), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    colour, depth, ids = torch.empty((H, W, 3), device=dev), torch.empty((H, W, 1), device=dev), torch.empty((H, W), dtype=torch.int32, device=dev)
    row = {"V": V, "T": T, "image": [H, W], "source": "texture" if bake is not None else "vertex colours"}
    row["whole_ms"], out = timed(lambda: rf.render_mesh(mesh, pose, intr, bake), reps)
    row["visibility_ms"], _ = timed(lambda: _lib.check(lib.rf_mesh_raster_visibility(C.byref(cam), mesh.vertices.data_ptr(), V, mesh.faces.data_ptr(), T, 0.0, 0, vis.data_ptr(),
                                                                                     status.data_ptr(), stream), "visibility"), reps, before=lambda: vis.fill_(-1))
    uv, tex = (None, None) if bake is None else (bake.uvs.data_ptr(), bake.texture.data_ptr())
    th, tw = (0, 0) if bake is None else bake.texture.shape[:2]
    row["shade_ms"], _ = timed(lambda: _lib.check(lib.rf_mesh_raster_shade(C.byref(cam), mesh.vertices.data_ptr(), V, mesh.faces.data_ptr(), T, vis.data_ptr(), uv, tex, th, tw,
                                                                           None if bake is not None else mesh.colours.data_ptr(), 0, colour.data_ptr(), depth.data_ptr(),
                                                                           ids.data_ptr(), None, stream), "shade"), reps)
    row["fill_ms"], _ = timed(lambda: vis.fill_(-1), reps)
    row["kernels_equal_whole_bitwise"] = bool(torch.equal(ids, out.face_ids) and torch.equal(colour, out.colour) and torch.equal(depth, out.depth))
    row["covered_pixels"] = int(out.mask.sum())
    row["wave_path_share_of_boxed_faces"], row["boxed_share_of_faces"] = (round(v, 6) for v in wave_share(mesh, pose, intr))
    row["faces_per_s_visibility"] = round(T / (row["visibility_ms"][0] * 1e-3), -6)
    if with_torch:
        t_intr = intr if small_intr is None else small_intr
        row["torch_image"] = [t_intr.height, t_intr.width]
        row["torch_ms"], restated = timed(lambda: torch_restatement(mesh, pose, t_intr), 3, warm=1)
        mine = out.face_ids if small_intr is None else rf.render_mesh(mesh, pose, t_intr, bake).face_ids
        row["torch_face_id_agreement"] = round(float((restated == mine).float().mean()), 6)
        scale = (H * W) / (t_intr.height * t_intr.width)
        row["torch_ms_scaled_to_the_frame"] = round(row["torch_ms"][0] * scale, 1)
        row["torch_over_kernels"] = round(row["torch_ms"][0] * scale / (row["visibility_ms"][0] + row["shade_ms"][0]), 1)
    print(json.dumps({"mesh": name, **row}), flush=True)
    return row


def main():
    dens, feat = sparse_scene_grid((G, G, G), 3 * (DEGREE + 1) ** 2, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), storage="split", density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0)
    intr, small = rf.CameraIntrinsics(800, 800, 1111.111), rf.CameraIntrinsics(100, 100, 1111.111 / 8)
    pose = rf.pose_spherical(30.0, -30.0, RADIUS)
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "iso_level": ISO, "runs": reps, "columns": "median, min, max ms", "meshes": {}}
    with torch.no_grad():
        full = rf.extract_mesh(grid, ISO, subdivisions=2)
        h = np.float32(2 * VOXEL)
        lowest = full.vertices.amin(dim=0).cpu().numpy()
        origin = np.asarray([r[0] for r in grid.aabb], dtype=np.float32)
        origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
        mesh = rf.simplify_mesh(full, float(h), origin=origin.tolist())
        del full
        bake = rf.bake_texture(mesh, grid, 8, reach=float(np.float32(3 * VOXEL)), samples=16, diffuse=True)
        report["meshes"]["simplified, textured"] = measure("simplified, textured", mesh, bake, pose, intr, None)
        raw = rf.extract_mesh(grid, ISO, subdivisions=1)
        report["meshes"]["raw, subdivisions 1"] = measure("raw, subdivisions 1", raw, None, pose, intr, small)
        grid.build_occupancy()
        cfg = rf.SHVoxGridRenderConfig(512, rf.CameraBounds(NEAR, FAR), perturb_sampled_points=True, white_bkgd=False)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        report["field_frame_ms"], _ = timed(lambda: model.render(pose, intr, use_occupancy_mask=True), reps)
        report["field_frame"] = "VolumetricModel.render, 800 x 800, 512 samples per ray, occupancy mask, host call included"
        metrics = rf.evaluate_mesh_against_field(mesh, bake, model, [pose], rf.CameraIntrinsics(400, 400, 1111.111 / 2), use_occupancy_mask=True)
        report["simplified_against_field_400x400"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
    print(json.dumps({k: v for k, v in report.items() if k != "meshes"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
