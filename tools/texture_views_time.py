#!/usr/bin/env python
"""Time and quality of texture baking from posed views (thr3ed_atom_amd.bake_texture_from_views: rf_mesh_raster_visibility per view +
rf_texture_project_views per chunk of 16) on the simplified mesh of DESIGN.md sections 21 / 22 -- the 256^3 sparse scene of
tests.helpers.sparse_scene_grid at level 5, subdivisions 2, cells of 2 voxels: 63,811 triangles -- at patch 8 from 42 turn-table views
of 800 x 800 pixels of the field's own renders.  HIP events, two warm-up runs, median of N timed runs, in a fresh process:

    projection   the three rf_texture_project_views launches (16 + 16 + 10 views) on visibility buffers made beforehand
    visibility   the 42 rf_mesh_raster_visibility launches into freshly filled buffers (the fill is outside the events)
    whole        rf.bake_texture_from_views as a user calls it on images that are on the device (checks, allocation, fills, 42 + 3
                 launches, the status read, the division)
    torch        a restatement of the projection with torch ops: per view the projection of all owned texels, the depth test against
                 the same visibility buffer, F.grid_sample of image and alpha plane, the sums -- against the projection launches

and the quality: rf.evaluate_mesh_against_field on poses NOT used for baking, for the normal-ray bake (rf.bake_texture, the bake of
section 22) and for the view bake with that bake as fallback; and the share of the owned texels the views saw.
Writes profiles/texture_views_time.json.

    python tools/texture_views_time.py [timed runs] [output json] [--no-torch]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import _lib, mesh_raster  # noqa: E402
from thr3ed_atom_amd import texture as tx  # noqa: E402
from thr3ed_atom_amd.constants import EXTRA_ACCUMULATED_WEIGHTS  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else os.path.join(ROOT, "profiles", "texture_views_time.json")
with_torch = "--no-torch" not in sys.argv[1:]
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, DEGREE, PATCH, VIEWS = 256, 5.0, 2, 8, 42
VOXEL = 3.0 / G
NEAR, FAR, RADIUS = float(np.float32(2.0) * 0.9), float(np.float32(6.0) * 1.1), 4.0311
MIN_COS, COS_POWER, MIN_WEIGHT = 0.1, 2, 1e-3


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


def owned_texels(mesh, lay):
    """(flat image index [M], point p [M, 3], unit normal n [M, 3]) of every owned texel, with torch from the documented layout"""
    B, P, T = lay.block, lay.patch, mesh.faces.shape[0]
    blk = torch.arange(lay.cols * lay.rows, device=dev)
    j, i = torch.meshgrid(torch.arange(B, device=dev), torch.arange(B, device=dev), indexing="ij")
    upper = (i + j > P + 3)
    tri = 2 * blk[:, None, None] + upper[None].long()
    a = torch.where(upper, P + 2 - i, i - 1).float() / (P - 1)
    b = torch.where(upper, P + 2 - j, j - 1).float() / (P - 1)
    pixel = ((blk // lay.cols)[:, None, None] * B + j[None]) * lay.width + (blk % lay.cols)[:, None, None] * B + i[None]
    own = tri < T
    tri, pixel = tri[own], pixel[own]
    b1, b2 = a[None].expand(len(blk), B, B)[own], b[None].expand(len(blk), B, B)[own]
    v = mesh.vertices[mesh.faces[tri]]
    p = ((1.0 - b1) - b2)[:, None] * v[:, 0] + b1[:, None] * v[:, 1] + b2[:, None] * v[:, 2]
    n = F.normalize(torch.linalg.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), dim=-1)
    return pixel, p, n


def torch_projection(pixel, p, n, lay, poses, intr, images, alphas, keys, depth_bias, background):
    """accum [Ht Wt, 4] and count [Ht Wt] of the same rule with torch ops, one view after another"""
    H, W, f = int(intr.height), int(intr.width), float(intr.focal)
    accum = torch.zeros((lay.height * lay.width, 4), device=dev)
    count = torch.zeros(lay.height * lay.width, dtype=torch.int32, device=dev)
    sums, seen = torch.zeros((p.shape[0], 4), device=dev), torch.zeros(p.shape[0], dtype=torch.int32, device=dev)
    for k, pose in enumerate(poses):
        R = torch.as_tensor(np.asarray(pose.rotation, np.float32), device=dev).reshape(3, 3)
        t = torch.as_tensor(np.asarray(pose.translation, np.float32), device=dev).reshape(3)
        d = p - t
        c = d @ R
        z = -c[:, 2]
        x, y = W / 2 + f * c[:, 0] / z, H / 2 - f * c[:, 1] / z
        cs = -(n * d).sum(-1) / d.norm(dim=-1)
        ok = (z > 0) & (x >= 0) & (x < W) & (y >= 0) & (y < H) & (cs > MIN_COS)
        jj, ii = x.clamp(0, W - 1).long(), y.clamp(0, H - 1).long()
        key = keys[k][ii, jj]
        zbuf = (key >> 32).to(torch.int32).view(torch.float32)
        ok &= (key != -1) & (z <= zbuf + depth_bias)
        grid = torch.stack([2 * x / W - 1, 2 * y / H - 1], dim=-1)[None, None]  # the fetch at (x - 1/2, y - 1/2) in pixel-index coordinates
        planes = torch.cat([images[k].permute(2, 0, 1), alphas[k][None]])[None]
        got = F.grid_sample(planes, grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].T  # [M, 4]
        m = got[:, 3]
        wm = cs ** COS_POWER * m
        terms = torch.cat([wm[:, None] * (got[:, :3] - ((1 - m) * background)[:, None]), (wm * m)[:, None]], dim=-1)
        sums += torch.where(ok[:, None], terms, torch.zeros_like(terms))
        seen += ok
    accum[pixel], count[pixel] = sums, seen
    return accum.reshape(lay.height, lay.width, 4), count.reshape(lay.height, lay.width)


def main():
    dens, feat = sparse_scene_grid((G, G, G), 3 * (DEGREE + 1) ** 2, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), storage="split", density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0)
    intr = rf.CameraIntrinsics(800, 800, 1111.111)
    poses = rf.get_thre360_animation_poses(RADIUS, -30.0, VIEWS + 1)
    held_out = [rf.pose_spherical(yaw, pitch, RADIUS) for yaw, pitch in ((17.0, -50.0), (107.0, -12.0), (197.0, -45.0), (287.0, -8.0), (62.0, -70.0), (242.0, -20.0))]
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "iso_level": ISO, "runs": reps, "columns": "median, min, max ms", "patch": PATCH, "views": VIEWS,
              "image": [800, 800], "min_cos": MIN_COS, "cos_power": COS_POWER, "bake_poses": f"turn-table, pitch -30, radius {RADIUS}",
              "held_out_poses": "6 poses at other yaws and pitches, 400 x 400"}
    lib = _lib.load()
    with torch.no_grad():
        full = rf.extract_mesh(grid, ISO, subdivisions=2)
        h = np.float32(2 * VOXEL)
        lowest = full.vertices.amin(dim=0).cpu().numpy()
        origin = np.asarray([r[0] for r in grid.aabb], dtype=np.float32)
        origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
        mesh = rf.simplify_mesh(full, float(h), origin=origin.tolist())
        del full
        V, T = mesh.vertices.shape[0], mesh.faces.shape[0]
        normal_bake = rf.bake_texture(mesh, grid, PATCH, reach=float(np.float32(3 * VOXEL)), samples=16, diffuse=True)
        grid.build_occupancy()
        cfg = rf.SHVoxGridRenderConfig(512, rf.CameraBounds(NEAR, FAR), perturb_sampled_points=False, white_bkgd=False)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        images = torch.stack([model.render(pose, intr, use_occupancy_mask=True).colour.float() for pose in poses]).contiguous()
        alphas = torch.stack([model.render_geometry(pose, intr, use_occupancy_mask=True).extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].float() for pose in poses]).contiguous()
        lay = tx.atlas_layout(T, PATCH)
        report.update({"V": V, "T": T, "atlas": [lay.height, lay.width]})
        corners = mesh.vertices.double()[mesh.faces]
        depth_bias = float(np.float32(float((corners - corners.roll(1, dims=1)).norm(dim=-1).mean())))
        report["depth_bias"] = depth_bias
        stream = torch.cuda.current_stream(dev).cuda_stream
        cams = [mesh_raster._camera(pose, intr) for pose in poses]
        keys = torch.empty((VIEWS, 800, 800), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)

        def visibility():
            for k in range(VIEWS):
                _lib.check(lib.rf_mesh_raster_visibility(C.byref(cams[k]), mesh.vertices.data_ptr(), V, mesh.faces.data_ptr(), T, 0.0, 0, keys[k].data_ptr(),
                                                         status.data_ptr(), stream), "visibility")
        report["visibility_ms"], _ = timed(visibility, reps, before=lambda: keys.fill_(-1))
        accum = torch.zeros((lay.height, lay.width, 4), device=dev)
        count = torch.zeros((lay.height, lay.width), dtype=torch.int32, device=dev)

        def projection():
            for lo in range(0, VIEWS, 16):
                n = min(16, VIEWS - lo)
                chunk = (_lib.RFCamera * n)(*cams[lo:lo + n])
                _lib.check(lib.rf_texture_project_views(mesh.vertices.data_ptr(), V, mesh.faces.data_ptr(), T, PATCH, lay.cols, lay.rows, n, chunk, images[lo:].data_ptr(),
                                                        keys[lo:].data_ptr(), alphas[lo:].data_ptr(), 0.0, depth_bias, MIN_COS, COS_POWER, 0.0, 0, accum.data_ptr(),
                                                        count.data_ptr(), status.data_ptr(), stream), "projection")
        report["projection_ms"], _ = timed(projection, reps, before=lambda: (accum.zero_(), count.zero_()))
        report["whole_ms"], out = timed(lambda: rf.bake_texture_from_views(mesh, images, poses, intr, PATCH, alphas=alphas, fallback=normal_bake, min_cos=MIN_COS,
                                                                             cos_power=COS_POWER, min_weight=MIN_WEIGHT), reps)
        texture, weight = tx.finalise_views(accum, normal_bake.texture, MIN_WEIGHT)
        report["kernels_equal_whole_bitwise"] = bool(torch.equal(texture, out.bake.texture) and torch.equal(weight, out.weight) and torch.equal(count, out.views))
        pixel, p, n = owned_texels(mesh, lay)
        M = int(pixel.numel())
        seen = out.views.reshape(-1)[pixel] >= 1
        used = out.weight.reshape(-1)[pixel] > MIN_WEIGHT
        report.update({"owned_texels": M, "share_of_owned_texels_seen": round(float(seen.float().mean()), 4), "share_of_owned_texels_baked_from_views": round(float(used.float().mean()), 4),
                       "mean_views_per_seen_texel": round(float(out.views.reshape(-1)[pixel][seen].float().mean()), 2),
                       "texel_views_per_s_projection": round(M * VIEWS / (report["projection_ms"][0] * 1e-3), -6)})
        if with_torch:
            report["torch_ms"], (t_accum, t_count) = timed(lambda: torch_projection(pixel, p, n, lay, poses, intr, images, alphas, keys, depth_bias, 0.0), 3, warm=1)
            same = (t_count == count).reshape(-1)[pixel]
            report["torch_view_count_agreement"] = round(float(same.float().mean()), 6)
            diff = (t_accum - accum).abs().amax(-1).reshape(-1)[pixel]
            report["torch_max_difference_where_counts_agree"] = float(diff[same].max())
            report["torch_over_projection"] = round(report["torch_ms"][0] / report["projection_ms"][0], 1)
        small = rf.CameraIntrinsics(400, 400, 1111.111 / 2)
        for name, bake in (("normal_ray_bake", normal_bake), ("view_bake", out.bake)):
            metrics = rf.evaluate_mesh_against_field(mesh, bake, model, held_out, small, use_occupancy_mask=True)
            report[f"{name}_against_field_held_out"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
        metrics = rf.evaluate_mesh_against_field(mesh, out.bake, model, poses[::7], small, use_occupancy_mask=True)
        report["view_bake_against_field_on_6_bake_poses"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
