#!/usr/bin/env python
"""Time and quality of the TSDF fusion of posed depth views (thr3ed_atom_amd.fusion: rf_fuse_depth_views) on the scene of DESIGN.md
sections 21 - 25 -- the 256^3 sparse scene of tests.helpers.sparse_scene_grid, 42 turn-table views of 800 x 800 pixels, depth = the
field's own median depth, alpha = its accumulated weight, colour = its render.  HIP events, two warm-up runs, then N rounds in which
the variants take turns (one process, interleaved), median / min / max per variant:

    hip          the pass (3 launches: 16 + 16 + 10 views over zeroed accumulators)
    torch        the same rule in plain torch ops, per view: project all nodes, index, where -- what a user of the library without
                 the kernel would have to write -- and how many nodes it counts differently

each with and without the colour images, and section 25's quality table (rf.evaluate_mesh_against_field on 6 held-out poses at
400 x 400) extended by the fused geometry: raw, simplified at 2 voxels, simplified and view-baked.  Writes profiles/fusion_time.json.

    python tools/fusion_time.py [rounds] [output json]"""
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
from thr3ed_atom_amd import _lib, _marshal  # noqa: E402
from thr3ed_atom_amd import fusion as fu  # noqa: E402
from thr3ed_atom_amd.constants import EXTRA_ACCUMULATED_WEIGHTS  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "fusion_time.json")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, DEGREE, PATCH, VIEWS = 256, 2, 8, 42
VOXEL = 3.0 / G
NEAR, FAR, RADIUS = float(np.float32(2.0) * 0.9), float(np.float32(6.0) * 1.1), 4.0311


def say(report, key):
    print(json.dumps({key: report[key]}), flush=True)


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    result = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), result


def summary(times):
    times = sorted(times)
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)]


def hip_pass(lo, hi, dims, cams, depths, alphas, images, truncation, state):
    """the launches of rf.fuse_depth_views over zeroed accumulators (the zeroing is inside the timed region: three memsets)"""
    lib = _lib.load()
    tsdf_sum, counts, colour = state
    tsdf_sum.zero_(), counts.zero_()
    if images is not None:
        colour.zero_()
    box_lo, box_hi, cdims, stream = _lib.float3(lo), _lib.float3(hi), (C.c_int32 * 3)(*dims), _marshal.stream(dev)
    for first in range(0, len(cams), fu.MAX_VIEWS):
        last = min(first + fu.MAX_VIEWS, len(cams))
        rc = lib.rf_fuse_depth_views(box_lo, box_hi, cdims, last - first, (_lib.RFCamera * (last - first))(*cams[first:last]), depths[first:last].data_ptr(),
                                     alphas[first:last].data_ptr(), None if images is None else images[first:last].data_ptr(), 0.0, truncation, 0.5, _lib.FUSE_CARVE,
                                     tsdf_sum.data_ptr(), counts.data_ptr(), None if images is None else colour.data_ptr(), stream)
        _lib.check(rc, "rf_fuse_depth_views")
    return state


def torch_pass(lo, hi, dims, poses, intr, depths, alphas, images, truncation):
    """rf_fuse_depth_views' rule in plain torch ops (float32), per view: project all nodes, index, where"""
    H, W, focal = int(intr[0]), int(intr[1]), float(intr[2])
    axes = [torch.tensor(lo[a], device=dev) + torch.tensor(hi[a] - lo[a], device=dev) * ((2 * torch.arange(dims[a], device=dev) + 1).float() / float(2 * dims[a])) for a in range(3)]
    px, py, pz = torch.meshgrid(*axes, indexing="ij")
    total, observed, hidden = torch.zeros(dims, device=dev), torch.zeros(dims, dtype=torch.int32, device=dev), torch.zeros(dims, dtype=torch.int32, device=dev)
    colour = torch.zeros(tuple(dims) + (4,), device=dev) if images is not None else None
    one = torch.ones((), device=dev)
    for k, pose in enumerate(poses):
        R = torch.as_tensor(pose.rotation, dtype=torch.float32).reshape(3, 3).tolist()
        t = torch.as_tensor(pose.translation, dtype=torch.float32).reshape(3).tolist()
        dx, dy, dz = px - t[0], py - t[1], pz - t[2]
        cx = (dx * R[0][0] + dy * R[1][0]) + dz * R[2][0]
        cy = (dx * R[0][1] + dy * R[1][1]) + dz * R[2][1]
        z = -((dx * R[0][2] + dy * R[1][2]) + dz * R[2][2])
        x = W * 0.5 + focal * cx / z
        y = H * 0.5 - focal * cy / z
        inside = (z > 0.0) & torch.isfinite(z) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        pixel = torch.where(inside, y.floor().clamp(0, H - 1) * W + x.floor().clamp(0, W - 1), torch.zeros_like(x)).long()
        D, A = depths[k].reshape(-1)[pixel], alphas[k].reshape(-1)[pixel]
        known = inside & torch.isfinite(D)
        miss = ~(D > 0) | (A < 0.5)
        sdf = D - z
        hit = known & ~miss
        behind = hit & (sdf < -truncation)
        counted = (hit & ~behind) | (known & miss)
        s = torch.where(hit, torch.minimum(one, sdf / truncation), one)
        total = torch.where(counted, total + s, total)
        observed += counted
        hidden += behind
        if images is not None:
            near_surface = hit & (sdf.abs() <= truncation)
            rgb = images[k].reshape(-1, 3)[pixel]
            colour = torch.where(near_surface[..., None], colour + torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1), colour)
    return total, observed, hidden, colour


def main():
    dens, feat = sparse_scene_grid((G, G, G), 3 * (DEGREE + 1) ** 2, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), storage="split", density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0)
    intr = rf.CameraIntrinsics(800, 800, 1111.111)
    poses = rf.get_thre360_animation_poses(RADIUS, -30.0, VIEWS + 1)
    held_out = [rf.pose_spherical(yaw, pitch, RADIUS) for yaw, pitch in ((17.0, -50.0), (107.0, -12.0), (197.0, -45.0), (287.0, -8.0), (62.0, -70.0), (242.0, -20.0))]
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "rounds": reps, "columns": "median, min, max ms", "views": VIEWS, "image": [800, 800],
              "fused_poses": f"turn-table, pitch -30, radius {RADIUS}", "held_out_poses": "6 poses at other yaws and pitches, 400 x 400", "truncation_voxels": 3.0}
    dims = (G, G, G)
    lo, hi = tuple(float(np.float32(r[0])) for r in grid.aabb), tuple(float(np.float32(r[1])) for r in grid.aabb)
    truncation = float(np.float32(fu.default_truncation(lo, hi, dims)))
    with torch.no_grad():
        grid.build_occupancy()
        cfg = rf.SHVoxGridRenderConfig(512, rf.CameraBounds(NEAR, FAR), perturb_sampled_points=False, white_bkgd=False)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        depths, alphas, images = [], [], []
        for pose in poses:
            geometry = model.render_geometry(pose, intr, quantile=0.5, use_occupancy_mask=True)
            depths.append(geometry.depth[..., 0].float())
            alphas.append(geometry.extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].float())
            images.append(model.render(pose, intr, use_occupancy_mask=True).colour.float())
        depths, alphas, images = torch.stack(depths).contiguous(), torch.stack(alphas).contiguous(), torch.stack(images).contiguous()
        cams = [_marshal.checked_camera(pose, intr) for pose in poses]
        state = (torch.zeros(dims, device=dev), torch.zeros(dims + (2,), dtype=torch.int32, device=dev), torch.zeros(dims + (4,), device=dev))

        variants = {}
        for with_images in (True, False):
            variants[f"hip{'' if with_images else '_no_images'}_ms"] = lambda with_images=with_images: hip_pass(lo, hi, dims, cams, depths, alphas, images if with_images else None, truncation, state)
        for with_images in (True, False):
            variants[f"torch{'' if with_images else '_no_images'}_ms"] = lambda with_images=with_images: torch_pass(lo, hi, dims, poses, intr, depths, alphas, images if with_images else None, truncation)
        times = {name: [] for name in variants}
        for k in range(2 + reps):  # two warm-up rounds; the variants take turns within every round
            for name, fn in variants.items():
                ms, _ = event_ms(fn)
                if k >= 2:
                    times[name].append(ms)
        for name in variants:
            report[name] = summary(times[name])
            say(report, name)
        report["torch_over_hip"] = round(report["torch_ms"][0] / report["hip_ms"][0], 2)
        say(report, "torch_over_hip")
        # two passes give the same bits; torch against the kernel
        a = [t.clone() for t in hip_pass(lo, hi, dims, cams, depths, alphas, images, truncation, state)]
        b = hip_pass(lo, hi, dims, cams, depths, alphas, images, truncation, state)
        report["two_passes_give_equal_bits"] = bool(all(torch.equal(u, v) for u, v in zip(a, b)))
        total, observed, hidden, _ = torch_pass(lo, hi, dims, poses, intr, depths, alphas, None, truncation)
        same = (observed == b[1][..., 0]) & (hidden == b[1][..., 1])
        report["torch_nodes_counted_differently"] = int((~same).sum())
        report["torch_max_tsdf_sum_difference_where_counted_alike"] = float((total - b[0]).abs()[same].max())
        report["nodes"] = {"observed": int((b[1][..., 0] > 0).sum()), "hidden_only": int(((b[1][..., 0] == 0) & (b[1][..., 1] > 0)).sum()),
                           "never_seen": int(((b[1][..., 0] == 0) & (b[1][..., 1] == 0)).sum())}
        for key in ("two_passes_give_equal_bits", "torch_nodes_counted_differently", "torch_max_tsdf_sum_difference_where_counted_alike", "nodes"):
            say(report, key)
        del a, total, observed, hidden, same

        # the whole public call, renders excluded, and the extraction
        ms, volume = event_ms(lambda: rf.fuse_depth_views(depths, poses, intr, lo, hi, dims, alphas=alphas, images=images))
        report["fuse_depth_views_call_ms"] = round(ms, 3)
        ms, raw = event_ms(lambda: volume.extract_mesh())
        report["extract_ms"] = round(ms, 3)
        h = np.float32(2 * VOXEL)
        lowest = raw.vertices.amin(dim=0).cpu().numpy()
        origin = np.asarray(lo, dtype=np.float32)
        origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
        small = rf.simplify_mesh(raw, float(h), origin=origin.tolist())
        report["fused_mesh"] = {"V": int(raw.vertices.shape[0]), "T": int(raw.faces.shape[0]), "simplified_V": int(small.vertices.shape[0]), "simplified_T": int(small.faces.shape[0])}
        for key in ("fuse_depth_views_call_ms", "extract_ms", "fused_mesh"):
            say(report, key)
        normal_bake = rf.bake_texture(small, grid, PATCH, reach=float(np.float32(3 * VOXEL)), samples=16, diffuse=True)
        view_bake = rf.bake_texture_from_views(small, images, poses, intr, PATCH, alphas=alphas, fallback=normal_bake).bake
        quarter = rf.CameraIntrinsics(400, 400, 1111.111 / 2)
        for name, (which, bake) in (("fused_raw", (raw, None)), ("fused_simplified", (small, None)), ("fused_simplified_view_bake", (small, view_bake))):
            metrics = rf.evaluate_mesh_against_field(which, bake, model, held_out, quarter, use_occupancy_mask=True)
            report[f"{name}_against_field_held_out"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
            say(report, f"{name}_against_field_held_out")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
