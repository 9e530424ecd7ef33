#!/usr/bin/env python
"""Time and quality of fitting a baked texture to posed views (thr3ed_atom_amd.texture_fit: rf_mesh_raster_taps, rf_texture_sample,
rf_texture_sample_backward) on the scene of DESIGN.md sections 21 - 23 -- the 256^3 sparse scene of tests.helpers.sparse_scene_grid at
level 5, subdivisions 2, cells of 2 voxels: 63,811 triangles, patch 8, 42 turn-table views of 800 x 800 pixels of the field's own
renders, starting from the view bake of section 23.  HIP events, two warm-up runs, median of N timed runs, in a fresh process:

    sampler      rf.MeshTextureSampler(...): 42 visibility + 42 taps launches, the expansion, the stable sort, the offsets
    forward      one rf_texture_sample launch over all views           -- against an indexed gather with torch ops on the same taps
    backward     one rf_texture_sample_backward launch                 -- against index_add_ with torch ops on the same taps,
                 and under other long-segment thresholds (the A/B that chose the default)
    render_mesh  42 rf.render_mesh calls: the parent's only route to the same colours
    iteration    one whole rf.fit_texture iteration (L2, and L1 + 0.2 D-SSIM): (6 iterations - 1 iteration) / 5

and the records (entries, coverage histogram, bytes moved by the backward and the share of the HBM peak that is), the loss curves
of a few learning rates, and the quality rows of section 23 extended by the two fits, on 6 held-out poses and on 6 of the fitted
poses.  Writes profiles/texture_fit_time.json.

    python tools/texture_fit_time.py [timed runs] [output json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import texture_fit as tf  # noqa: E402
from thr3ed_atom_amd.constants import EXTRA_ACCUMULATED_WEIGHTS  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "texture_fit_time.json")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, DEGREE, PATCH, VIEWS = 256, 5.0, 2, 8, 42
VOXEL = 3.0 / G
NEAR, FAR, RADIUS = float(np.float32(2.0) * 0.9), float(np.float32(6.0) * 1.1), 4.0311
HBM_PEAK = 8.0e12  # bytes per second, the MI355X's data-sheet figure
THRESHOLDS = (2, 4, 8, 12, 16, 24, 32, 64, 128, 256, 1024, 1 << 30)
LEARNING_RATES = (1e-3, 3e-3, 1e-2, 3e-2, 1e-1)
SWEEP_ITERATIONS, FIT_ITERATIONS = 100, 200


def timed(fn, runs, warm=2):
    times = []
    for k in range(warm + runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = fn()
        stop.record()
        stop.synchronize()
        if k >= warm:
            times.append(start.elapsed_time(stop))
    times.sort()
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)], result


def say(report, key):
    print(json.dumps({key: report[key]}), flush=True)


def main():
    dens, feat = sparse_scene_grid((G, G, G), 3 * (DEGREE + 1) ** 2, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), storage="split", density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0)
    intr = rf.CameraIntrinsics(800, 800, 1111.111)
    poses = rf.get_thre360_animation_poses(RADIUS, -30.0, VIEWS + 1)
    held_out = [rf.pose_spherical(yaw, pitch, RADIUS) for yaw, pitch in ((17.0, -50.0), (107.0, -12.0), (197.0, -45.0), (287.0, -8.0), (62.0, -70.0), (242.0, -20.0))]
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "iso_level": ISO, "runs": reps, "columns": "median, min, max ms", "patch": PATCH, "views": VIEWS,
              "image": [800, 800], "fit_poses": f"turn-table, pitch -30, radius {RADIUS}", "held_out_poses": "6 poses at other yaws and pitches, 400 x 400"}
    with torch.no_grad():
        full = rf.extract_mesh(grid, ISO, subdivisions=2)
        h = np.float32(2 * VOXEL)
        lowest = full.vertices.amin(dim=0).cpu().numpy()
        origin = np.asarray([r[0] for r in grid.aabb], dtype=np.float32)
        origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
        mesh = rf.simplify_mesh(full, float(h), origin=origin.tolist())
        del full
        normal_bake = rf.bake_texture(mesh, grid, PATCH, reach=float(np.float32(3 * VOXEL)), samples=16, diffuse=True)
        grid.build_occupancy()
        cfg = rf.SHVoxGridRenderConfig(512, rf.CameraBounds(NEAR, FAR), perturb_sampled_points=False, white_bkgd=False)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        images = torch.stack([model.render(pose, intr, use_occupancy_mask=True).colour.float() for pose in poses]).contiguous()
        alphas = torch.stack([model.render_geometry(pose, intr, use_occupancy_mask=True).extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].float() for pose in poses]).contiguous()
        start = rf.bake_texture_from_views(mesh, images, poses, intr, PATCH, alphas=alphas, fallback=normal_bake).bake
        Ht, Wt = start.texture.shape[:2]
        report.update({"V": mesh.vertices.shape[0], "T": mesh.faces.shape[0], "atlas": [Ht, Wt]})
        say(report, "T")

        report["sampler_ms"], sampler = timed(lambda: rf.MeshTextureSampler(mesh, start, poses, intr), min(reps, 5), warm=1)
        say(report, "sampler_ms")
        E, P, texels = sampler.num_entries, sampler.P, Ht * Wt
        cov = sampler.coverage.reshape(-1).to(torch.int64)
        edges = [0, 1, 5, 17, 65, 257, 1025, 4097]
        labels = ["0", "1-4", "5-16", "17-64", "65-256", "257-1024", "1025-4096", ">4096"]
        histogram = {label: int(((cov >= lo) & (cov < hi)).sum()) for label, lo, hi in zip(labels, edges, edges[1:] + [1 << 62])}
        report.update({"pixels": P, "hit_pixels": E // 4, "entries": E, "coverage_histogram": histogram, "coverage_max": int(cov.max()),
                       "coverage_median_of_covered": int(cov[cov > 0].median())})
        say(report, "coverage_histogram")

        texture = start.texture.contiguous()
        report["forward_ms"], colour = timed(lambda: sampler._forward(texture), reps)
        grad_colour = torch.randn_like(colour)
        report["backward_ms"], grad = timed(lambda: sampler._backward(grad_colour), reps)
        report["backward_ms_by_long_segment"] = {}
        for threshold in THRESHOLDS:
            sampler.long_segment = threshold
            report["backward_ms_by_long_segment"]["none" if threshold == 1 << 30 else str(threshold)], other = timed(lambda: sampler._backward(grad_colour), reps)
            report.setdefault("backward_max_difference_between_thresholds", 0.0)
            report["backward_max_difference_between_thresholds"] = max(report["backward_max_difference_between_thresholds"], float((other - grad).abs().max()))
        sampler.long_segment = 0
        moved = 8 * E + 12 * E + 8 * (texels + 1) + 12 * texels  # entries, one gathered gradient per entry, offsets, the texture gradient
        report.update({"backward_bytes": moved, "backward_share_of_hbm_peak": round(moved / (report["backward_ms"][0] * 1e-3) / HBM_PEAK, 4), "hbm_peak_bytes_per_s": HBM_PEAK})
        for key in ("forward_ms", "backward_ms", "backward_ms_by_long_segment", "backward_share_of_hbm_peak"):
            say(report, key)

        # the torch restatement on the same taps
        x0, x1, y0, y1, fx, fy = tf.tap_fields(sampler.taps)
        hit = torch.nonzero(x0 != tf.NO_TAP).view(-1)
        x0, x1, y0, y1, fx, fy = (a[hit] for a in (x0, x1, y0, y1, fx, fy))
        flat = texture.view(-1, 3)
        ids = [y0 * Wt + x0, y0 * Wt + x1, y1 * Wt + x0, y1 * Wt + x1]
        fx3, fy3 = fx[:, None], fy[:, None]
        weights = [(1 - fx3) * (1 - fy3), fx3 * (1 - fy3), (1 - fx3) * fy3, fx3 * fy3]

        def torch_forward():
            out = torch.zeros((P, 3), device=dev)
            top = (1 - fx3) * flat[ids[0]] + fx3 * flat[ids[1]]
            bot = (1 - fx3) * flat[ids[2]] + fx3 * flat[ids[3]]
            out[hit] = (1 - fy3) * top + fy3 * bot
            return out

        def torch_backward():
            g = grad_colour.view(-1, 3)[hit]
            out = torch.zeros((texels, 3), device=dev)
            for idx, w in zip(ids, weights):
                out.index_add_(0, idx, w * g)
            return out
        report["torch_forward_ms"], t_colour = timed(torch_forward, reps)
        report["torch_backward_ms"], t_grad = timed(torch_backward, reps)
        report["torch_forward_equal_bitwise"] = bool(torch.equal(t_colour.view_as(colour), colour))
        report["torch_backward_max_difference"] = float((t_grad.view_as(grad) - grad).abs().max())
        report["torch_forward_over_kernel"] = round(report["torch_forward_ms"][0] / report["forward_ms"][0], 2)
        report["torch_backward_over_kernel"] = round(report["torch_backward_ms"][0] / report["backward_ms"][0], 2)
        del t_colour, t_grad, ids, weights, x0, x1, y0, y1, fx, fy, fx3, fy3
        report["render_mesh_42_ms"], renders = timed(lambda: [rf.render_mesh(mesh, pose, intr, start).colour for pose in poses], reps)
        report["forward_equals_render_mesh_bitwise"] = bool(all(torch.equal(colour[k], renders[k]) for k in range(VIEWS)))
        report["render_mesh_over_forward"] = round(report["render_mesh_42_ms"][0] / report["forward_ms"][0], 1)
        del renders, colour, grad, grad_colour, sampler
        for key in ("torch_forward_ms", "torch_backward_ms", "render_mesh_42_ms", "forward_equals_render_mesh_bitwise"):
            say(report, key)

    common = dict(alphas=alphas, background=0.0)
    for name, kw in (("l2", dict(loss="l2")), ("l1_dssim", dict(loss="l1", dssim_weight=0.2))):
        one, _ = timed(lambda: rf.fit_texture(mesh, start, images, poses, intr, iterations=1, **common, **kw), 3, warm=1)
        six, _ = timed(lambda: rf.fit_texture(mesh, start, images, poses, intr, iterations=6, **common, **kw), 3, warm=1)
        report[f"fit_iteration_{name}_ms"] = round((six[0] - one[0]) / 5.0, 3)
        say(report, f"fit_iteration_{name}_ms")

    report["loss_curves_l2"] = {}
    marks = [0, 9, 29, 99]
    for lr in LEARNING_RATES:
        history = rf.fit_texture(mesh, start, images, poses, intr, iterations=SWEEP_ITERATIONS, lr=lr, **common).history.cpu().numpy()
        report["loss_curves_l2"][f"{lr:g}"] = {str(k + 1): float(history[k]) for k in marks}
    say(report, "loss_curves_l2")
    best = min(LEARNING_RATES, key=lambda lr: report["loss_curves_l2"][f"{lr:g}"][str(SWEEP_ITERATIONS)])
    report.update({"lr_with_lowest_loss_after_sweep": best, "default_lr": tf.DEFAULT_LR, "quality_fit_iterations": FIT_ITERATIONS})

    small = rf.CameraIntrinsics(400, 400, 1111.111 / 2)
    bakes = {"normal_ray_bake": normal_bake, "view_bake": start}
    for name, kw in (("views_fit_l2", dict(loss="l2")), ("views_fit_l1_dssim", dict(loss="l1", dssim_weight=0.2))):
        fit = rf.fit_texture(mesh, start, images, poses, intr, iterations=FIT_ITERATIONS, lr=tf.DEFAULT_LR, **common, **kw)
        history = fit.history.cpu().numpy()
        report[f"{name}_loss"] = [float(history[0]), float(history[-1])]
        bakes[name] = fit.bake
    for name, bake in bakes.items():
        for where, which in (("held_out", held_out), ("on_6_fit_poses", poses[::7])):
            metrics = rf.evaluate_mesh_against_field(mesh, bake, model, which, small, use_occupancy_mask=True)
            report[f"{name}_against_field_{where}"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
            say(report, f"{name}_against_field_{where}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
