#!/usr/bin/env python
"""Time and quality of fitting mesh vertices to posed views (thr3ed_atom_amd.mesh_fit: rf_mesh_raster_coverage,
rf_mesh_geometry_backward_pixels, rf_mesh_geometry_backward_gather) on the scene of DESIGN.md sections 21 - 24 -- the 256^3 sparse scene of
tests.helpers.sparse_scene_grid at level 5, subdivisions 2, cells of 2 voxels: 63,811 triangles, 42 turn-table views of 800 x 800 pixels,
targets = the field's own median depth and accumulated weight.  HIP events, two warm-up runs, median of N timed runs, in a fresh
process:

    forward      42 x (visibility + coverage) launches        -- one view against a torch evaluation of the coverage rule on the
                                                                 face ids and vertices of rf.render_mesh
    pixels       42 rf_mesh_geometry_backward_pixels launches
    sort         the stable sort of the hit pixels by face, bincount, cumsum (once per iteration)
    gather       rf_mesh_geometry_backward_gather (two launches) -- against index_add_ of the same 9-float records onto faces and then
                 vertices, and under other long-segment thresholds
    iteration    one whole rf.fit_mesh_to_views iteration: (6 iterations - 1 iteration) / 5

and the loss curves of a few step sizes (as fractions of the mean edge length), and section 24's quality table extended by the
fitted geometry before and after re-baking the texture.  Writes profiles/mesh_fit_time.json.

    python tools/mesh_fit_time.py [timed runs] [output json] [fit iterations]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import mesh_fit as mf  # noqa: E402
from thr3ed_atom_amd.constants import EXTRA_ACCUMULATED_WEIGHTS  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mesh_fit_time.json")
FIT_ITERATIONS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, DEGREE, PATCH, VIEWS = 256, 5.0, 2, 8, 42
VOXEL = 3.0 / G
NEAR, FAR, RADIUS = float(np.float32(2.0) * 0.9), float(np.float32(6.0) * 1.1), 4.0311
THRESHOLDS = (2, 4, 8, 16, 32, 64, 256, 1 << 30)
LR_FRACTIONS = (0.005, 0.01, 0.02, 0.05, 0.1)
SWEEP_ITERATIONS = 60


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


def torch_coverage(vertices, faces, face_ids, pose, intr):
    """the coverage rule of include/relu_field.h with torch ops, for one view, from the face ids of rf.render_mesh: (coverage [H, W], margin
    [H, W]); margin = over the pairs a pixel is part of, the smallest |e_k(b)| relative to the magnitude of its terms -- how far the
    missed centre is from the nearest edge line of the winning face, in units where float32 rounding is about 1e-7"""
    H, W, focal = int(intr[0]), int(intr[1]), float(intr[2])
    R = torch.as_tensor(pose.rotation, dtype=torch.float32, device=dev).reshape(3, 3)
    t = torch.as_tensor(pose.translation, dtype=torch.float32, device=dev).reshape(3)
    j, i = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="xy")
    cam = torch.stack([((j + 0.5) - W * 0.5) / focal, -(((i + 0.5) - H * 0.5) / focal), -torch.ones_like(j)], -1)
    d = (cam @ R.T).reshape(-1, 3)
    ids = face_ids.reshape(-1).to(torch.int64)
    hit = ids >= 0
    a = torch.nonzero(hit).view(-1)
    p = vertices[faces[ids[a]]] - t
    c = torch.stack([torch.cross(p[:, 1], p[:, 2], dim=1), torch.cross(p[:, 2], p[:, 0], dim=1), torch.cross(p[:, 0], p[:, 1], dim=1)], 1)  # [M, 3 edges, 3]
    ea = (c * d[a][:, None, :]).sum(-1)
    sa = ea.sum(-1)
    gain, loss = torch.zeros(H * W, device=dev), torch.zeros(H * W, device=dev)
    margin = torch.full((H * W,), float("inf"), device=dev)
    ai, aj = a // W, a % W
    for di, dj in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        bi, bj = ai + di, aj + dj
        ok = (bi >= 0) & (bi < H) & (bj >= 0) & (bj < W)
        b = torch.where(ok, bi * W + bj, torch.zeros_like(bi))
        ok &= ~hit[b]
        m = torch.nonzero(ok).view(-1)
        eb = (c[m] * d[b[m]][:, None, :]).sum(-1)
        outside = torch.sign(sa[m])[:, None] * eb < 0
        tau = torch.where(outside, ea[m] / (ea[m] - eb), torch.full_like(eb, float("inf"))).amin(1)
        counts = outside.any(1)
        tau = torch.where(counts, tau.clamp(0.0, 1.0), torch.full_like(tau, 0.5))
        gain.index_add_(0, b[m], (tau - 0.5).clamp(min=0.0))
        loss.index_add_(0, a[m], (0.5 - tau).clamp(min=0.0))
        relative = (eb.abs() / (c[m].abs() * d[b[m]].abs()[:, None, :]).sum(-1).clamp(min=1e-30)).amin(1)
        margin.index_reduce_(0, b[m], relative, "amin")
        margin.index_reduce_(0, a[m], relative, "amin")
    return torch.where(hit, (1.0 - loss).clamp(min=0.0), gain.clamp(max=1.0)).view(H, W), margin.view(H, W)


def main():
    dens, feat = sparse_scene_grid((G, G, G), 3 * (DEGREE + 1) ** 2, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), storage="split", density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0)
    intr = rf.CameraIntrinsics(800, 800, 1111.111)
    poses = rf.get_thre360_animation_poses(RADIUS, -30.0, VIEWS + 1)
    held_out = [rf.pose_spherical(yaw, pitch, RADIUS) for yaw, pitch in ((17.0, -50.0), (107.0, -12.0), (197.0, -45.0), (287.0, -8.0), (62.0, -70.0), (242.0, -20.0))]
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "iso_level": ISO, "runs": reps, "columns": "median, min, max ms", "views": VIEWS,
              "image": [800, 800], "fit_poses": f"turn-table, pitch -30, radius {RADIUS}", "held_out_poses": "6 poses at other yaws and pitches, 400 x 400"}
    with torch.no_grad():
        full = rf.extract_mesh(grid, ISO, subdivisions=2)
        h = np.float32(2 * VOXEL)
        lowest = full.vertices.amin(dim=0).cpu().numpy()
        origin = np.asarray([r[0] for r in grid.aabb], dtype=np.float32)
        origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
        mesh = rf.simplify_mesh(full, float(h), origin=origin.tolist())
        del full
        grid.build_occupancy()
        cfg = rf.SHVoxGridRenderConfig(512, rf.CameraBounds(NEAR, FAR), perturb_sampled_points=False, white_bkgd=False)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        depths, alphas = [], []
        for pose in poses:
            geometry = model.render_geometry(pose, intr, quantile=0.5, use_occupancy_mask=True)
            depths.append(geometry.depth[..., 0].float())
            alphas.append(geometry.extra[EXTRA_ACCUMULATED_WEIGHTS][..., 0].float())
        depths, alphas = torch.stack(depths).contiguous(), torch.stack(alphas).contiguous()
        V, T = mesh.vertices.shape[0], mesh.faces.shape[0]
        report.update({"V": V, "T": T})
        say(report, "T")

        renderer = rf.MeshGeometryRenderer(mesh.faces, poses, intr)
        vertices = mesh.vertices.contiguous()
        report["forward_ms"], (depth, coverage, face_ids) = timed(lambda: renderer._forward(vertices), reps)
        hits = int((face_ids >= 0).sum())
        report.update({"pixels": renderer.P, "hit_pixels": hits})
        one = rf.MeshGeometryRenderer(mesh.faces, poses[:1], intr)
        report["forward_one_view_ms"], (_, cover_one, ids_one) = timed(lambda: one._forward(vertices), reps)
        report["render_mesh_one_view_ms"], render = timed(lambda: rf.render_mesh(mesh, poses[0], intr, barycentrics=True), reps)
        report["torch_coverage_one_view_ms"], (t_cover, margin) = timed(lambda: torch_coverage(vertices, mesh.faces, render.face_ids, poses[0], intr), reps)
        difference = (t_cover - cover_one[0]).abs()
        off = difference > 1e-3
        report["torch_coverage_max_difference"] = float(difference.max())
        report["torch_coverage_pixels_off_by_more_than_1e-3"] = int(off.sum())
        report["torch_coverage_largest_margin_among_those"] = float(margin[off].max()) if bool(off.any()) else 0.0
        report["torch_coverage_max_difference_where_margin_above_1e-5"] = float(difference[margin > 1e-5].max()) if bool((margin > 1e-5).any()) else 0.0
        report["torch_coverage_pixels_off"] = [[int(i), int(j), float(difference[i, j]), float(margin[i, j])] for i, j in torch.nonzero(off)[:12].tolist()]
        report["torch_coverage_plus_render_over_kernel"] = round((report["torch_coverage_one_view_ms"][0] + report["render_mesh_one_view_ms"][0]) / report["forward_one_view_ms"][0], 2)
        for key in ("forward_ms", "forward_one_view_ms", "render_mesh_one_view_ms", "torch_coverage_one_view_ms", "torch_coverage_max_difference", "torch_coverage_pixels_off"):
            say(report, key)

        grad_depth, grad_coverage = torch.randn_like(depth) * 1e-3, torch.randn_like(coverage) * 1e-3
        report["backward_pixels_ms"], records = timed(lambda: renderer._records(vertices, face_ids, coverage, grad_depth, grad_coverage), reps)
        report["sort_ms"], (hit_pixels, face_offsets) = timed(lambda: renderer.hit_lists(face_ids), reps)
        renderer.corner_lists(V)
        report["backward_gather_ms"], grad = timed(lambda: renderer._gather(records, hit_pixels, face_offsets, V), reps)
        per_face = face_offsets[1:] - face_offsets[:-1]
        per_vertex = renderer.corner_lists(V)[1]
        per_vertex = per_vertex[1:] - per_vertex[:-1]
        report.update({"pixels_per_face_max": int(per_face.max()), "pixels_per_face_median_of_seen": int(per_face[per_face > 0].median()),
                       "faces_seen": int((per_face > 0).sum()), "corners_per_vertex_max": int(per_vertex.max())})
        report["backward_gather_ms_by_long_segment"] = {}
        worst = 0.0
        for threshold in THRESHOLDS:
            renderer.long_segment = threshold
            report["backward_gather_ms_by_long_segment"]["none" if threshold == 1 << 30 else str(threshold)], other = timed(lambda: renderer._gather(records, hit_pixels, face_offsets, V), reps)
            worst = max(worst, float((other - grad).abs().max()))
        renderer.long_segment = 0
        report["backward_gather_max_difference_between_thresholds"] = worst
        face_of_hit = face_ids.view(-1)[hit_pixels.to(torch.int64)].to(torch.int64)

        def torch_gather():
            per = torch.zeros((T, 9), device=dev).index_add_(0, face_of_hit, records[hit_pixels.to(torch.int64)])
            return torch.zeros((V, 3), device=dev).index_add_(0, mesh.faces.view(-1), per.view(-1, 3))
        report["torch_gather_ms"], t_grad = timed(torch_gather, reps)
        report["torch_gather_max_difference"] = float((t_grad - grad).abs().max())
        report["gradient_max_magnitude"] = float(grad.abs().max())
        report["torch_gather_over_kernel"] = round(report["torch_gather_ms"][0] / report["backward_gather_ms"][0], 2)
        for key in ("backward_pixels_ms", "sort_ms", "backward_gather_ms", "backward_gather_ms_by_long_segment", "torch_gather_ms", "torch_gather_over_kernel",
                    "pixels_per_face_max", "corners_per_vertex_max"):
            say(report, key)
        del records, grad, t_grad, depth, coverage, face_ids, grad_depth, grad_coverage, renderer, one

    cell = float(2 * VOXEL)
    one_it, _ = timed(lambda: rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, iterations=1, max_move=cell), 3, warm=1)
    six_it, _ = timed(lambda: rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, iterations=6, max_move=cell), 3, warm=1)
    report["fit_iteration_ms"] = round((six_it[0] - one_it[0]) / 5.0, 3)
    say(report, "fit_iteration_ms")

    edges = mf._edge_list(mesh.faces)
    edge_length = float((mesh.vertices[edges[:, 0]] - mesh.vertices[edges[:, 1]]).norm(dim=1).mean())
    report["mean_edge_length"] = edge_length
    report["loss_curves"] = {}
    marks = [0, 9, 29, SWEEP_ITERATIONS - 1]
    for fraction in LR_FRACTIONS:
        history = rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, iterations=SWEEP_ITERATIONS, lr=fraction * edge_length, max_move=cell).history.cpu().numpy()
        report["loss_curves"][f"{fraction:g}"] = {str(k + 1): float(history[k]) for k in marks}
    say(report, "loss_curves")
    report.update({"default_lr_fraction": mf.DEFAULT_LR_FRACTION, "quality_fit_iterations": FIT_ITERATIONS})

    fit = rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, iterations=FIT_ITERATIONS, max_move=cell)
    history = fit.history.cpu().numpy()
    report["fit_loss"] = [float(history[0]), float(history[-1])]
    report["fit_moved_mean_max_voxels"] = [float(fit.moved.mean()) / VOXEL, float(fit.moved.max()) / VOXEL]
    say(report, "fit_loss")
    small = rf.CameraIntrinsics(400, 400, 1111.111 / 2)
    with torch.no_grad():
        images = torch.stack([model.render(pose, intr, use_occupancy_mask=True).colour.float() for pose in poses]).contiguous()
        rows = {}
        for name, which in (("input_geometry", mesh), ("fitted_geometry", fit.mesh)):
            normal_bake = rf.bake_texture(which, grid, PATCH, reach=float(np.float32(3 * VOXEL)), samples=16, diffuse=True)
            rows[f"{name}_view_bake"] = (which, rf.bake_texture_from_views(which, images, poses, intr, PATCH, alphas=alphas, fallback=normal_bake).bake)
            if name == "input_geometry":
                rows["fitted_geometry_input_bake"] = (fit.mesh, rows[f"{name}_view_bake"][1])  # before re-baking: the old texture on the moved surface
        for name, (which, bake) in rows.items():
            metrics = rf.evaluate_mesh_against_field(which, bake, model, held_out, small, use_occupancy_mask=True)
            report[f"{name}_against_field_held_out"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
            say(report, f"{name}_against_field_held_out")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
