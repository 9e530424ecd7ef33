#!/usr/bin/env python
"""Time and quality of the gradients of the mesh surface distance and of the Chamfer fit built on them
(thr3ed_atom_amd.mesh_distance_grad: rf_mesh_closest_gradients and the gather of rf_mesh_geometry_backward_gather) on the pair of
DESIGN.md section 27: the raw ``extract_mesh`` surface of the 256^3 sparse scene of tests.helpers.sparse_scene_grid (iso level 5, one
subdivision) and its ``simplify_mesh`` at two voxels, 10^6 area-weighted surface samples each way.  No trained field is needed: the
scene is synthetic and generated here.  HIP events on one device, two warm-up runs, then N timed runs per step, median / min / max ms:

    backward     per direction: rf_mesh_closest_gradients (with and without the records), the stable sort of the queries by face,
                 the gather (two launches) -- against the same backward in torch ops: a gather of the corners, the barycentric
                 formula and index_add_
    iteration    one rf.fit_mesh_to_mesh iteration at 10^5 and 10^6 samples: (6 iterations - 1 iteration) / 5, and the share of the
                 search-structure builds and of the two forward queries
    fit          Chamfer L1, the Hausdorff lower bound and the F-score at one voxel of the two-voxel and the four-voxel
                 simplification against the raw surface, before and after ``fit`` iterations (10^5 samples per iteration), with the
                 whole-frame numbers of rf.evaluate_mesh_against_field (vertex colours, 6 poses of 400 x 400) for the same meshes

Writes profiles/mesh_chamfer_time.json.

    python tools/mesh_chamfer_time.py [timed runs] [output json] [fit iterations]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import mesh_distance_grad as mdg  # noqa: E402
from thr3ed_atom_amd.mesh_distance import mesh_distance_dict  # noqa: E402
from thr3ed_atom_amd.mesh_fit import corner_slot_lists, gather_vertex_gradients  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mesh_chamfer_time.json")
FIT_ITERATIONS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, SAMPLES, FIT_SAMPLES = 256, 5.0, 1_000_000, 100_000
VOXEL = 3.0 / G
NEAR, FAR, RADIUS = float(np.float32(2.0) * 0.9), float(np.float32(6.0) * 1.1), 4.0311


def timed(fn, runs=None, warm=2):
    """(median, min, max) ms over the timed runs after the warm-ups, and the last result"""
    runs = reps if runs is None else runs
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


def torch_backward(points, vertices, faces, found, upstream, want_vertices):
    """the same backward in torch ops: gather the corners, barycentrics of the closest point by the area formula, index_add_"""
    has = found.face >= 0
    face = found.face.clamp(min=0)
    r = points - found.point
    length = r.norm(dim=1, keepdim=True)
    g = torch.where(has[:, None] & (length > 0), upstream[:, None] * r / length.clamp(min=1e-30), torch.zeros_like(r))
    if not want_vertices:
        return g, None
    idx = faces[face]
    c = vertices[idx]
    n = torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    nn = (n * n).sum(1).clamp(min=1e-30)
    q = found.point
    beta = torch.stack([(torch.linalg.cross(c[:, 2] - c[:, 1], q - c[:, 1]) * n).sum(1), (torch.linalg.cross(c[:, 0] - c[:, 2], q - c[:, 2]) * n).sum(1),
                        (torch.linalg.cross(c[:, 1] - c[:, 0], q - c[:, 0]) * n).sum(1)], 1) / nn[:, None]
    grad = torch.zeros_like(vertices)
    for k in range(3):
        grad.index_add_(0, idx[:, k], -beta[:, k:k + 1] * g)
    return g, grad


def backward_timings(name, mesh, points):
    """the backward of the distance of ``points`` to ``mesh``, step by step"""
    grid = rf.MeshDistanceGrid(mesh)
    found = grid.closest(points)
    N, V, T = points.shape[0], mesh.vertices.shape[0], mesh.faces.shape[0]
    upstream = torch.full((N,), 0.5 / N, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    grad_points, records = torch.empty((N, 3), device=dev), torch.empty((N, 9), device=dev)
    row = {"queries": N, "V": V, "T": T}
    row["closest_gradients_points_only_ms"], _ = timed(lambda: mdg.closest_gradients_raw(grid.vertices, grid.faces, points, found.face, upstream, status, grad_points=grad_points))
    row["closest_gradients_ms"], _ = timed(lambda: mdg.closest_gradients_raw(grid.vertices, grid.faces, points, found.face, upstream, status, grad_points=grad_points, records=records))
    row["sort_ms"], (entries, face_offsets) = timed(lambda: mdg.face_entry_lists(found.face, T))
    slots, vertex_offsets = corner_slot_lists(grid.faces, V)
    row["gather_ms"], grad = timed(lambda: gather_vertex_gradients(records, entries, face_offsets, T, slots, vertex_offsets, V, 0, status))
    per_face = face_offsets[1:] - face_offsets[:-1]
    row.update({"queries_per_face_max": int(per_face.max()), "faces_with_queries": int((per_face > 0).sum()), "status": int(status.item())})
    row["torch_points_only_ms"], _ = timed(lambda: torch_backward(points, grid.vertices, grid.faces, found, upstream, False))
    row["torch_ms"], (t_points, t_grad) = timed(lambda: torch_backward(points, grid.vertices, grid.faces, found, upstream, True))
    row["torch_max_difference"] = [float((t_points - grad_points).abs().max()), float((t_grad - grad).abs().max())]
    row["gradient_max_magnitude"] = [float(grad_points.abs().max()), float(grad.abs().max())]
    ours = row["closest_gradients_ms"][0] + row["sort_ms"][0] + row["gather_ms"][0]
    row["torch_over_kernels"] = round(row["torch_ms"][0] / ours, 2)
    row["torch_points_only_over_kernel"] = round(row["torch_points_only_ms"][0] / row["closest_gradients_points_only_ms"][0], 2)
    again = gather_vertex_gradients(records, entries, face_offsets, T, slots, vertex_offsets, V, 0, status)
    row["two_calls_give_equal_bits"] = bool(torch.equal(again, grad))
    return row


def iteration_timings(moving, target, samples):
    one, _ = timed(lambda: rf.fit_mesh_to_mesh(moving, target, iterations=1, samples=samples), 3, warm=1)
    six, _ = timed(lambda: rf.fit_mesh_to_mesh(moving, target, iterations=6, samples=samples), 3, warm=1)
    row = {"samples": samples, "fit_iteration_ms": round((six[0] - one[0]) / 5.0, 3), "one_iteration_call_ms": one}
    loss = rf.MeshChamferLoss(moving.faces, target, samples=samples)
    loss(moving.vertices)
    row["build_target_once_ms"], _ = timed(lambda: rf.MeshDistanceGrid(target), 3, warm=1)
    row["build_moving_ms"], grid = timed(lambda: rf.MeshDistanceGrid(moving, loss.cell_size), 3, warm=1)
    moving_points = rf.mesh_surface_points(moving.vertices, moving.faces, loss.sample_faces, loss.barycentrics)
    row["query_target_ms"], _ = timed(lambda: loss.target_grid.closest(moving_points), 3, warm=1)
    row["query_moving_ms"], _ = timed(lambda: grid.closest(loss.target_points), 3, warm=1)
    row["builds_and_queries_share"] = round((row["build_moving_ms"][0] + row["query_target_ms"][0] + row["query_moving_ms"][0]) / row["fit_iteration_ms"], 3)
    return row


def main():
    dens, feat = sparse_scene_grid((G, G, G), 27, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, storage="split")
    report = {"device": torch.cuda.get_device_name(dev), "scene": f"synthetic sparse scene of tests.helpers.sparse_scene_grid at {G}^3, iso level {ISO}, generated in the tool",
              "runs": reps, "columns": "median, min, max ms (HIP events, one device, two warm-up runs)", "samples": SAMPLES, "fit_iterations": FIT_ITERATIONS,
              "fit_samples": FIT_SAMPLES}
    with torch.no_grad():
        raw = rf.extract_mesh(grid, ISO, subdivisions=1)
        two, four = rf.simplify_mesh(raw, float(np.float32(2 * VOXEL))), rf.simplify_mesh(raw, float(np.float32(4 * VOXEL)))
        samples_raw, samples_two = rf.sample_mesh_surface(raw, SAMPLES, seed=1)[0], rf.sample_mesh_surface(two, SAMPLES, seed=0)[0]
        report["backward_moving_samples_to_raw"] = backward_timings("raw", raw, samples_two)
        say(report, "backward_moving_samples_to_raw")
        report["backward_raw_samples_to_moving"] = backward_timings("two-voxel", two, samples_raw)
        say(report, "backward_raw_samples_to_moving")
        del samples_raw, samples_two
    for samples in (FIT_SAMPLES, SAMPLES):
        report[f"iteration_{samples}"] = iteration_timings(two, raw, samples)
        say(report, f"iteration_{samples}")
    grid.build_occupancy()
    cfg = rf.SHVoxGridRenderConfig(512, rf.CameraBounds(NEAR, FAR), perturb_sampled_points=False, white_bkgd=False)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    held_out = [rf.pose_spherical(yaw, pitch, RADIUS) for yaw, pitch in ((17.0, -50.0), (107.0, -12.0), (197.0, -45.0), (287.0, -8.0), (62.0, -70.0), (242.0, -20.0))]
    small = rf.CameraIntrinsics(400, 400, 1111.111 / 2)
    for name, mesh in (("two_voxel", two), ("four_voxel", four)):
        fit = rf.fit_mesh_to_mesh(mesh, raw, iterations=FIT_ITERATIONS, samples=FIT_SAMPLES)
        history = fit.history.cpu().numpy()
        row = {"V": int(mesh.vertices.shape[0]), "T": int(mesh.faces.shape[0]), "loss": [float(history[0]), float(history[-1])],
               "moved_mean_max_voxels": [float(fit.moved.mean()) / VOXEL, float(fit.moved.max()) / VOXEL]}
        for when, which in (("before", mesh), ("after", fit.mesh)):
            distance = rf.mesh_distance(which, raw, samples=SAMPLES, thresholds=(VOXEL,), seed=1000)  # (a seed the fit never used)
            row[when] = {"chamfer_l1_voxels": distance.chamfer_l1 / VOXEL, "hausdorff_lower_bound_voxels": distance.hausdorff / VOXEL,
                         "fscore_at_one_voxel": distance.thresholds[0].fscore, "distance": mesh_distance_dict(distance)}
            with torch.no_grad():
                metrics = rf.evaluate_mesh_against_field(which, None, model, held_out, small, use_occupancy_mask=True)
            row[when]["against_field_held_out"] = {k: round(v, 4) for k, v in metrics.items() if k != "per_image"}
        report[f"fit_{name}"] = row
        say(report, f"fit_{name}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
