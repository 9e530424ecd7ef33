#!/usr/bin/env python
"""Time of the mesh-to-mesh surface distance (thr3ed_atom_amd.mesh_distance: rf_mesh_grid_pairs, rf_mesh_closest_points) on the scene of
DESIGN.md sections 19 - 26: the raw ``extract_mesh`` surface of the 256^3 sparse scene of tests.helpers.sparse_scene_grid (iso level 5,
one subdivision) against its ``simplify_mesh`` at two voxels, 10^6 area-weighted surface samples of each against the other.  No trained
field is needed: the scene is synthetic and generated here.  HIP events on one device, two warm-up runs, then N timed runs per step,
median / min / max ms:

    build        MeshDistanceGrid of each mesh: the whole constructor, and its pairs launch and its sort alone
    query        closest() of the 10^6 samples of the other mesh: the whole call, and its query sort and its kernel alone, with the
                 histogram of the Chebyshev radius at which the queries stopped
    torch        the same rule as a chunked brute force in plain float32 torch ops on a subsample of the queries against ALL faces,
                 scaled to 10^6 queries -- what a user without the kernel would have to write -- and its largest difference
    distance     rf.mesh_distance of the pair, whole call

Writes profiles/mesh_distance_time.json.

    python tools/mesh_distance_time.py [timed runs] [output json]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import ops  # noqa: E402
from thr3ed_atom_amd.mesh_distance import _cells_of, _face_cell_counts, mesh_distance_dict  # noqa: E402  (the package attribute of that name is the function)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mesh_distance_time.json")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, SAMPLES, TORCH_QUERIES, TORCH_FACE_CHUNK = 256, 5.0, 1_000_000, 256, 1 << 18
VOXEL = 3.0 / G


def timed(fn):
    """(median, min, max) ms over `reps` runs after two warm-ups, and the last result"""
    for _ in range(2):
        result = fn()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)], result


def say(report, key):
    print(json.dumps({key: report[key]}), flush=True)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def torch_rule(p, a, b, c):
    """closest_on_face of csrc/mesh_distance.h in float32 torch ops: d2 [N, F] of queries p [N, 1, 3] against faces a, b, c [1, F, 3]"""
    lo, hi = torch.minimum(torch.minimum(a, b), c), torch.maximum(torch.maximum(a, b), c)

    def candidate(q):
        d = p - torch.minimum(torch.maximum(q, lo), hi)
        return dot(d, d)

    def segment(s, e):
        g, w = e - s, p - s
        l = dot(g, g)
        t = torch.where(l > 0, (dot(w, g) / l).clamp(0, 1), torch.zeros_like(l))
        return candidate(s + t[..., None] * g)

    best = torch.minimum(torch.minimum(segment(a, b), segment(b, c)), segment(c, a))
    n = torch.linalg.cross(b - a, c - a)
    nn = dot(n, n)
    q = p - (dot(p - a, n) / nn)[..., None] * n
    edge = lambda s, e: dot(torch.linalg.cross((e - s).expand_as(q), q - s), n)  # noqa: E731
    inside = (nn > 0) & (edge(a, b) >= 0) & (edge(b, c) >= 0) & (edge(c, a) >= 0)
    return torch.where(inside, torch.minimum(best, candidate(q)), best)


def torch_brute_force(points, mesh):
    """distance [N] and face [N]: the smallest d2 over all faces, chunked over the faces"""
    best = torch.full((points.shape[0],), math.inf, device=dev)
    face = torch.zeros(points.shape[0], dtype=torch.int64, device=dev)
    p = points[:, None, :]
    for first in range(0, mesh.faces.shape[0], TORCH_FACE_CHUNK):
        corners = mesh.vertices[mesh.faces[first:first + TORCH_FACE_CHUNK]]
        d2, at = torch_rule(p, corners[None, :, 0], corners[None, :, 1], corners[None, :, 2]).min(dim=1)
        better = d2 < best
        best, face = torch.where(better, d2, best), torch.where(better, at + first, face)
    return torch.sqrt(best), face


def kernel_only(grid, points):
    """the query sort and the launch of closest(), apart"""
    g = grid.lattice
    cell = _cells_of(points, g)
    key = (cell[:, 0] * int(g.cells[1]) + cell[:, 1]) * int(g.cells[2]) + cell[:, 2]
    sort_ms, order = timed(lambda: torch.sort(key).indices)
    N = points.shape[0]
    distance, face, point = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int64, device=dev), torch.empty((N, 3), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    launch = lambda o: ops.mesh_closest_points_raw(grid.vertices, grid.faces, g.origin, g.h, g.cells, grid.cell_begin, grid.cell_faces, points, o, math.inf,  # noqa: E731
                                                   distance, face, point, None, status)
    kernel_ms, _ = timed(lambda: launch(order))
    unsorted_ms, _ = timed(lambda: launch(None))
    return sort_ms, kernel_ms, unsorted_ms


def build_only(grid):
    """the pairs launch and the sort of MeshDistanceGrid, apart (the lists of ``grid`` give the offsets back)"""
    g, T = grid.lattice, grid.faces.shape[0]
    corners = grid.vertices[grid.faces]
    counts = _face_cell_counts(corners.amin(dim=1), corners.amax(dim=1), g)
    offsets = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, dim=0, out=offsets[1:])
    keys, faces = torch.empty(grid.pairs, dtype=torch.int64, device=dev), torch.empty(grid.pairs, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    pairs_ms, _ = timed(lambda: ops.mesh_grid_pairs_raw(grid.vertices, grid.faces, g.origin, g.h, g.cells, offsets, keys, faces, status))
    sort_ms, _ = timed(lambda: torch.sort(keys, stable=True))
    return pairs_ms, sort_ms


def main():
    dens, feat = sparse_scene_grid((G, G, G), 27, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, storage="split")
    report = {"device": torch.cuda.get_device_name(dev), "scene": f"synthetic sparse scene of tests.helpers.sparse_scene_grid at {G}^3, iso level {ISO}, generated in the tool",
              "runs": reps, "columns": "median, min, max ms (HIP events, one device, two warm-up runs)", "samples": SAMPLES}
    with torch.no_grad():
        raw = rf.extract_mesh(grid, ISO, subdivisions=1)
        raw = rf.Mesh(raw.vertices, raw.faces, None, None)
        small = rf.simplify_mesh(raw, float(np.float32(2 * VOXEL)))
        meshes = {"raw": raw, "simplified": small}
        samples = {name: rf.sample_mesh_surface(mesh, SAMPLES, seed=k)[0] for k, (name, mesh) in enumerate(meshes.items())}
        for name, mesh in meshes.items():
            other = "simplified" if name == "raw" else "raw"
            row = {"V": int(mesh.vertices.shape[0]), "T": int(mesh.faces.shape[0])}
            row["build_ms"], built = timed(lambda: rf.MeshDistanceGrid(mesh))
            row["cell_size"], row["cell_size_in_voxels"], row["cells"], row["pairs"] = built.cell_size, round(built.cell_size / VOXEL, 3), [int(c) for c in built.lattice.cells], built.pairs
            row["build_pairs_launch_ms"], row["build_sort_ms"] = build_only(built)
            points = samples[other]
            row["queries"] = f"{SAMPLES} surface samples of the {other} mesh"
            row["closest_call_ms"], (result, rings) = timed(lambda: built.closest(points, return_rings=True))
            row["query_sort_ms"], row["query_kernel_ms"], row["query_kernel_unsorted_queries_ms"] = kernel_only(built, points)
            row["rings_histogram"] = torch.bincount(rings.long()).cpu().tolist()
            row["mean_distance_in_voxels"] = round(float(result.distance.double().mean()) / VOXEL, 4)
            again = built.closest(points)
            row["two_calls_give_equal_bits"] = bool(torch.equal(again.distance, result.distance) and torch.equal(again.face, result.face) and torch.equal(again.point.nan_to_num(), result.point.nan_to_num()))
            subsample = points[:: SAMPLES // TORCH_QUERIES][:TORCH_QUERIES].contiguous()
            ms, (d, face) = timed(lambda: torch_brute_force(subsample, mesh))
            row["torch_brute_force_ms"] = {"queries": TORCH_QUERIES, "measured": ms, "scaled_to_all_queries": [round(t * SAMPLES / TORCH_QUERIES, 1) for t in ms]}
            kept = result.distance[:: SAMPLES // TORCH_QUERIES][:TORCH_QUERIES]
            row["torch_largest_distance_difference"] = float((d - kept).abs().max())
            row["torch_over_kernel"] = round(row["torch_brute_force_ms"]["scaled_to_all_queries"][0] / row["query_kernel_ms"][0], 1)
            row["torch_over_closest_call"] = round(row["torch_brute_force_ms"]["scaled_to_all_queries"][0] / row["closest_call_ms"][0], 1)
            report[f"queries_against_{name}"] = row
            say(report, f"queries_against_{name}")
        ms, result = timed(lambda: rf.mesh_distance(small, raw, samples=SAMPLES, thresholds=(VOXEL, 2 * VOXEL)))
        report["mesh_distance_call_ms"] = ms
        report["mesh_distance_simplified_against_raw"] = mesh_distance_dict(result)
        report["mesh_distance_simplified_against_raw"]["thresholds_are"] = "one and two voxels"
        say(report, "mesh_distance_call_ms")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
