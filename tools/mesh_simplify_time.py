#!/usr/bin/env python
"""Time of mesh simplification (thr3ed_atom_amd.simplify_mesh) on the three meshes of DESIGN.md section 10 -- the 256^3 sparse scene
of tests.helpers.sparse_scene_grid at level 5, subdivisions 1, 2 and 4 -- with cells of 2 and 4 voxels aligned with the grid.  HIP
events, two warm-up runs, median of N timed runs, stage by stage:

    keys      rf_mesh_cluster_keys + torch.unique (clusters and the cluster of every vertex; one host synchronisation)
    sorts     the two stable sorts and bincounts that build the member and corner lists
    cluster   rf_mesh_cluster_vertices alone (the HIP hot path)
    faces     remap, drop, rotate, two stable sorts, de-duplicate
    whole     rf.simplify_mesh as a user calls it

"cluster_bytes" are the bytes the cluster kernel REQUESTS (68 per corner record: corner id, face, three vertices; 44 per member:
index, position, colour, normal; 76 per cluster) -- gathered vertices are served by the caches many times over, so this is an upper
bound of the HBM traffic, set against the 6.29 TB/s measured copy rate.  "torch" is the same representative computed with
index_add_ of float64 quadric columns and a batched torch.linalg.solve (no clamp, no attributes: a favourable restatement); its two
runs are compared bit for bit, as are two runs of the HIP pass.  "field_error" is the mean |sigma(x) - tau| over the output vertices
(ops.grid_query) for both placements.  Writes profiles/mesh_simplify_time.json.

    python tools/mesh_simplify_time.py [timed runs] [output json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import mesh_simplify as ms, ops  # noqa: E402

HBM_MEASURED = 6.29e12  # B/s, float4 copy
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mesh_simplify_time.json")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO = 256, 5.0
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


def torch_restatement(mesh, cluster, cluster_keys, lattice, regularisation=1e-3):
    """the quadric representative with torch ops: per-face normals once, index_add_ (float64 atomics) per corner, batched solve"""
    count = cluster_keys.numel()
    cells = torch.as_tensor(lattice.cells, device=dev)
    k = torch.stack([cluster_keys // (cells[1] * cells[2]), cluster_keys // cells[2] % cells[1], cluster_keys % cells[2]], -1)
    centre = torch.as_tensor(lattice.origin, device=dev).double() + (k.double() + 0.5) * float(lattice.h)
    p = mesh.vertices.double()
    corner_cluster = cluster[mesh.faces]  # [T, 3]
    A = torch.zeros((count, 9), dtype=torch.float64, device=dev)
    b = torch.zeros((count, 3), dtype=torch.float64, device=dev)
    for j in range(3):
        m = centre[corner_cluster[:, j]]
        q0, q1, q2 = (p[mesh.faces[:, i]] - m for i in range(3))
        n = torch.linalg.cross(q1 - q0, q2 - q0)
        d = (n * q0).sum(dim=1, keepdim=True)
        A.index_add_(0, corner_cluster[:, j], (n[:, :, None] * n[:, None, :]).reshape(-1, 9))
        b.index_add_(0, corner_cluster[:, j], d * n)
    sums = torch.zeros((count, 3), dtype=torch.float64, device=dev).index_add_(0, cluster, p - centre[cluster])
    xbar = sums / torch.bincount(cluster, minlength=count)[:, None]
    A = A.reshape(count, 3, 3)
    trace = A.diagonal(dim1=1, dim2=2).sum(dim=1)
    M = A + (regularisation * trace.clamp_min(1e-300))[:, None, None] * torch.eye(3, dtype=torch.float64, device=dev)
    delta = torch.linalg.solve(M, (b - (A @ xbar[:, :, None])[:, :, 0])[:, :, None])[:, :, 0]
    return (centre + xbar + delta).float()


def main():
    dens, feat = sparse_scene_grid((G, G, G), 27, 11)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, storage="split")
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "iso_level": ISO, "runs": reps, "columns": "median, min, max ms", "meshes": {}}
    with torch.no_grad():
        for m in (1, 2, 4):
            mesh = rf.extract_mesh(grid, ISO, subdivisions=m)
            V, T = len(mesh.vertices), len(mesh.faces)
            entry = {"V": V, "T": T, "ply_bytes": 27 * V + 13 * T, "cells": {}}
            lowest = mesh.vertices.amin(dim=0).cpu().numpy()
            for voxels in (2, 4):
                h = np.float32(voxels * VOXEL)
                origin = np.asarray([r[0] for r in grid.aabb], dtype=np.float32)
                origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
                bounds = ms._host_bounds(mesh)
                lattice = ms._lattice(bounds, h, origin)
                row = {}
                row["keys_ms"], (cluster_keys, cluster) = timed(lambda: ms._cluster_keys(mesh.vertices, lattice))
                count = cluster_keys.numel()
                row["sorts_ms"], lists = timed(lambda: ms._cluster_lists(cluster, mesh.faces, count))
                row["cluster_ms"], reps_out = timed(lambda: ms._cluster_vertices(mesh, lists, cluster_keys, lattice, "quadric", 1e-3))
                again = ms._cluster_vertices(mesh, lists, cluster_keys, lattice, "quadric", 1e-3)
                row["cluster_bitwise_repeatable"] = all(torch.equal(a, b) for a, b in zip(reps_out, again))
                row["faces_ms"], _ = timed(lambda: ms._cluster_faces(cluster, mesh.faces, count))
                row["whole_ms"], (out, stats) = timed(lambda: rf.simplify_mesh(mesh, float(h), origin=origin.tolist(), return_stats=True))
                requested = 68 * 3 * T + 44 * V + 76 * count
                row["cluster_bytes"] = requested
                row["cluster_bytes_per_s"] = round(requested / (row["cluster_ms"][0] * 1e-3), -9)
                row["cluster_fraction_of_hbm_copy_rate"] = round(requested / (row["cluster_ms"][0] * 1e-3) / HBM_MEASURED, 3)
                row["torch_ms"], first = timed(lambda: torch_restatement(mesh, cluster, cluster_keys, lattice))
                second = torch_restatement(mesh, cluster, cluster_keys, lattice)
                row["torch_bitwise_repeatable"] = bool(torch.equal(first, second))
                row["torch_over_hip"] = round(row["torch_ms"][0] / row["cluster_ms"][0], 2)
                row["clusters"], row["V_out"], row["T_out"] = count, stats.vertices, stats.faces
                row["collapsed_faces"], row["merged_duplicates"] = stats.collapsed_faces, stats.merged_duplicates
                row["ply_bytes_out"] = 27 * stats.vertices + 13 * stats.faces
                mean_out = rf.simplify_mesh(mesh, float(h), origin=origin.tolist(), placement="mean")
                row["field_error"] = {name: round(float((ops.grid_query(grid, o.vertices)[:, -1] - ISO).abs().mean()), 5) for name, o in (("quadric", out), ("mean", mean_out))}
                row["field_error_input"] = round(float((ops.grid_query(grid, mesh.vertices)[:, -1] - ISO).abs().mean()), 5)
                entry["cells"][f"{voxels} voxels"] = row
                print(json.dumps({"subdivisions": m, "cell_voxels": voxels, **row}), flush=True)
                del lists, reps_out, again, out, mean_out, first, second, cluster, cluster_keys
                torch.cuda.empty_cache()
            report["meshes"][f"m={m}"] = entry
            del mesh
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
