#!/usr/bin/env python
"""Time of texture baking (thr3ed_atom_amd.bake_texture, rf_texture_bake) on the simplified meshes of DESIGN.md section 10's scene --
the 256^3 sparse scene of tests.helpers.sparse_scene_grid at level 5, subdivisions 2, vertex-clustered with cells of 2 and 4 voxels --
at patch 8 and 16, diffuse on and off, split and reference storage, 16 samples per texel, reach = the cell plus one voxel.  HIP
events, two warm-up runs, median of N timed runs, in a fresh process:

    whole    rf.bake_texture as a user calls it (checks, allocation, UVs, the launch, the status word's host read)
    kernel   rf_texture_bake alone into preallocated images

with the atlas size and the texels and samples per second of the kernel.  "torch" is a restatement with torch ops: the texel points
from integer arithmetic on the device, ops.grid_query on the sample points in chunks of 2^22, torch compositing (one warm-up, median
of 3; patch 8, specular only: its time does not depend on diffuse -- grid_query returns every channel) and the largest difference
between its texture and the kernel's.  Writes profiles/texture_bake_time.json.

    python tools/texture_bake_time.py [timed runs] [output json] [--no-torch]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from oracle.relu_field_oracle import sh_basis  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import _lib, ops, texture as tx  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "texture_bake_time.json")
with_torch = "--no-torch" not in sys.argv[3:]
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, SAMPLES, DEGREE = 256, 5.0, 16, 2
VOXEL = 3.0 / G
CHUNK = 1 << 22


def timed(fn, runs, warm=2):
    for _ in range(warm):
        result = fn()
    times = []
    for _ in range(runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)], result


def kernel_call(grid, mesh, layout, reach, diffuse, texture, opacity, status):
    rf_grid = grid.to_rf_grid()
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.load()

    def run():
        _lib.check(lib.rf_texture_bake(C.byref(rf_grid), mesh.vertices.data_ptr(), mesh.vertices.shape[0], mesh.faces.data_ptr(), mesh.faces.shape[0],
                                       layout.patch, layout.cols, layout.rows, reach, SAMPLES, _lib.FLAG_RENDER_DIFFUSE if diffuse else 0, texture.data_ptr(),
                                       opacity.data_ptr(), status.data_ptr(), stream), "rf_texture_bake")
    return run


def torch_restatement(grid, mesh, layout, reach):
    """the same bake with torch ops (specular), block-major texels in chunks; returns the texture [H, W, 3]"""
    P, B, T = layout.patch, layout.block, mesh.faces.shape[0]
    aabb = torch.tensor([[float(np.float32(lo)), float(np.float32(hi))] for lo, hi in grid.aabb], device=dev)
    texture = torch.zeros((layout.height, layout.width, 3), device=dev)
    delta = 2.0 * reach / SAMPLES
    ts = reach - (torch.arange(SAMPLES, device=dev, dtype=torch.float32) + 0.5) * delta
    total = layout.cols * layout.rows * B * B
    per = max(1, CHUNK // SAMPLES)
    for lo in range(0, total, per):
        t = torch.arange(lo, min(lo + per, total), device=dev)
        blk, r = t // (B * B), t % (B * B)
        j, i = r // B, r % B
        upper = i + j > P + 3
        tri = 2 * blk + upper
        own = tri < T
        t, blk, i, j, upper, tri = t[own], blk[own], i[own], j[own], upper[own], tri[own]
        v = mesh.vertices[mesh.faces[tri]]
        b1 = torch.where(upper, P + 2 - i, i - 1).float() / (P - 1)
        b2 = torch.where(upper, P + 2 - j, j - 1).float() / (P - 1)
        p = (1 - b1 - b2)[:, None] * v[:, 0] + b1[:, None] * v[:, 1] + b2[:, None] * v[:, 2]
        n = torch.linalg.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        length = n.norm(dim=1, keepdim=True)
        n = torch.where(length > 0, n / length.clamp_min(1e-30), torch.zeros_like(n))
        Y = sh_basis(DEGREE, -n)  # [M, K]
        q = (p[:, None, :] + ts[None, :, None] * n[:, None, :]).reshape(-1, 3)
        out = ops.grid_query(grid, q)
        inside = ((q > aabb[:, 0]) & (q < aabb[:, 1])).all(dim=1)
        sigma = torch.where(inside, out[:, -1], torch.zeros_like(out[:, -1])).reshape(-1, SAMPLES)
        colour = torch.sigmoid((out[:, :-1].reshape(-1, SAMPLES, 3, Y.shape[1]) * Y[:, None, None, :]).sum(-1))
        E = torch.exp(-sigma * delta)
        trans = torch.cumprod(torch.cat([torch.ones_like(E[:, :1]), E[:, :-1]], dim=1), dim=1)
        w = (1 - E) * trans
        base = torch.sigmoid((ops.grid_query(grid, p)[:, :-1].reshape(-1, 3, Y.shape[1]) * Y[:, None, :]).sum(-1))
        value = (w[..., None] * colour).sum(1) + (1 - w.sum(1, keepdim=True)) * base
        texture[(blk // layout.cols) * B + j, (blk % layout.cols) * B + i] = value
    return texture


def main():
    dens, feat = sparse_scene_grid((G, G, G), 3 * (DEGREE + 1) ** 2, 11)
    modes = dict(density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0)
    grids = {s: rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), storage=s, **modes) for s in ("split", "reference")}
    report = {"device": torch.cuda.get_device_name(dev), "grid": G, "iso_level": ISO, "subdivisions": 2, "samples": SAMPLES, "runs": reps,
              "columns": "median, min, max ms", "cells": {}}
    with torch.no_grad():
        full = rf.extract_mesh(grids["split"], ISO, subdivisions=2)
        lowest = full.vertices.amin(dim=0).cpu().numpy()
        for voxels in (2, 4):
            h = np.float32(voxels * VOXEL)
            origin = np.asarray([r[0] for r in grids["split"].aabb], dtype=np.float32)
            origin = (origin - np.ceil(np.maximum(origin - lowest, 0.0) / h + 1e-6).astype(np.float32) * h).astype(np.float32)
            mesh = rf.simplify_mesh(full, float(h), origin=origin.tolist())
            reach = float(np.float32((voxels + 1) * VOXEL))
            entry = {"V": len(mesh.vertices), "T": len(mesh.faces), "reach": reach, "bakes": []}
            for patch in (8, 16):
                layout = tx.atlas_layout(len(mesh.faces), patch)
                texels = layout.width * layout.height
                texture = torch.empty((layout.height, layout.width, 3), device=dev)
                opacity = torch.empty((layout.height, layout.width), device=dev)
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                for storage, grid in grids.items():
                    for diffuse in (False, True):
                        row = {"patch": patch, "storage": storage, "diffuse": diffuse, "atlas": [layout.width, layout.height], "texels": texels}
                        row["kernel_ms"], _ = timed(kernel_call(grid, mesh, layout, reach, diffuse, texture, opacity, status), reps)
                        kept = texture.clone()
                        row["whole_ms"], bake = timed(lambda: rf.bake_texture(mesh, grid, patch, reach=reach, samples=SAMPLES, diffuse=diffuse), reps)
                        row["whole_equals_kernel_bitwise"] = bool(torch.equal(bake.texture, kept))
                        seconds = row["kernel_ms"][0] * 1e-3
                        row["texels_per_s"] = round(texels / seconds, -6)
                        row["samples_per_s"] = round(texels * SAMPLES / seconds, -6)
                        if patch == 8 and not diffuse and with_torch:
                            row["torch_ms"], restated = timed(lambda: torch_restatement(grid, mesh, layout, reach), 3, warm=1)
                            row["torch_over_kernel"] = round(row["torch_ms"][0] / row["kernel_ms"][0], 1)
                            row["torch_max_difference"] = float((restated - kept).abs().max())
                            del restated
                        entry["bakes"].append(row)
                        print(json.dumps({"cell_voxels": voxels, **row}), flush=True)
                        del bake, kept
                        torch.cuda.empty_cache()
            report["cells"][f"{voxels} voxels"] = entry
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
