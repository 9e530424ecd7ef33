#!/usr/bin/env python
"""Time of the iso-surface extraction (thr3ed_atom_amd.extract_mesh: count pass + scan + emit pass + face index lookup) on the
256^3 sparse scene of tests.helpers.sparse_scene_grid at subdivisions 1, 2 and 4 (level 5), reference and split storage.  HIP events
around the whole call (it synchronises once, to size the outputs), two warm-up calls per shape, median of N timed calls.  One JSON
line per configuration.

Bytes: the density channel is read once per lattice sigma -- 4 evaluations of 8 corners per lattice point (four staged runs per
workgroup), almost all from the caches; the floor is one pass over the channel: 4 B per node in the reference layout (67 MB at
256^3: fits the 256 MiB Infinity Cache) and the 16 B base record per node in split / bricked storage (268 MB: does not).
"density_floor_ms" = those bytes over the 6.29 TB/s measured HBM copy rate (8.0 TB/s spec).

    python tools/mesh_time.py [timed calls]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402

HBM_MEASURED = 6.29e12  # B/s, float4 copy
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G = 256
dens, feat = sparse_scene_grid((G, G, G), 27, 11)
voxel = 3.0 / G
# sigma reaches ~16.7 at the centre of this scene (0.5 * 100/3): the CLI's default level ln 2 / voxel = 59 would cut nothing, so the
# level is fixed at 5 (a surface near radius 0.35 of the half-extent)
iso = 5.0
for storage in ("reference", "split"):
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(voxel, voxel, voxel), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, storage=storage)
    node_bytes = 4 if storage == "reference" else 16
    for m in (1, 2, 4):
        for _ in range(2):
            mesh = rf.extract_mesh(grid, iso, subdivisions=m)
        times = []
        for _ in range(reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            mesh = rf.extract_mesh(grid, iso, subdivisions=m)
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
        times.sort()
        lattice = (m * G + 2) ** 3
        floor_bytes = G ** 3 * node_bytes
        print(json.dumps({"storage": storage, "grid": G, "subdivisions": m, "iso_level": round(iso, 4), "lattice_points": lattice,
                          "V": len(mesh.vertices), "T": len(mesh.faces), "median_ms": round(times[len(times) // 2], 3),
                          "min_ms": round(times[0], 3), "max_ms": round(times[-1], 3), "density_bytes_floor": floor_bytes,
                          "density_floor_ms": round(1e3 * floor_bytes / HBM_MEASURED, 4),
                          "lattice_points_per_s": round(lattice / (times[len(times) // 2] * 1e-3), -6)}), flush=True)
        del mesh
    del grid
    torch.cuda.empty_cache()
