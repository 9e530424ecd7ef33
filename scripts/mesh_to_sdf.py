#!/usr/bin/env python
"""Turn a closed triangle mesh (a binary PLY as ``write_ply`` and the scripts of this project write them) into a signed distance volume
on a lattice of nodes, and optionally back into a mesh: the remeshed surface, or the surface --offset away from it
(thr3ed_atom_amd.mesh_sign: rf.mesh_to_sdf, MeshSDF.extract_mesh).  The distance is negative inside.

    python scripts/mesh_to_sdf.py -i mesh.ply --grid_dims 256 256 256 --truncation_voxels 3 --remesh remeshed.ply -o sdf.npz

The box defaults to the mesh's bounds grown by --margin_voxels voxels on every side.  Without --truncation_voxels every node gets its
exact distance; with it, nodes farther than that many (longest) voxel edges get +-truncation.  The .npz holds sdf [X, Y, Z] float32,
known [X, Y, Z] bool, aabb_min, aabb_max and truncation (NaN without one).  The sign is guaranteed for closed, consistently oriented
meshes only; --orientation auto takes inside / outside from the sign of the mesh's volume.
"""
import os
import sys
import time

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd.mesh import read_ply  # noqa: E402


# fmt: off
@click.command()
@click.option("-i", "--input_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="the .ply file of the mesh")
@click.option("--grid_dims", type=click.IntRange(min=1), nargs=3, required=True, help="nodes along x, y and z")
@click.option("--aabb_min", type=click.FLOAT, nargs=3, default=None, required=False, help="the box's lower corner (default: from the mesh)")
@click.option("--aabb_max", type=click.FLOAT, nargs=3, default=None, required=False, help="the box's upper corner (default: from the mesh)")
@click.option("--margin_voxels", type=click.FloatRange(min=0.0), default=2.0, required=False, help="voxels of free space round the mesh's bounds when the box is not given")
@click.option("--truncation_voxels", type=click.FloatRange(min=0.0), default=None, required=False, help="truncate the distance at this many (longest) voxel edges; more than 1.5")
@click.option("--orientation", type=click.Choice(["outward", "inward", "auto"]), default="outward", required=False, help="which way the mesh's face normals point")
@click.option("--remesh", type=click.Path(file_okay=True, dir_okay=False), default=None, required=False, help="write the surface extracted from the volume as a .ply file here")
@click.option("--offset", type=click.FLOAT, default=0.0, required=False, help="with --remesh: extract the surface this far outside (negative: inside) the mesh's")
@click.option("--subdivisions", type=click.IntRange(min=1, max=8), default=1, required=False, help="with --remesh: lattice points per voxel and axis")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), default=None, required=False, help="write the volume as .npz here")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    if (config["aabb_min"] is None) != (config["aabb_max"] is None):
        raise click.UsageError("give both --aabb_min and --aabb_max, or neither")
    dev = torch.device("cuda:0")
    vertices, _, _, faces = read_ply(config["input_path"])
    mesh = rf.Mesh(torch.from_numpy(np.ascontiguousarray(vertices)).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev), None, None)
    dims = tuple(int(d) for d in config["grid_dims"])
    if config["aabb_min"] is None:
        low, high = vertices.min(axis=0).astype(np.float64), vertices.max(axis=0).astype(np.float64)
        # the box whose voxels, margin included, cover the bounds: extent = bounds * n / (n - 2 margin)
        inner = np.maximum(np.asarray(dims, dtype=np.float64) - 2.0 * config["margin_voxels"], 1.0)
        pad = 0.5 * (np.maximum(high - low, 1e-6) * np.asarray(dims) / inner - (high - low))
        aabb_min, aabb_max = tuple(float(x) for x in low - pad), tuple(float(x) for x in high + pad)
    else:
        aabb_min, aabb_max = tuple(config["aabb_min"]), tuple(config["aabb_max"])
    topology = rf.mesh_topology(mesh)
    print(f"{config['input_path']}: V = {len(mesh.vertices)}, T = {len(mesh.faces)}, closed {topology.closed} ({topology.boundary_edges} boundary, "
          f"{topology.nonmanifold_edges} non-manifold, {topology.inconsistent_edges} inconsistent edges), signed volume {topology.signed_volume:.6g}")
    edge = max((b - a) / n for a, b, n in zip(aabb_min, aabb_max, dims))
    truncation = None if config["truncation_voxels"] is None else config["truncation_voxels"] * edge
    torch.cuda.synchronize()
    t0 = time.time()
    volume = rf.mesh_to_sdf(mesh, aabb_min, aabb_max, dims, truncation=truncation, orientation=config["orientation"])
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"{dims[0]} x {dims[1]} x {dims[2]} nodes in {volume.aabb[0]} .. {volume.aabb[1]}: {float(volume.known.double().mean()):.4f} known, "
          f"{float((volume.sdf < 0).double().mean()):.4f} inside, in {1e3 * dt:.1f} ms (incl. host synchronisation)")
    if config["output_path"]:
        os.makedirs(os.path.dirname(os.path.abspath(config["output_path"])), exist_ok=True)
        np.savez_compressed(config["output_path"], sdf=volume.sdf.cpu().numpy(), known=volume.known.cpu().numpy(), aabb_min=np.asarray(volume.aabb[0], np.float32),
                            aabb_max=np.asarray(volume.aabb[1], np.float32), truncation=np.float32(np.nan if volume.truncation is None else volume.truncation))
        print(f"-> {config['output_path']}")
    if config["remesh"]:
        out = volume.extract_mesh(config["offset"], config["subdivisions"])
        os.makedirs(os.path.dirname(os.path.abspath(config["remesh"])), exist_ok=True)
        rf.write_ply(out, config["remesh"])
        print(f"offset {config['offset']:.6g}: V = {len(out.vertices)}, T = {len(out.faces)} -> {config['remesh']}")


if __name__ == "__main__":
    main()
