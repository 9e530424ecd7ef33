#!/usr/bin/env python
"""Extract the geometry of a trained model from what its VIEWS see instead of from the level set of its density: the median depth and
the accumulated weight of a turn-table of renders -- the camera path of scripts/render_mesh.py -- are fused into a truncated signed
distance volume on the GPU (rf.fuse_field_views) whose zero set is written as a coloured, closed triangle mesh
(binary PLY).  Haze that no ray accumulates to 1/2 leaves no shell, and a surface the views see as solid leaves no hole.

    python scripts/fuse_mesh.py -i out/saved_models/model_final.pth -o fused.ply --views 42
    python scripts/fuse_mesh.py -i model.pth -o fused.ply --views 42 --grid_dims 128 128 128 --truncation_voxels 4 --keep_largest 1 --simplify_voxels 2

--grid_dims defaults to the model's own grid; the box is always the model's.  --keep_largest N keeps the N largest connected components
(26-connectivity) of the nodes inside the fused surface; --simplify_voxels X simplifies the mesh by vertex clustering with cells of
X (smallest) edges of the fused lattice.
"""
import os
import sys
import time

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd.fusion import default_truncation  # noqa: E402


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path of the .ply file to write")
@click.option("--views", type=click.IntRange(min=1), default=42, required=False, help="frames of the turn-table that are fused")
@click.option("--grid_dims", type=click.IntRange(min=1, max=4096), nargs=3, default=None, required=False, help="nodes of the fused lattice (default: the model's grid)")
@click.option("--truncation_voxels", type=click.FloatRange(min=0.0, min_open=True), default=3.0, required=False, help="truncation distance in (longest) voxel edges of the fused lattice")
@click.option("--camera_pitch", type=click.FLOAT, default=60.0, required=False, help="pitch-angle value for the camera for 360 path animation")
@click.option("--render_scale_factor", type=click.FLOAT, default=1.0, required=False, help="scales the image size and the focal of the fused views")
@click.option("--subdivisions", type=click.IntRange(min=1, max=8), default=1, required=False, help="lattice points per voxel and axis of the extraction")
@click.option("--keep_largest", type=click.IntRange(min=1), default=None, required=False, help="keep only this many of the largest connected components inside the fused surface")
@click.option("--simplify_voxels", type=click.FloatRange(min=0.0, min_open=True), default=None, required=False, help="simplify the mesh by vertex clustering with cells of this many (smallest) voxel edges")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    dev = torch.device("cuda:0")
    creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
    model, extra = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
    intr = rf.scale_camera_intrinsics((extra or {}).get("camera_intrinsics", rf.CameraIntrinsics(800, 800, 1111.111)), config["render_scale_factor"])
    poses = rf.get_thre360_animation_poses((extra or {}).get("hemispherical_radius", 4.0311), config["camera_pitch"], config["views"] + 1)  # (the path drops its last frame)
    grid = model.thre3d_repr
    dims = tuple(config["grid_dims"]) if config["grid_dims"] else tuple(grid.grid_dims)
    truncation = default_truncation([r[0] for r in grid.aabb], [r[1] for r in grid.aabb], dims, config["truncation_voxels"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    volume = rf.fuse_field_views(model, poses, intr, dims, truncation=truncation)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    fused = volume.to_voxel_grid()
    if config["keep_largest"] is not None:
        stats = rf.remove_small_components(fused, 0.0, 26, keep_largest=config["keep_largest"], fill_density=-1.0)
        print(f"connected components inside the fused surface: {stats.components}, removed {stats.removed_components} ({stats.removed_nodes} nodes; {stats.kept_nodes} kept)")
    mesh = rf.extract_mesh(fused, 0.0, subdivisions=config["subdivisions"])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    extracted = (len(mesh.vertices), len(mesh.faces))
    if config["simplify_voxels"] is not None and len(mesh.faces):
        # cells aligned with the lattice, as scripts/extract_mesh_from_sh_based_voxel_grid.py aligns them with the voxels
        h = np.float32(config["simplify_voxels"] * min(fused.voxel_size))
        origin = np.asarray([r[0] for r in fused.aabb], dtype=np.float32)
        lowest = mesh.vertices.amin(dim=0).cpu().numpy()
        origin = origin - np.ceil(np.maximum(origin - lowest, 0.0) / h).astype(np.float32) * h
        origin = np.where(origin > lowest, origin - h, origin).astype(np.float32)
        mesh = rf.simplify_mesh(mesh, float(h), origin=origin.tolist())
        print(f"simplified (cells of {config['simplify_voxels']:g} voxels): V = {extracted[0]} -> {len(mesh.vertices)}, T = {extracted[1]} -> {len(mesh.faces)}")
    os.makedirs(os.path.dirname(os.path.abspath(config["output_path"])), exist_ok=True)
    rf.write_ply(mesh, config["output_path"])
    observed, hidden = int((volume.observed > 0).sum()), int(((volume.observed == 0) & (volume.hidden > 0)).sum())
    print(f"fused {len(poses)} views of {intr[0]}x{intr[1]} into {dims} nodes (truncation {truncation:.6g}): {observed} nodes observed, {hidden} hidden in every view that saw them, "
          f"{volume.tsdf.numel() - observed - hidden} never seen, in {1e3 * (t1 - t0):.1f} ms incl. the renders; V = {extracted[0]}, T = {extracted[1]} in {1e3 * (t2 - t1):.1f} ms "
          f"-> {config['output_path']}")


if __name__ == "__main__":
    main()
