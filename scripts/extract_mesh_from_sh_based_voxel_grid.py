#!/usr/bin/env python
"""Extract the geometry of a trained model as a coloured, closed triangle mesh (binary PLY) -- the iso-surface sigma = iso_level
of the ReLU field sampled at sub-voxel resolution on the GPU (thr3ed_atom_amd.mesh).  Checkpoints written by this build OR by the
reference load (create_volumetric_model_from_saved_model maps the reference's pickled names).

    python scripts/extract_mesh_from_sh_based_voxel_grid.py -i out/saved_models/model_final.pth -o mesh.ply --subdivisions 2
    python scripts/extract_mesh_from_sh_based_voxel_grid.py -i model.pth -o mesh.ply --keep_largest 1

    python scripts/extract_mesh_from_sh_based_voxel_grid.py -i model.pth -o mesh.ply --simplify_voxels 2
    python scripts/extract_mesh_from_sh_based_voxel_grid.py -i model.pth -o mesh.ply --target_faces 200000

--simplify_voxels X / --target_faces N simplify the mesh on the GPU before it is written (thr3ed_atom_amd.mesh_simplify: vertex
clustering with quadric-error representatives): cells of X * min(voxel_size) that start at the grid's AABB minimum, so the clusters
align with the voxels, or the finest cells that leave at most N faces.  Off by default.

--texture_patch P also writes a textured OBJ beside the PLY (mesh.obj, mesh.mtl, mesh.png for -o mesh.ply): the appearance of the field
baked onto the written mesh -- after the simplification when that is on -- by thr3ed_atom_amd.texture with P texel centres per triangle
leg, --texture_samples samples per texel and a ray of --texture_reach_voxels (smallest) voxel edges to either side of the surface
(default: the simplification cell plus one voxel; two voxels without simplification).  Unset, nothing changes.
--texture_views N (with --texture_patch) then re-bakes the texels a camera sees from the field's own renders over the turn-table of
scripts/render_mesh.py with --num_frames N and the checkpoint's camera (rf.bake_texture_from_field_views); the
texels no view sees keep the normal-ray bake.  --texture_fit_iterations N (with --texture_views) then fits the texture to those same
renders by N Adam steps on the L2 error of the mesh render (rf.fit_texture_to_field_views); unset, nothing of the
fit is allocated or launched.  scripts/bake_texture.py has the remaining options.

--geometry_fit_iterations N moves the (simplified) mesh's vertices towards the field's own median depth and accumulated weight over a
turn-table of --geometry_fit_views frames by N Adam steps (rf.fit_mesh_to_field_views), each vertex at most one
clustering cell (two voxels without simplification) from where it started.  It runs after the simplification and before any texture
bake, so the bake sees the fitted surface.  Off by default: unset, nothing of it is allocated or launched.

--fuse_views N replaces the density iso-surface by the surface the field's VIEWS see: the median depth and accumulated weight of a
turn-table of N frames are fused into a truncated signed distance volume on the model's grid (rf.fuse_field_views; DESIGN.md section
26; truncation --fuse_truncation_voxels longest voxel edges) and its zero set is extracted instead; --keep_largest /
--min_component_nodes then filter the components inside the fused surface, and the simplification, fit and bake options act on the
fused mesh as on any other.  Unset, the script does exactly what it does without the option.  scripts/fuse_mesh.py has the
remaining options.

--keep_largest / --min_component_nodes drop the detached shells of floaters: the connected components (26-connectivity) of the nodes
whose own density exceeds the iso level are filtered in memory before the extraction (thr3ed_atom_amd.components); the checkpoint is
not touched.
"""
import math
import os
import sys
import time

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402


# fmt: off
@click.command()
# Required arguments:
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path of the .ply file to write")
# Non-required extraction options:
@click.option("--iso_level", type=click.FLOAT, default=None, required=False,
              help="density of the surface; default ln 2 / min(voxel_size): a one-voxel slab at that density is 50 % opaque")
@click.option("--subdivisions", type=click.IntRange(min=1, max=8), default=2, required=False, help="lattice points per voxel and axis (sub-voxel surfaces of the ReLU field)")
@click.option("--keep_largest", type=click.IntRange(min=1), default=None, required=False, help="keep only this many of the largest connected components of the nodes above the iso level")
@click.option("--min_component_nodes", type=click.IntRange(min=1), default=None, required=False, help="drop the connected components with fewer nodes above the iso level than this")
@click.option("--fill_density", type=click.FLOAT, default=None, required=False, help="raw density of an emptied node (default 0; required for softplus fields, e.g. -10)")
@click.option("--simplify_voxels", type=click.FloatRange(min=0.0, min_open=True), default=None, required=False,
              help="simplify the mesh by vertex clustering with cells of this many (smallest) voxel edges, aligned with the grid")
@click.option("--target_faces", type=click.IntRange(min=0), default=None, required=False, help="simplify the mesh to at most this many faces")
@click.option("--simplify_placement", type=click.Choice(["quadric", "mean"]), default="quadric", required=False, help="where a cluster's vertex goes")
@click.option("--texture_patch", type=click.IntRange(min=2, max=64), default=None, required=False, help="also write a textured OBJ with this many texel centres per triangle leg")
@click.option("--texture_reach_voxels", type=click.FloatRange(min=0.0), default=None, required=False, help="half length of a texel's ray, in (smallest) voxel edges")
@click.option("--texture_samples", type=click.IntRange(min=1, max=256), default=16, required=False, help="samples per texel")
@click.option("--texture_views", type=click.IntRange(min=2), default=None, required=False, help="with --texture_patch: re-bake the seen texels from the field's renders over a turn-table of this many frames")
@click.option("--texture_fit_iterations", type=click.IntRange(min=0), default=0, required=False, help="with --texture_views: then fit the texture to those renders by this many Adam steps")
@click.option("--geometry_fit_iterations", type=click.IntRange(min=0), default=0, required=False, help="fit the vertices to the field's depth and alpha renders by this many Adam steps")
@click.option("--geometry_fit_views", type=click.IntRange(min=2), default=42, required=False, help="with --geometry_fit_iterations: frames of the turn-table the fit looks from")
@click.option("--fuse_views", type=click.IntRange(min=1), default=None, required=False, help="extract the surface fused from this many turn-table views of the field instead of the density iso-surface")
@click.option("--fuse_truncation_voxels", type=click.FloatRange(min=0.0, min_open=True), default=3.0, required=False, help="with --fuse_views: truncation distance in (longest) voxel edges")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    if config["simplify_voxels"] is not None and config["target_faces"] is not None:
        raise click.UsageError("--simplify_voxels and --target_faces exclude each other")
    filtering = config["keep_largest"] is not None or config["min_component_nodes"] is not None
    if filtering and config["iso_level"] is not None and config["iso_level"] < 0.0:
        raise click.UsageError("--keep_largest / --min_component_nodes need a non-negative --iso_level (the occupancy threshold of the components)")
    dev = torch.device("cuda:0")
    creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
    if config["texture_views"] is not None and config["texture_patch"] is None:
        raise click.UsageError("--texture_views needs --texture_patch")
    if config["texture_fit_iterations"] and config["texture_views"] is None:
        raise click.UsageError("--texture_fit_iterations needs --texture_views")
    model, extra = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
    grid = model.thre3d_repr
    iso = config["iso_level"]
    if iso is None:
        iso = math.log(2.0) / min(grid._voxel_size)
    source = grid  # what is meshed, and at which level
    if config["fuse_views"] is not None:
        from thr3ed_atom_amd.fusion import default_truncation

        intr = (extra or {}).get("camera_intrinsics", rf.CameraIntrinsics(800, 800, 1111.111))
        poses = rf.get_thre360_animation_poses((extra or {}).get("hemispherical_radius", 4.0311), 60.0, config["fuse_views"] + 1)  # (the path drops its last frame)
        truncation = default_truncation([r[0] for r in grid.aabb], [r[1] for r in grid.aabb], grid.grid_dims, config["fuse_truncation_voxels"])
        volume = rf.fuse_field_views(model, poses, intr, truncation=truncation)
        source, iso = volume.to_voxel_grid(), 0.0
        print(f"fused {len(poses)} views of {intr[0]}x{intr[1]} (truncation {truncation:.6g}): {int((volume.observed > 0).sum())} of {volume.tsdf.numel()} nodes observed")
        if filtering:
            stats = rf.remove_small_components(source, 0.0, 26, min_nodes=config["min_component_nodes"], keep_largest=config["keep_largest"], fill_density=-1.0)
            print(f"connected components inside the fused surface: {stats.components}, removed {stats.removed_components} ({stats.removed_nodes} nodes; {stats.kept_nodes} kept)")
    elif filtering:
        stats = rf.remove_small_components(grid, iso, 26, min_nodes=config["min_component_nodes"], keep_largest=config["keep_largest"], fill_density=config["fill_density"])
        print(f"connected components above the iso level: {stats.components}, removed {stats.removed_components} ({stats.removed_nodes} nodes; {stats.kept_nodes} kept)")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = rf.extract_mesh(source, iso, subdivisions=config["subdivisions"])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    extracted, summary = (len(mesh.vertices), len(mesh.faces)), ""
    cell_voxels = None
    if (config["simplify_voxels"] is not None or config["target_faces"] is not None) and len(mesh.faces):
        t1 = time.perf_counter()
        if config["target_faces"] is not None:
            mesh, stats = rf.simplify_mesh(mesh, target_faces=config["target_faces"], placement=config["simplify_placement"], return_stats=True)
        else:
            # cells aligned with the voxels: the origin is the AABB minimum, moved down by whole cells where the surface's guard
            # layer reaches below it
            h = np.float32(config["simplify_voxels"] * min(grid.voxel_size))
            origin = np.asarray([r[0] for r in grid.aabb], dtype=np.float32)
            lowest = mesh.vertices.amin(dim=0).cpu().numpy()
            origin = origin - np.ceil(np.maximum(origin - lowest, 0.0) / h).astype(np.float32) * h
            origin = np.where(origin > lowest, origin - h, origin).astype(np.float32)  # (float32 rounding of the step)
            mesh, stats = rf.simplify_mesh(mesh, float(h), origin=origin.tolist(), placement=config["simplify_placement"], return_stats=True)
        torch.cuda.synchronize()
        cell_voxels = stats.cell_size / min(grid.voxel_size)
        summary = (f"simplified ({config['simplify_placement']}, cell size {stats.cell_size:.6g}): V = {extracted[0]} -> {len(mesh.vertices)}, "
                   f"T = {extracted[1]} -> {len(mesh.faces)} in {1e3 * (time.perf_counter() - t1):.1f} ms\n")
    if config["geometry_fit_iterations"] and len(mesh.faces):
        t3 = time.perf_counter()
        intr = (extra or {}).get("camera_intrinsics", rf.CameraIntrinsics(800, 800, 1111.111))
        poses = rf.get_thre360_animation_poses((extra or {}).get("hemispherical_radius", 4.0311), 60.0, config["geometry_fit_views"] + 1)  # (the path drops its last frame)
        cell = (2.0 if cell_voxels is None else cell_voxels) * min(grid.voxel_size)
        fitted = rf.fit_mesh_to_field_views(mesh, model, poses, intr, iterations=config["geometry_fit_iterations"], max_move=cell)
        history = fitted.history.cpu()
        mesh = fitted.mesh
        torch.cuda.synchronize()
        summary += (f"geometry: fitted to {len(poses)} views of the field, loss {float(history[0]):.6g} -> {float(history[-1]):.6g} in {len(history)} iterations, vertices moved "
                    f"{float(fitted.moved.mean()):.4g} on average and at most {float(fitted.moved.max()):.4g} (limit {cell:.4g}) in {1e3 * (time.perf_counter() - t3):.1f} ms\n")
    out_dir = os.path.dirname(os.path.abspath(config["output_path"]))
    os.makedirs(out_dir, exist_ok=True)
    rf.write_ply(mesh, config["output_path"])
    print(summary, end="")
    if config["texture_patch"] is not None and len(mesh.faces):
        reach_voxels = config["texture_reach_voxels"]
        if reach_voxels is None:
            reach_voxels = 2.0 if cell_voxels is None else cell_voxels + 1.0
        t2 = time.perf_counter()
        bake = rf.bake_texture(mesh, grid, config["texture_patch"], reach=reach_voxels * min(grid.voxel_size), samples=config["texture_samples"], opacity=False)
        if config["texture_views"] is not None:
            intr = (extra or {}).get("camera_intrinsics", rf.CameraIntrinsics(800, 800, 1111.111))
            poses = rf.get_thre360_animation_poses((extra or {}).get("hemispherical_radius", 4.0311), 60.0, config["texture_views"])
            views = rf.bake_texture_from_field_views(mesh, model, poses, intr, config["texture_patch"], fallback=bake)
            print(f"texture: {int((views.views > 0).sum())} texels re-baked from {len(poses)} renders of {intr[0]}x{intr[1]}")
            bake = views.bake
            if config["texture_fit_iterations"]:
                fitted = rf.fit_texture_to_field_views(mesh, bake, model, poses, intr, iterations=config["texture_fit_iterations"])
                history = fitted.history.cpu()
                print(f"texture: fitted to the same renders, L2 loss {float(history[0]):.6g} -> {float(history[-1]):.6g} in {len(history)} iterations")
                bake = fitted.bake
        torch.cuda.synchronize()
        stem = os.path.splitext(config["output_path"])[0]
        rf.write_obj(mesh, bake, stem)
        print(f"texture: atlas {bake.cols * bake.block} x {bake.rows * bake.block} (patch {bake.patch}), reach {reach_voxels:.4g} voxels, {config['texture_samples']} samples "
              f"in {1e3 * (time.perf_counter() - t2):.1f} ms -> {stem}.obj / .mtl / .png")
    print(f"grid {grid.grid_dims}, iso_level {iso:.6g}, subdivisions {config['subdivisions']}: V = {extracted[0]}, T = {extracted[1]} "
          f"in {1e3 * dt:.1f} ms (extraction incl. host synchronisation) -> {config['output_path']}")


if __name__ == "__main__":
    main()
