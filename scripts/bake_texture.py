#!/usr/bin/env python
"""Bake the appearance of a trained model onto a triangle mesh (a binary PLY as ``write_ply``, scripts/simplify_mesh.py and
scripts/extract_mesh_from_sh_based_voxel_grid.py write it) and write a textured OBJ: ``textured.obj``, ``textured.mtl`` and
``textured.png`` (thr3ed_atom_amd.texture).  Every triangle gets its own patch of ``--patch`` texels per leg in
a uniform atlas; every texel composites ``--samples`` samples of the field along the triangle's normal, from ``--reach_voxels``
(largest) voxel edges outside the surface to as far inside, against the colour of the surface point itself.

    python scripts/bake_texture.py -i model.pth --mesh small.ply -o textured
    python scripts/bake_texture.py -i model.pth --mesh small.ply -o textured --patch 16 --reach_voxels 3 --samples 32 --diffuse

--diffuse bakes the degree-0 colour only (what ``extract_mesh`` stores per vertex); without it the spherical harmonics are evaluated
for a camera that faces each triangle.

    python scripts/bake_texture.py -i model.pth --mesh small.ply -o textured --views 42
    python scripts/bake_texture.py -i model.pth --mesh small.ply -o textured --dataset_views -d scene.npz

--views N bakes from posed views instead (rf.bake_texture_from_field_views): the field is rendered over the
turn-table of scripts/render_mesh.py (--num_frames N there; camera of the checkpoint unless --view_height / --view_width / --view_focal /
--view_radius say otherwise, --camera_pitch as there) and the renders are projected onto the atlas through the mesh rasteriser's
depth test; texels that no view sees keep the normal-ray bake described above.  --dataset_views projects the training images with
their poses instead (rf.bake_texture_from_views; the data options are those of scripts/train_sh_based_voxel_grid.py, the same views
are held out).  --depth_bias (default: the mean edge length of the mesh), --min_cos and --cos_power are passed on.  Without --views and
--dataset_views the script does what it did before.

    python scripts/bake_texture.py -i model.pth --mesh small.ply -o textured --views 42 --fit_iterations 200

--fit_iterations N (with --views or --dataset_views) then fits the baked texture to those same views by N Adam steps through the mesh
render's texture gradient (rf.fit_texture / rf.fit_texture_to_field_views): --fit_lr, --fit_loss l2 | l1 and
--fit_dssim_weight are passed on.  Without it nothing of the fit is allocated or launched.
"""
import os
import sys
import time

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd.mesh import read_ply  # noqa: E402


def bake_from_views(config, model, extra, mesh, fallback, dev):
    """the view bake of --views / --dataset_views on top of the normal-ray bake ``fallback``"""
    common = dict(depth_bias=config["depth_bias"], min_cos=config["min_cos"], cos_power=config["cos_power"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if config["dataset_views"]:
        from train_sh_based_voxel_grid import load_datasets

        train, _ = load_datasets(config, dev)
        images = train.images.permute(0, 2, 3, 1)[..., :3].contiguous()
        poses = [rf.CameraPose(pose[:, :3], pose[:, 3:]) for pose in train.poses]
        out = rf.bake_texture_from_views(mesh, images, poses, train.camera_intrinsics, config["patch"], fallback=fallback, **common)
        source = f"{len(poses)} training images"
    else:
        intr = (extra or {}).get("camera_intrinsics", rf.CameraIntrinsics(800, 800, 1111.111))
        intr = rf.CameraIntrinsics(config["view_height"] or intr[0], config["view_width"] or intr[1], config["view_focal"] or intr[2])
        radius = config["view_radius"] or (extra or {}).get("hemispherical_radius", 4.0311)
        poses = rf.get_thre360_animation_poses(radius, config["camera_pitch"], config["views"])
        out = rf.bake_texture_from_field_views(mesh, model, poses, intr, config["patch"], fallback=fallback, **common)
        source = f"{len(poses)} renders of {intr[0]}x{intr[1]} (radius {radius:.6g}, pitch {config['camera_pitch']:.6g})"
    torch.cuda.synchronize()
    seen = float((out.views > 0).sum()) / max(int((fallback.texture.sum(-1) != 0).sum()), 1)
    print(f"view bake from {source}: {int((out.views > 0).sum())} texels seen (about {100 * seen:.1f} % of the non-black texels of the normal-ray bake), "
          f"{1e3 * (time.perf_counter() - t0):.1f} ms (incl. the renders and host synchronisation)")
    bake = out.bake
    if config["fit_iterations"]:
        fit = dict(iterations=config["fit_iterations"], lr=config["fit_lr"], loss=config["fit_loss"], dssim_weight=config["fit_dssim_weight"])
        t0 = time.perf_counter()
        if config["dataset_views"]:
            fitted = rf.fit_texture(mesh, bake, images, poses, train.camera_intrinsics, **fit)
        else:
            fitted = rf.fit_texture_to_field_views(mesh, bake, model, poses, intr, **fit)
        history = fitted.history.cpu()
        print(f"texture fit ({config['fit_loss']}, D-SSIM weight {config['fit_dssim_weight']:.6g}, lr {config['fit_lr']:.6g}): loss {float(history[0]):.6g} -> {float(history[-1]):.6g} "
              f"in {len(history)} iterations over {int((fitted.coverage > 0).sum())} texels, {1e3 * (time.perf_counter() - t0):.1f} ms (incl. the renders)")
        bake = fitted.bake
    return bake


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("--mesh", "mesh_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="the .ply mesh to texture")
@click.option("-o", "--output_stem", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path stem of the .obj / .mtl / .png files to write")
@click.option("--patch", type=click.IntRange(min=2, max=64), default=8, required=False, help="texel centres per leg of a triangle's patch")
@click.option("--reach_voxels", type=click.FloatRange(min=0.0), default=2.0, required=False, help="half length of a texel's ray, in (largest) voxel edges")
@click.option("--samples", type=click.IntRange(min=1, max=256), default=16, required=False, help="samples per texel")
@click.option("--diffuse", is_flag=True, default=False, help="bake the degree-0 colour only")
# Baking from posed views (off unless --views or --dataset_views is given):
@click.option("--views", type=click.IntRange(min=2), default=None, required=False, help="bake from the field's renders over the turn-table of scripts/render_mesh.py with this --num_frames")
@click.option("--dataset_views", is_flag=True, default=False, help="bake from the training images and their poses (data options as for training)")
@click.option("--view_height", type=click.IntRange(min=1), default=None, required=False, help="image height of the rendered views (default: the checkpoint's camera)")
@click.option("--view_width", type=click.IntRange(min=1), default=None, required=False, help="image width of the rendered views (default: the checkpoint's camera)")
@click.option("--view_focal", type=click.FLOAT, default=None, required=False, help="focal length of the rendered views in pixels (default: the checkpoint's camera)")
@click.option("--view_radius", type=click.FLOAT, default=None, required=False, help="radius of the camera path (default: the checkpoint's)")
@click.option("--camera_pitch", type=click.FLOAT, default=60.0, required=False, help="pitch-angle value for the camera of the turn-table")
@click.option("--depth_bias", type=click.FloatRange(min=0.0), default=None, required=False, help="how far behind the rasterised depth a texel may lie and still count as seen (default: the mean edge length)")
@click.option("--min_cos", type=click.FloatRange(min=0.0, max=1.0, max_open=True), default=0.1, required=False, help="views at a flatter angle to the face than this cosine do not count")
@click.option("--cos_power", type=click.IntRange(min=0, max=8), default=2, required=False, help="a view is weighted by the cosine to this power")
# Fitting the baked texture to the views it was baked from (off unless --fit_iterations is given):
@click.option("--fit_iterations", type=click.IntRange(min=0), default=0, required=False, help="Adam steps on the texture against the views of --views / --dataset_views")
@click.option("--fit_lr", type=click.FloatRange(min=0.0, min_open=True), default=rf.texture_fit.DEFAULT_LR, required=False, help="learning rate of the fit")
@click.option("--fit_loss", type=click.Choice(["l2", "l1"]), default="l2", required=False, help="the per-pixel loss of the fit")
@click.option("--fit_dssim_weight", type=click.FloatRange(min=0.0, max=1.0), default=0.0, required=False, help="weight of 1 - SSIM in the loss of the fit")
@click.option("-d", "--data_path", type=click.Path(), required=False, default=None, help=".npz with images, poses, focal, near, far (as for training)")
@click.option("--data_downsample_factor", type=click.FloatRange(min=1.0), required=False, default=1.0, help="downscale factor for the input images")
@click.option("--synthetic", type=click.BOOL, required=False, default=False, help="the procedural scene of the training script")
@click.option("--synthetic_size", type=click.INT, required=False, default=200, help="image size of the synthetic scene")
@click.option("--train_num_samples_per_ray", type=click.INT, required=False, default=512, help="(as for training: sample count of the synthetic scene's images)")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    if config["views"] is not None and config["dataset_views"]:
        raise click.UsageError("--views and --dataset_views exclude each other")
    if config["fit_iterations"] and config["views"] is None and not config["dataset_views"]:
        raise click.UsageError("--fit_iterations needs --views or --dataset_views")
    dev = torch.device("cuda:0")
    creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
    model, extra = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
    grid = model.thre3d_repr
    vertices, normals, _, faces = read_ply(config["mesh_path"])
    on_device = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    mesh = rf.Mesh(on_device(vertices), on_device(faces), None, on_device(normals) if np.any(normals) else None)
    reach = config["reach_voxels"] * max(grid.voxel_size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bake = rf.bake_texture(mesh, model, config["patch"], reach=reach, samples=config["samples"], diffuse=config["diffuse"], opacity=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if config["views"] is not None or config["dataset_views"]:
        bake = bake_from_views(config, model, extra, mesh, bake, dev)
    rf.write_obj(mesh, bake, config["output_stem"])
    print(f"V = {len(mesh.vertices)}, T = {len(mesh.faces)}: atlas {bake.cols * bake.block} x {bake.rows * bake.block} (patch {bake.patch}, {bake.cols} x {bake.rows} blocks), "
          f"reach {reach:.6g}, {config['samples']} samples, {'diffuse' if config['diffuse'] else 'specular'} in {1e3 * dt:.1f} ms (incl. host synchronisation) "
          f"-> {config['output_stem']}.obj / .mtl / .png")


if __name__ == "__main__":
    main()
