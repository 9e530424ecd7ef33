#!/usr/bin/env python
"""Render a turn-table of an exported mesh with the HIP rasteriser (rf.render_mesh) -- the camera path of
scripts/render_sh_based_voxel_grid.py -- and, with --compare, say how far the mesh is from the field it came from
(rf.evaluate_mesh_against_field: PSNR, SSIM, depth L1, mask IoU).  Takes the OBJ / MTL / texture triple that scripts/bake_texture.py
writes (--obj STEM, textured) or a PLY written by scripts/extract_mesh_from_sh_based_voxel_grid.py / scripts/simplify_mesh.py (--mesh,
vertex colours).  Frames are written as PNG files (PIL) or, without PIL, as .npy.

    python scripts/render_mesh.py --obj textured -o frames --num_frames 42
    python scripts/render_mesh.py --mesh small.ply -o frames --num_frames 42 --compare out/saved_models/model_final.pth
"""
import json
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
@click.option("--obj", "obj_stem", type=click.Path(), default=None, help="stem of the .obj / .mtl / texture triple write_obj wrote (with or without the .obj suffix)")
@click.option("--mesh", "ply_path", type=click.Path(file_okay=True, dir_okay=False), default=None, help="a PLY written by write_ply (vertex colours)")
@click.option("-o", "--output_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="path for saving rendered output")
@click.option("--compare", "model_path", type=click.Path(file_okay=True, dir_okay=False), default=None, help="a trained model: also write metrics.json (mesh against field over the frames); its camera replaces --height / --width / --focal / --radius")
@click.option("--height", type=click.IntRange(min=1), default=800, help="image height")
@click.option("--width", type=click.IntRange(min=1), default=800, help="image width")
@click.option("--focal", type=click.FLOAT, default=1111.111, help="focal length in pixels")
@click.option("--radius", type=click.FLOAT, default=4.0311, help="radius of the camera path")
@click.option("--render_scale_factor", type=click.FLOAT, default=1.0, help="scales the image size and the focal")
@click.option("--camera_pitch", type=click.FLOAT, default=60.0, help="pitch-angle value for the camera for 360 path animation")
@click.option("--num_frames", type=click.IntRange(min=1), default=180, help="number of frames")
@click.option("--near", type=click.FLOAT, default=0.0, help="faces with a corner nearer than this are not drawn")
@click.option("--white_bkgd", is_flag=True, default=False, help="white background (default: the model's with --compare, else black)")
@click.option("--cull_backfaces", is_flag=True, default=False, help="draw only the faces whose normal looks at the camera")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    if (config["obj_stem"] is None) == (config["ply_path"] is None):
        raise click.UsageError("give exactly one of --obj and --mesh")
    dev = torch.device("cuda:0")
    if config["obj_stem"] is not None:
        stem = config["obj_stem"][:-4] if config["obj_stem"].endswith(".obj") else config["obj_stem"]
        mesh, bake = rf.read_obj(stem, device=dev)
    else:
        vertices, normals, colours, faces = read_ply(config["ply_path"])
        mesh = rf.Mesh(torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(colours.astype(np.float32) / np.float32(255.0)).to(dev),
                       torch.from_numpy(normals).to(dev))
        bake = None
    intr = rf.CameraIntrinsics(config["height"], config["width"], config["focal"])
    radius, white, model = config["radius"], config["white_bkgd"], None
    if config["model_path"] is not None:
        creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
        model, extra = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
        radius, intr = extra["hemispherical_radius"], extra["camera_intrinsics"]
        white = white or bool(getattr(model.render_config, "white_bkgd", False))
    intr = rf.scale_camera_intrinsics(intr, config["render_scale_factor"])
    poses = rf.get_thre360_animation_poses(radius, config["camera_pitch"], config["num_frames"])
    os.makedirs(config["output_path"], exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, pose in enumerate(poses):
        out = rf.render_mesh(mesh, pose, intr, bake, near=config["near"], white_bkgd=white, cull_backfaces=config["cull_backfaces"])
        frame = (out.colour.clamp(0, 1) * 255).byte().cpu().numpy()
        if Image is not None:
            Image.fromarray(frame).save(os.path.join(config["output_path"], f"frame_{i:04d}.png"))
        else:
            np.save(os.path.join(config["output_path"], f"frame_{i:04d}.npy"), frame)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{len(poses)} frames of {intr.height}x{intr.width}, {mesh.faces.shape[0]} faces, in {dt:.2f} s ({len(poses) / dt:.1f} fps incl. host copies and image encoding)")
    if model is not None:
        metrics = rf.evaluate_mesh_against_field(mesh, bake, model, poses, intr, white_bkgd=white)
        with open(os.path.join(config["output_path"], "metrics.json"), "w") as fh:
            json.dump(metrics, fh, indent=1)
            fh.write("\n")
        print({k: v for k, v in metrics.items() if k != "per_image"})


if __name__ == "__main__":
    main()
