#!/usr/bin/env python
"""Export the surface of a trained model as an oriented, coloured point cloud (binary PLY without faces): the median-depth points
of a ring of views, back-projected, with the composited surface normals and the rendered colours
(thr3ed_atom_amd.geometry.back_project_points).  Checkpoints written by this build OR by the reference load.

    python scripts/export_point_cloud_from_sh_based_voxel_grid.py -i out/saved_models/model_final.pth -o cloud.ply --num_views 24
"""
import os
import sys
import time

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402


# fmt: off
@click.command()
# Required arguments:
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path of the .ply file to write")
# Non-required options:
@click.option("--num_views", type=click.IntRange(min=1), default=24, required=False, help="views on a ring around the object")
@click.option("--camera_pitch", type=click.FLOAT, default=60.0, required=False, help="pitch-angle of the ring of views")
@click.option("--quantile", type=click.FloatRange(min=0.0, max=1.0, min_open=True, max_open=True), default=0.5, required=False, help="opacity quantile of the depth (0.5: median)")
@click.option("--min_acc", type=click.FLOAT, default=0.5, required=False, help="pixels below this accumulated weight give no point")
@click.option("--stride", type=click.IntRange(min=1), default=1, required=False, help="take every stride-th pixel of rows and columns")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    dev = torch.device("cuda:0")
    creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
    model, extra = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
    radius, intr = extra["hemispherical_radius"], extra["camera_intrinsics"]
    poses = rf.get_thre360_animation_poses(radius, config["camera_pitch"], config["num_views"] + 1)  # (the path drops its last pose)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    points, normals, colours = rf.back_project_points(model, poses, intr, quantile=config["quantile"], min_acc=config["min_acc"], stride=config["stride"])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(config["output_path"])), exist_ok=True)
    rf.write_point_cloud_ply(points, normals, colours, config["output_path"])
    print(f"{len(poses)} views of {intr.height}x{intr.width}: {len(points)} points in {1e3 * dt:.1f} ms -> {config['output_path']}")


if __name__ == "__main__":
    main()
