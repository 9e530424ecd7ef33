#!/usr/bin/env python
"""Tighten a trained ReLU field to its content: find the box of the nodes whose activated density exceeds a threshold, crop the
grid to it (plus a margin of nodes) and, with --num_nodes, resample the cropped box to about that many cubic voxels.

    python scripts/crop_sh_based_voxel_grid.py -i out/saved_models/model_final.pth -o cropped.pth --threshold 0 --margin 1
    python scripts/crop_sh_based_voxel_grid.py -i model.pth -o tight.pth --threshold 0 --num_nodes 2097152

The crop is exact (kept nodes keep their bits and their world positions).  Prints the dims and the bounding box before and after."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(exists=True, dir_okay=False), required=True, help="checkpoint written by the training script")
@click.option("-o", "--output_path", type=click.Path(dir_okay=False), required=True, help="where the cropped checkpoint goes")
@click.option("--threshold", type=click.FloatRange(min=0.0), required=False, default=0.0, help="a node is content when its activated density exceeds this (softplus fields need a positive value)")
@click.option("--margin", type=click.IntRange(min=0), required=False, default=1, help="nodes kept around the content box")
@click.option("--num_nodes", type=click.IntRange(min=1), required=False, default=None, help="resample the cropped box to about this many cubic voxels (default: keep the voxel size)")
# fmt: on
def main(**config) -> None:
    dev = torch.device("cuda", 0)
    model, extra = rf.create_volumetric_model_from_saved_model(Path(config["model_path"]), rf.create_voxel_grid_from_saved_info_dict, device=dev)
    new_grid, stats = rf.tighten_voxel_grid(model.thre3d_repr, config["threshold"], config["margin"], num_nodes=config["num_nodes"])
    if stats.passing_nodes == 0:
        print(f"no node above {config['threshold']}: the field is written unchanged")
    model.thre3d_repr = new_grid.to(dev)
    print(f"nodes above the threshold: {stats.passing_nodes}  margin: {config['margin']}")
    print(f"dims: {stats.old_dims} -> {stats.new_dims}")
    print(f"aabb: {tuple(stats.old_aabb)} -> {tuple(stats.new_aabb)}")
    torch.save(model.get_save_info(extra_info=extra), config["output_path"])


if __name__ == "__main__":
    main()
