#!/usr/bin/env python
"""Prune a trained ReLU field by visibility: render the training views, record per grid node the largest compositing weight any
ray gave it, and empty the nodes that stay at or below a threshold (with threshold 0: the nodes no view ever weighted).

    python scripts/prune_sh_based_voxel_grid.py -i out/saved_models/model_final.pth -o pruned.pth --threshold 1e-3 --dilate 1 --synthetic True
    python scripts/prune_sh_based_voxel_grid.py -i model.pth -o pruned.pth -d scene.npz --threshold 0

The data options are those of scripts/train_sh_based_voxel_grid.py (the same views are held out).  Prints the kept / pruned node
counts and the number of occupied cells (rf_build_occupancy) before and after."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thr3ed_atom_amd as rf  # noqa: E402
from train_sh_based_voxel_grid import load_datasets  # noqa: E402


def occupied_cells(grid) -> int:
    words = grid.build_occupancy()
    return int(sum(int(((words >> b) & 1).sum()) for b in range(32)))


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(exists=True, dir_okay=False), required=True, help="checkpoint written by the training script")
@click.option("-o", "--output_path", type=click.Path(dir_okay=False), required=True, help="where the pruned checkpoint goes")
@click.option("--threshold", type=click.FloatRange(min=0.0), required=False, default=1e-3, help="nodes whose largest weight (and whose neighbours') stays at or below this are emptied")
@click.option("--dilate", type=click.IntRange(0, 4), required=False, default=1, help="nodes within this many steps of a node above the threshold are kept")
@click.option("--fill_density", type=click.FLOAT, required=False, default=None, help="raw density of an emptied node (default 0; required for softplus fields, e.g. -10)")
@click.option("--num_samples_per_ray", type=click.INT, required=False, default=None, help="samples per ray of the statistic (default: the model's training value)")
@click.option("-d", "--data_path", type=click.Path(), required=False, default=None, help=".npz with images, poses, focal, near, far (as for training)")
@click.option("--data_downsample_factor", type=click.FloatRange(min=1.0), required=False, default=1.0, help="downscale factor for the input images")
@click.option("--synthetic", type=click.BOOL, required=False, default=False, help="the procedural scene of the training script")
@click.option("--synthetic_size", type=click.INT, required=False, default=200, help="image size of the synthetic scene")
@click.option("--train_num_samples_per_ray", type=click.INT, required=False, default=512, help="(as for training: sample count of the synthetic scene's images)")
# fmt: on
def main(**config) -> None:
    dev = torch.device("cuda", 0)
    model, extra = rf.create_volumetric_model_from_saved_model(Path(config["model_path"]), rf.create_voxel_grid_from_saved_info_dict, device=dev)
    train, _ = load_datasets(config, dev)
    grid = model.thre3d_repr
    samples = config["num_samples_per_ray"] or model.render_config.num_samples_per_ray
    before = occupied_cells(grid)
    weights = rf.node_max_weights(model, train.poses, train.camera_intrinsics, train.camera_bounds, samples, render_config=model.render_config)
    stats = rf.prune_voxel_grid(grid, weights, config["threshold"], config["dilate"], config["fill_density"])
    after = occupied_cells(grid)
    print(f"views: {len(train)}  samples per ray: {samples}  threshold: {config['threshold']}  dilate: {config['dilate']}")
    print(f"kept nodes: {stats.kept}  pruned nodes: {stats.pruned}")
    print(f"occupied cells: {before} -> {after}")
    torch.save(model.get_save_info(extra_info=extra), config["output_path"])


if __name__ == "__main__":
    main()
