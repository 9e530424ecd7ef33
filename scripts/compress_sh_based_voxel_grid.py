#!/usr/bin/env python
"""Compress a trained ReLU field into a compact checkpoint (VQRF-style): render the training views, record per grid node the largest
compositing weight any ray gave it, drop the nodes that carry the least of that importance, keep the ones that carry most of it
verbatim and vector-quantise the feature vectors of the rest against a small codebook (importance-weighted k-means on the GPU).

    python scripts/compress_sh_based_voxel_grid.py -i out/saved_models/model_final.pth -o model_vq.pth --synthetic True
    python scripts/compress_sh_based_voxel_grid.py -i model.pth -o model_vq.pth -d scene.npz --num_codes 4096 --keep_share 0.6

The data options are those of scripts/train_sh_based_voxel_grid.py (the same views are held out).  The written file loads wherever a
plain checkpoint does (render, evaluate, extract_mesh, prune, crop, refine pose, export point cloud: ``-i model_vq.pth``).  Prints the
node counts per class, the weighted distortion of every k-means assignment and both file sizes."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thr3ed_atom_amd as rf  # noqa: E402
from train_sh_based_voxel_grid import load_datasets  # noqa: E402


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(exists=True, dir_okay=False), required=True, help="checkpoint written by the training script")
@click.option("-o", "--output_path", type=click.Path(dir_okay=False), required=True, help="where the compact checkpoint goes")
@click.option("--prune_share", type=click.FloatRange(0.0, 1.0), required=False, default=0.001, help="share of the total importance whose least important nodes are dropped")
@click.option("--keep_share", type=click.FloatRange(0.0, 1.0), required=False, default=0.6, help="share of the total importance whose most important nodes are kept verbatim")
@click.option("--num_codes", type=click.IntRange(1, 65536), required=False, default=4096, help="size of the codebook")
@click.option("--iterations", type=click.IntRange(min=0), required=False, default=10, help="k-means iterations")
@click.option("--value_dtype", type=click.Choice(["float16", "float32"]), required=False, default="float16", help="stored precision of densities, kept features and codebook")
@click.option("--fill_density", type=click.FLOAT, required=False, default=None, help="raw density of a dropped node (default 0; required for softplus fields, e.g. -10)")
@click.option("--seed", type=click.INT, required=False, default=0, help="seed of the codebook's initialisation")
@click.option("--num_samples_per_ray", type=click.INT, required=False, default=None, help="samples per ray of the importance statistic (default: the model's training value)")
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
    samples = config["num_samples_per_ray"] or model.render_config.num_samples_per_ray
    importance = rf.node_max_weights(model, train.poses, train.camera_intrinsics, train.camera_bounds, samples, render_config=model.render_config)
    field = rf.compress_voxel_grid(model, importance, prune_share=config["prune_share"], keep_share=config["keep_share"], num_codes=config["num_codes"],
                                   iterations=config["iterations"], value_dtype=config["value_dtype"], fill_density=config["fill_density"], seed=config["seed"])
    torch.save(model.get_save_info(extra_info=extra, compressed=field), config["output_path"])
    stats = field.stats
    print(f"views: {len(train)}  samples per ray: {samples}  prune_share: {config['prune_share']}  keep_share: {config['keep_share']}  value_dtype: {config['value_dtype']}")
    print(f"pruned nodes: {stats['pruned']}  kept nodes: {stats['kept']}  quantised nodes: {stats['quantised']}  codes: {stats['num_codes']}")
    print("distortion per assignment: " + " ".join(f"{v:.6e}" for v in stats["distortions"]))
    print(f"file size: {os.path.getsize(config['model_path'])} -> {os.path.getsize(config['output_path'])} bytes (payload {stats['payload_bytes']})")


if __name__ == "__main__":
    main()
