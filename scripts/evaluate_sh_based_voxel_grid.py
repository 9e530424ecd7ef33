#!/usr/bin/env python
"""Evaluate a trained ReLU field on the held-out views: PSNR and SSIM (LPIPS needs network weights and is out of scope).

    python scripts/evaluate_sh_based_voxel_grid.py -i out/saved_models/model_final.pth --synthetic True -o metrics.json
    python scripts/evaluate_sh_based_voxel_grid.py -i model.pth -d scene.npz -o metrics.json

The data options are those of scripts/train_sh_based_voxel_grid.py (the same views are held out).  Prints one JSON line with the mean
PSNR and SSIM and writes them with the per-image table to the output file."""
import json
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd.trainers import evaluate_sh_vox_grid_vol_mod_with_posed_images  # noqa: E402
from train_sh_based_voxel_grid import load_datasets  # noqa: E402


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(exists=True, dir_okay=False), required=True, help="checkpoint written by the training script")
@click.option("-o", "--output_path", type=click.Path(dir_okay=False), required=True, help="where the metrics (JSON: means and the per-image table) go")
@click.option("-d", "--data_path", type=click.Path(), required=False, default=None, help=".npz with images, poses, focal, near, far (as for training)")
@click.option("--data_downsample_factor", type=click.FloatRange(min=1.0), required=False, default=1.0, help="downscale factor for the input images")
@click.option("--synthetic", type=click.BOOL, required=False, default=False, help="the procedural scene of the training script")
@click.option("--synthetic_size", type=click.INT, required=False, default=200, help="image size of the synthetic scene")
@click.option("--train_num_samples_per_ray", type=click.INT, required=False, default=512, help="(as for training: sample count of the synthetic scene's images)")
@click.option("--parallel_rays_chunk_size", type=click.INT, required=False, default=32768, help="number of parallel rays processed on the GPU")
# fmt: on
def main(**config) -> None:
    dev = torch.device("cuda", 0)
    model, _ = rf.create_volumetric_model_from_saved_model(Path(config["model_path"]), rf.create_voxel_grid_from_saved_info_dict, device=dev)
    _, test = load_datasets(config, dev)
    scores = evaluate_sh_vox_grid_vol_mod_with_posed_images(model, test, config["parallel_rays_chunk_size"])
    print(json.dumps({"psnr": scores["psnr"], "ssim": scores["ssim"], "num_images": len(scores["per_image"])}))
    out = Path(config["output_path"])
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as fh:
        json.dump(scores, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
