#!/usr/bin/env python
"""Remove the floaters of a trained ReLU field: label the connected components of the nodes whose own activated density exceeds a
threshold and empty every component that is too small or ranks too low (thr3ed_atom_amd.components).  Unlike visibility pruning this
needs no views and also removes a floater the cameras did see.

    python scripts/clean_sh_based_voxel_grid.py -i out/saved_models/model_final.pth -o cleaned.pth --threshold 0 --keep_largest 1
    python scripts/clean_sh_based_voxel_grid.py -i model.pth -o cleaned.pth --threshold 0.5 --min_nodes 64 --connectivity 26

Prints the component table (largest first) before and after."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402

TABLE_ROWS = 10


def print_components(title: str, grid, found) -> None:
    roots, sizes = found.roots.tolist(), found.sizes.tolist()
    _, Y, Z = (int(v) for v in grid.grid_dims)
    print(f"{title}: {len(roots)} components, {sum(sizes)} occupied nodes")
    for rank, (root, size) in enumerate(zip(roots[:TABLE_ROWS], sizes[:TABLE_ROWS])):
        print(f"  #{rank}: {size} nodes, first node ({root // (Y * Z)}, {root // Z % Y}, {root % Z})")
    if len(roots) > TABLE_ROWS:
        print(f"  ... and {len(roots) - TABLE_ROWS} smaller ones ({sum(sizes[TABLE_ROWS:])} nodes)")


# fmt: off
@click.command()
@click.option("-i", "--model_path", type=click.Path(exists=True, dir_okay=False), required=True, help="checkpoint written by the training script")
@click.option("-o", "--output_path", type=click.Path(dir_okay=False), required=True, help="where the cleaned checkpoint goes")
@click.option("--threshold", type=click.FloatRange(min=0.0), required=False, default=0.0, help="a node is occupied when its own activated density exceeds this (softplus fields: positive)")
@click.option("--keep_largest", type=click.IntRange(min=1), required=False, default=None, help="keep only this many of the largest components")
@click.option("--min_nodes", type=click.IntRange(min=1), required=False, default=None, help="remove the components with fewer nodes than this")
@click.option("--connectivity", type=click.Choice(["6", "18", "26"]), required=False, default="26", help="neighbours of a node: faces, + edges, + corners")
@click.option("--fill_density", type=click.FLOAT, required=False, default=None, help="raw density of an emptied node (default 0; required for softplus fields, e.g. -10)")
# fmt: on
def main(**config) -> None:
    if config["keep_largest"] is None and config["min_nodes"] is None:
        raise click.UsageError("give --keep_largest, --min_nodes or both")
    dev = torch.device("cuda", 0)
    model, extra = rf.create_volumetric_model_from_saved_model(Path(config["model_path"]), rf.create_voxel_grid_from_saved_info_dict, device=dev)
    grid = model.thre3d_repr
    connectivity = int(config["connectivity"])
    print(f"grid {tuple(grid.grid_dims)}  threshold: {config['threshold']}  connectivity: {connectivity}  keep_largest: {config['keep_largest']}  min_nodes: {config['min_nodes']}")
    print_components("before", grid, rf.label_components(grid, config["threshold"], connectivity))
    stats = rf.remove_small_components(grid, config["threshold"], connectivity, min_nodes=config["min_nodes"], keep_largest=config["keep_largest"],
                                       fill_density=config["fill_density"])
    print(f"removed components: {stats.removed_components} of {stats.components}  removed nodes: {stats.removed_nodes}  kept nodes: {stats.kept_nodes}")
    print_components("after", grid, rf.label_components(grid, config["threshold"], connectivity))
    torch.save(model.get_save_info(extra_info=extra), config["output_path"])


if __name__ == "__main__":
    main()
