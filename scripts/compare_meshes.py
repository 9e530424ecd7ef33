#!/usr/bin/env python
"""How far two triangle meshes lie from each other (binary PLYs as ``write_ply`` and the scripts of this project write them): Chamfer
distance, Hausdorff distance (a lower bound: the maximum over the samples and the vertices) and the F-score at given thresholds, from
area-weighted surface samples and their closest points on the other mesh (thr3ed_atom_amd.mesh_distance).
--signed adds which way they lie from each other: the signed mean, the share of samples inside the other mesh and both signed volumes
(thr3ed_atom_amd.mesh_sign; the sign is guaranteed for closed oriented meshes only).

    python scripts/compare_meshes.py -a raw.ply -b small.ply --threshold 0.01 --threshold 0.02 -o metrics.json

Precision is the share of a's samples within the threshold of b, recall the share of b's within it of a: pass the reconstruction as
-a and the reference as -b.
"""
import json
import os
import sys

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd.mesh import read_ply  # noqa: E402
from thr3ed_atom_amd.mesh_distance import format_mesh_distance, mesh_distance_dict  # noqa: E402
from thr3ed_atom_amd.mesh_sign import format_signed_mesh_distance, signed_mesh_distance_dict  # noqa: E402


def load(path: str, dev) -> "rf.Mesh":
    vertices, _, _, faces = read_ply(path)
    return rf.Mesh(torch.from_numpy(np.ascontiguousarray(vertices)).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev), None, None)


# fmt: off
@click.command()
@click.option("-a", "--mesh_a", type=click.Path(file_okay=True, dir_okay=False), required=True, help="the first .ply file (precision is measured on its samples)")
@click.option("-b", "--mesh_b", type=click.Path(file_okay=True, dir_okay=False), required=True, help="the second .ply file (recall is measured on its samples)")
@click.option("--samples", type=click.IntRange(min=1), default=1_000_000, required=False, help="surface samples per mesh")
@click.option("--threshold", type=click.FloatRange(min=0.0), multiple=True, required=False, help="a distance at which to report precision, recall and F-score (repeatable)")
@click.option("--seed", type=click.INT, default=0, required=False, help="seed of the surface samples")
@click.option("--signed", is_flag=True, default=False, help="add the signed distances (negative: inside the other mesh) and the signed volumes (rf.signed_mesh_distance)")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), default=None, required=False, help="write the metrics as JSON here")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    dev = torch.device("cuda:0")
    a, b = load(config["mesh_a"], dev), load(config["mesh_b"], dev)
    result = rf.mesh_distance(a, b, samples=config["samples"], thresholds=config["threshold"], seed=config["seed"])
    print(f"a: {config['mesh_a']} (V = {len(a.vertices)}, T = {len(a.faces)})\nb: {config['mesh_b']} (V = {len(b.vertices)}, T = {len(b.faces)})")
    print(format_mesh_distance(result))
    signed = rf.signed_mesh_distance(a, b, samples=config["samples"], seed=config["seed"]) if config["signed"] else None
    if signed is not None:
        print(format_signed_mesh_distance(signed))
    if config["output_path"]:
        os.makedirs(os.path.dirname(os.path.abspath(config["output_path"])), exist_ok=True)
        with open(config["output_path"], "w") as out:
            json.dump({"mesh_a": config["mesh_a"], "mesh_b": config["mesh_b"], "seed": config["seed"], **mesh_distance_dict(result),
                       **({"signed": signed_mesh_distance_dict(signed)} if signed is not None else {})}, out, indent=1)
        print(f"-> {config['output_path']}")


if __name__ == "__main__":
    main()
