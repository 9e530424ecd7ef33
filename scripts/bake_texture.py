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
"""
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
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("--mesh", "mesh_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="the .ply mesh to texture")
@click.option("-o", "--output_stem", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path stem of the .obj / .mtl / .png files to write")
@click.option("--patch", type=click.IntRange(min=2, max=64), default=8, required=False, help="texel centres per leg of a triangle's patch")
@click.option("--reach_voxels", type=click.FloatRange(min=0.0), default=2.0, required=False, help="half length of a texel's ray, in (largest) voxel edges")
@click.option("--samples", type=click.IntRange(min=1, max=256), default=16, required=False, help="samples per texel")
@click.option("--diffuse", is_flag=True, default=False, help="bake the degree-0 colour only")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    dev = torch.device("cuda:0")
    creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
    model, _ = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
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
    rf.write_obj(mesh, bake, config["output_stem"])
    print(f"V = {len(mesh.vertices)}, T = {len(mesh.faces)}: atlas {bake.cols * bake.block} x {bake.rows * bake.block} (patch {bake.patch}, {bake.cols} x {bake.rows} blocks), "
          f"reach {reach:.6g}, {config['samples']} samples, {'diffuse' if config['diffuse'] else 'specular'} in {1e3 * dt:.1f} ms (incl. host synchronisation) "
          f"-> {config['output_stem']}.obj / .mtl / .png")


if __name__ == "__main__":
    main()
