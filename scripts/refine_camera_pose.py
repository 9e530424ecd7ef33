#!/usr/bin/env python
"""Refine the camera pose of an image against a trained model (the field is frozen; only the pose moves).
Checkpoints written by this build OR by the reference load (create_volumetric_model_from_saved_model maps the reference's pickled
names).  The initial pose is a pose_spherical(yaw, pitch, radius) or a [3, 4] camera-to-world matrix (.npy); the image is a PNG
(PIL) or an [H, W, 3] .npy in [0, 1], at the model's camera intrinsics or at --focal.

    python scripts/refine_camera_pose.py -i out/saved_models/model_final.pth --image photo.png --yaw 30 --pitch -30 -o refined
"""
import json
import os
import sys

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402


def _load_image(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        img = np.load(path).astype(np.float32)
        return img if img.max() <= 1.0 else img / 255.0
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) / 255.0


# fmt: off
@click.command()
# Required arguments:
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("--image", "image_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="image whose pose is refined (PNG or .npy [H, W, 3])")
@click.option("-o", "--output_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="directory for the refined pose and the final render")
# initial pose: spherical, or a [3, 4] matrix
@click.option("--yaw", type=click.FLOAT, default=0.0, required=False, help="initial pose: yaw (degrees) of pose_spherical")
@click.option("--pitch", type=click.FLOAT, default=-30.0, required=False, help="initial pose: pitch (degrees) of pose_spherical")
@click.option("--radius", type=click.FLOAT, default=None, required=False, help="initial pose: radius of pose_spherical (default: the model's hemispherical radius)")
@click.option("--pose", "pose_path", type=click.Path(file_okay=True, dir_okay=False), default=None, required=False, help="initial pose as a [3, 4] camera-to-world .npy (overrides yaw / pitch / radius)")
@click.option("--focal", type=click.FLOAT, default=None, required=False, help="focal length in pixels (default: the model's, scaled to the image width)")
# optimisation
@click.option("--num_iterations", type=click.IntRange(min=1), default=200, required=False, help="Adam iterations")
@click.option("--learning_rate", type=click.FLOAT, default=3e-3, required=False, help="Adam learning rate of the pose perturbation")
@click.option("--rays_per_iteration", type=click.IntRange(min=1), default=None, required=False, help="random pixels per iteration (default: all)")
@click.option("--num_samples_per_ray", type=click.IntRange(min=1), default=None, required=False, help="overridden num_samples_per_ray")
@click.option("--seed", type=click.INT, default=0, required=False, help="seed of the pixel subsets")
@click.option("--dssim_weight", type=click.FloatRange(0.0, 1.0), default=0.0, required=False, help="lambda of (1 - lambda) L1 + lambda (1 - SSIM) on the full frame (0: plain L1; needs all rays per iteration)")
# fmt: on
def main(**kwargs) -> None:
    config = dict(kwargs)
    dev = torch.device("cuda:0")
    creator = lambda info: rf.create_voxel_grid_from_saved_info_dict(info, storage="split")  # noqa: E731
    model, extra = rf.create_volumetric_model_from_saved_model(config["model_path"], creator, device=dev)
    image = _load_image(config["image_path"])
    H, W = image.shape[:2]
    intr = extra.get("camera_intrinsics") if isinstance(extra, dict) else None
    focal = config["focal"] if config["focal"] is not None else (float(intr.focal) * W / float(intr.width) if intr is not None else 1.2 * W)
    intrinsics = rf.CameraIntrinsics(H, W, focal)
    if config["pose_path"] is not None:
        m = np.load(config["pose_path"]).astype(np.float32).reshape(3, 4)
        pose0 = rf.CameraPose(torch.from_numpy(m[:, :3].copy()), torch.from_numpy(m[:, 3:].copy()))
    else:
        radius = config["radius"] if config["radius"] is not None else float(extra.get("hemispherical_radius", 4.0311))
        pose0 = rf.pose_spherical(config["yaw"], config["pitch"], radius)
    render_kwargs = {"perturb_sampled_points": False}
    if config["num_samples_per_ray"] is not None:
        render_kwargs["num_samples_per_ray"] = config["num_samples_per_ray"]
    pose, history = rf.refine_camera_pose(model, torch.from_numpy(image), intrinsics, pose0, num_iterations=config["num_iterations"],
                                          learning_rate=config["learning_rate"], rays_per_iteration=config["rays_per_iteration"],
                                          seed=config["seed"], dssim_weight=config["dssim_weight"], **render_kwargs)
    os.makedirs(config["output_path"], exist_ok=True)
    c2w = np.concatenate([pose.rotation.cpu().numpy(), pose.translation.cpu().numpy()], axis=1).astype(np.float32)
    np.save(os.path.join(config["output_path"], "refined_pose.npy"), c2w)
    with open(os.path.join(config["output_path"], "refined_pose.json"), "w") as fh:
        json.dump({"camera_to_world": c2w.tolist(), "initial_loss": history[0]["loss"], "final_loss": history[-1]["loss"],
                   "num_iterations": len(history), "height": H, "width": W, "focal": focal}, fh, indent=1)
    with torch.no_grad():
        out = model.render(pose, intrinsics, **render_kwargs)
    frame = (out.colour.clamp(0, 1) * 255).byte().cpu().numpy()
    try:
        from PIL import Image

        Image.fromarray(frame).save(os.path.join(config["output_path"], "refined_render.png"))
    except ImportError:
        np.save(os.path.join(config["output_path"], "refined_render.npy"), frame)
    label = "L1" if config["dssim_weight"] == 0.0 else "(1 - w) L1 + w (1 - SSIM)"
    print(f"{label} {history[0]['loss']:.5f} -> {history[-1]['loss']:.5f} after {len(history)} iterations; pose written to {config['output_path']}")


if __name__ == "__main__":
    main()
