"""Camera pose refinement against a trained ReLU field (registration of a photograph to the field, iNeRF-style).

The field is frozen: only the pose moves.  The pose is parametrised as a perturbation of an initial pose,
R = so3_exp(omega) R0 and t = t0 + tau (camera.perturb_pose), and (omega, tau) are fitted with Adam on the reference's L1
colour loss.  Every step goes cast_rays (HIP kernel, differentiable in R and t) -> render_rays (the fused HIP render,
differentiable in the rays through rf_render_backward_rays) -> L1 (optionally mixed with D-SSIM), so no grid gradient is ever computed.
"""
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from .camera import CameraIntrinsics, CameraPose, perturb_pose
from .render_interface import Rays, flatten_rays
from .volumetric_model import VolumetricModel, cast_rays


def refine_camera_pose(
    vol_mod: VolumetricModel,
    image: Tensor,
    camera_intrinsics: CameraIntrinsics,
    initial_pose: CameraPose,
    num_iterations: int = 200,
    learning_rate: float = 3e-3,
    rays_per_iteration: Optional[int] = None,
    seed: int = 0,
    final_learning_rate_fraction: float = 0.01,
    dssim_weight: float = 0.0,
    **render_kwargs,
) -> Tuple[CameraPose, List[Dict[str, Any]]]:
    """Fit the pose of ``image`` [H, W, 3] (values in [0, 1]) starting from ``initial_pose``.

    The learning rate decays exponentially to ``final_learning_rate_fraction`` of ``learning_rate`` over the iterations (the L1
    loss's gradient does not shrink near the optimum, so a constant rate would leave the pose jittering at the step size).
    ``rays_per_iteration``: None renders every pixel per iteration; a number draws that many pixels per iteration, a keyed random
    subset (seeded by ``seed`` and the iteration, reproducible).  ``dssim_weight`` = lambda in (0, 1]: the loss becomes
    (1 - lambda) L1 + lambda (1 - SSIM) of the full frame, SSIM with the zero-padded "same" windows (the D-SSIM term of 3DGS, against
    L1's flat basin; metrics.ssim); it needs the image, so it cannot be combined with ``rays_per_iteration`` below the frame.  0 is
    the plain L1 path.  ``render_kwargs`` override render-config fields for the renders
    (the volumetric model's own configuration is used otherwise).  Returns the refined pose (float32 tensors on the model's device,
    t of shape [3, 1]) and the history: one dict per iteration with ``loss`` (of the pose before the step), ``rotation`` and
    ``translation`` (numpy, after the step)."""
    device = vol_mod.device
    H, W, _ = camera_intrinsics
    target = torch.as_tensor(image).to(device, torch.float32).reshape(-1, 3)
    if target.shape[0] != int(H) * int(W):
        raise ValueError(f"image must be [{H}, {W}, 3], got {tuple(torch.as_tensor(image).shape)}")
    dssim_weight = float(dssim_weight)
    if not 0.0 <= dssim_weight <= 1.0:
        raise ValueError(f"dssim_weight must lie in [0, 1], got {dssim_weight}")
    if dssim_weight > 0.0 and rays_per_iteration is not None and int(rays_per_iteration) < target.shape[0]:
        raise ValueError("dssim_weight > 0 needs the whole frame per iteration (SSIM is a function of the image): leave rays_per_iteration at None")
    pose0 = CameraPose(torch.as_tensor(initial_pose.rotation).to(device, torch.float32).reshape(3, 3),
                       torch.as_tensor(initial_pose.translation).to(device, torch.float32).reshape(3, 1))
    omega = torch.zeros(3, dtype=torch.float32, device=device, requires_grad=True)
    tau = torch.zeros(3, dtype=torch.float32, device=device, requires_grad=True)
    optimizer = torch.optim.Adam([omega, tau], lr=learning_rate)
    gamma = float(final_learning_rate_fraction) ** (1.0 / max(int(num_iterations), 1))
    schedule = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=gamma)
    params = list(vol_mod.thre3d_repr.parameters())
    was_trainable = [p.requires_grad for p in params]
    history: List[Dict[str, Any]] = []
    try:
        for p in params:  # a frozen field: the renders compute no grid gradient
            p.requires_grad_(False)
        for it in range(int(num_iterations)):
            pose = perturb_pose(pose0, omega, tau)
            rays = flatten_rays(cast_rays(camera_intrinsics, pose, device))
            tgt = target
            if rays_per_iteration is not None and int(rays_per_iteration) < target.shape[0]:
                gen = torch.Generator().manual_seed(int(seed) * 1000003 + it)
                sel = torch.randperm(target.shape[0], generator=gen)[: int(rays_per_iteration)].to(device)
                rays = Rays(rays.origins[sel], rays.directions[sel])
                tgt = target[sel]
            out = vol_mod.render_rays(rays, **render_kwargs)
            loss = torch.nn.functional.l1_loss(out.colour, tgt)
            if dssim_weight > 0.0:
                from .metrics import ssim

                frame = out.colour.reshape(int(H), int(W), 3)
                loss = (1.0 - dssim_weight) * loss + dssim_weight * (1.0 - ssim(frame, tgt.reshape(int(H), int(W), 3), padding="same"))
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            optimizer.step()
            schedule.step()
            with torch.no_grad():
                now = perturb_pose(pose0, omega, tau)
            history.append({"loss": float(loss.item()), "rotation": now.rotation.detach().cpu().numpy(),
                            "translation": now.translation.detach().cpu().numpy()})
    finally:
        for p, t in zip(params, was_trainable):
            p.requires_grad_(t)
    with torch.no_grad():
        final = perturb_pose(pose0, omega, tau)
    return CameraPose(final.rotation.detach(), final.translation.detach()), history


def pose_error(pose: CameraPose, reference: CameraPose) -> Tuple[float, float]:
    """(rotation error in degrees, translation error in world units) of ``pose`` against ``reference``."""
    R = torch.as_tensor(pose.rotation).detach().to("cpu", torch.float64).reshape(3, 3)
    R0 = torch.as_tensor(reference.rotation).detach().to("cpu", torch.float64).reshape(3, 3)
    cos = ((R.T @ R0).trace() - 1.0) / 2.0
    angle = float(torch.rad2deg(torch.arccos(cos.clamp(-1.0, 1.0))))
    t = torch.as_tensor(pose.translation).detach().to("cpu", torch.float64).reshape(3)
    t0 = torch.as_tensor(reference.translation).detach().to("cpu", torch.float64).reshape(3)
    return angle, float((t - t0).norm())
