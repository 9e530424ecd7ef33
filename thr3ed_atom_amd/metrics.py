"""Image metrics on the GPU.  ``ssim`` is the structural similarity of Wang et al. 2004 as the radiance-field literature reports it
(PSNR / SSIM / LPIPS; LPIPS needs network weights and is out of scope), computed by the HIP kernels of csrc/image_kernels.hip."""
from typing import Tuple, Union

import torch
from torch import Tensor

from . import ops


def ssim(image: Tensor, target: Tensor, *, padding: str = "valid", return_map: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """Mean SSIM of two float32 images [H, W, C] with values of data range 1, per colour channel: Gaussian 11 x 11 window of
    sigma 1.5, C1 = 0.01^2, C2 = 0.03^2, variances NOT clamped (the form of pytorch-msssim and 3DGS, not jaxnerf's clamped one), and
    S = (A1 A2) / (B1 B2) in the association of include/relu_field.h: ``ssim(a, a)`` is exactly 1.

    ``padding="valid"`` (the convention of the NeRF literature's numbers) counts only the windows inside the image: the map is
    [H - 10, W - 10, C] and the image must be at least 11 x 11.  ``padding="same"`` (the D-SSIM convention of 3DGS) zero-pads the
    image by 5: the map is [H, W, C] for any size.  Returns the 0-d mean, and with ``return_map`` also the map (not differentiable).

    The inputs may be views -- a [C, H, W] tensor as ``.permute(1, 2, 0)``, a crop of a larger frame: the kernels address them by
    strides and copy nothing.  Differentiable with respect to ``image`` (one gather launch, bitwise reproducible).  SSIM is
    symmetric, so a ``target`` that requires grad is refused: swap the arguments.  HIP tensors only: there is no CPU fallback."""
    image, target = torch.as_tensor(image), torch.as_tensor(target)
    ops._require_hip(image, "image")
    ops._require_hip(target, "target")
    if target.requires_grad:
        raise ValueError("ssim is differentiable with respect to `image` only; SSIM is symmetric, so pass the tensor that needs the gradient first")
    return ops._SSIM.apply(image, target, padding, bool(return_map))
