"""Time rf_ssim_forward / rf_ssim_backward against the float32 F.conv2d form a user would write today (HIP events after warm-up,
median of 20 runs each, the same random images on the same GPU).

    python tools/ssim_time.py [--out profiles/ssim_time.json]

At 800 x 800 x 3 and 200 x 200 x 3, both paddings:
  * forward alone (no map, no derivative maps), forward with the derivative maps (what a forward under autograd runs), the adjoint
    launch alone, and forward + backward through autograd (rf.ssim(...).backward());
  * the torch form: five grouped F.conv2d of the 11 x 11 window and the pointwise formula, forward alone and forward + backward.
There is no earlier SSIM of this project to compare with.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeats=20, warmup=5):
    import torch

    times = []
    for i in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}


def torch_ssim(x, y, window, padding):
    """mean SSIM of [H, W, C] float32 tensors with grouped F.conv2d: the contract of rf.ssim in plain torch"""
    import torch.nn.functional as F

    C = x.shape[2]
    w = window.expand(C, 1, 11, 11)
    f = lambda v: F.conv2d(v.permute(2, 0, 1)[None], w, padding=5 if padding == "same" else 0, groups=C)  # noqa: E731
    mx, my, xx, yy, xy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    a1, a2 = 2.0 * mx * my + 1e-4, 2.0 * (xy - mx * my) + 9e-4
    b1, b2 = mx * mx + my * my + 1e-4, (xx - mx * mx) + (yy - my * my) + 9e-4
    return ((a1 * a2) / (b1 * b2)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import thr3ed_atom_amd as rf
    from thr3ed_atom_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("tools/ssim_time.py needs a GPU")
    dev = torch.device("cuda:0")
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / 4.5)
    g = g / g.sum()
    window = (g[:, None] * g[None, :]).to(dev, torch.float32)[None, None]
    res = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for size in (800, 200):
        torch.manual_seed(size)
        x, y = torch.rand((size, size, 3), device=dev), torch.rand((size, size, 3), device=dev)
        for padding in ("valid", "same"):
            leaf, tleaf = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            _, _, dmaps = ops.ssim_forward_raw(x, y, padding, False, True)
            one, grad = torch.ones((), device=dev), torch.empty_like(x)

            def hip_both():
                leaf.grad = None
                rf.ssim(leaf, y, padding=padding).backward()

            def torch_both():
                tleaf.grad = None
                torch_ssim(tleaf, y, window, padding).backward()

            r = {
                "hip_forward": median_ms(lambda: ops.ssim_forward_raw(x, y, padding)),
                "hip_forward_with_derivative_maps": median_ms(lambda: ops.ssim_forward_raw(x, y, padding, False, True)),
                "hip_backward_launch": median_ms(lambda: ops.ssim_backward_raw(x, y, padding, dmaps, one, grad)),
                "hip_forward_backward": median_ms(hip_both),
                "torch_forward": median_ms(lambda: torch_ssim(x, y, window, padding)),
                "torch_forward_backward": median_ms(torch_both),
            }
            r["value_hip"], r["value_torch"] = float(rf.ssim(x, y, padding=padding)), float(torch_ssim(x, y, window, padding))
            r["torch_over_hip_forward"] = r["torch_forward"]["ms_median"] / r["hip_forward"]["ms_median"]
            r["torch_over_hip_forward_backward"] = r["torch_forward_backward"]["ms_median"] / r["hip_forward_backward"]["ms_median"]
            res["cases"][f"{size}x{size}x3 {padding}"] = r
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
