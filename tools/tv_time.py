"""Time rf_tv_grad against the streaming yardstick rf_adam_step (HIP events, median of 20 launches each).

    python tools/tv_time.py [--grid 128] [--degree 2] [--storage split] [--steps 30] [--out profiles/tv_time.json]

Reports, at grid^3 / SH degree / storage:
  * rf_tv_grad with and without the sums, as achieved bytes per second over its COMPULSORY traffic of 3 x 4 B per parameter (the
    parameters read once, the gradient read and written);
  * rf_adam_step on the same parameter count (7 x 4 B per parameter: parameter, gradient and two moments read; parameter and two
    moments written);
  * the training step of TrainStepper(fuse_optimizer=False) on the bench-sized problem (32768 rays x 256 samples) without and with TV.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thr3ed_atom_amd as rf  # noqa: E402
from thr3ed_atom_amd import ops  # noqa: E402
from thr3ed_atom_amd.trainers import TrainStepper  # noqa: E402


def median_ms(fn, repeats=20, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def make_grid(dev, G, F, storage):
    dens = torch.empty((G, G, G, 1), device=dev).uniform_(-1, 1)
    feat = torch.empty((G, G, G, F), device=dev).uniform_(-1, 1)
    return rf.VoxelGrid(dens, feat, rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=True, storage=storage)


def step_ms(dev, G, F, storage, steps, tv):
    torch.manual_seed(0)
    grid = make_grid(dev, G, F, storage)
    cfg = rf.SHVoxGridRenderConfig(256, rf.CameraBounds(1.8, 6.6), white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
    stepper = TrainStepper(model, 32768, 0.03, data_parallel=False, fuse_optimizer=False, **({"tv_density_weight": 1e-3, "tv_feature_weight": 1e-4} if tv else {}))
    n = 32768
    o = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1) * 4.0
    d = -o / 4.0 + 0.15 * torch.randn(n, 3, device=dev)
    rays, pixels = rf.Rays(o, d), torch.rand(n, 3, device=dev)
    out = median_ms(lambda: stepper.step_on(rays, pixels), repeats=steps, warmup=5)
    stepper.flat.detach()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--storage", default="split")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tv_time.py needs a GPU")
    dev = torch.device("cuda:0")
    G, F = a.grid, 3 * (a.degree + 1) ** 2
    grid = make_grid(dev, G, F, a.storage)
    first, second = grid.kernel_tensors()
    gf, gs = torch.zeros_like(first), (None if second is None else torch.zeros_like(second))
    sums = torch.zeros(2, device=dev)
    params = G**3 * (F + 1)
    res = {"grid": G, "num_features": F, "storage": a.storage, "parameters": params, "device": torch.cuda.get_device_name(0)}
    for name, s in (("tv_grad", None), ("tv_grad_with_sums", sums)):
        med, lo, hi = median_ms(lambda: ops.tv_grad_raw(grid, 1e-3, 1e-4, gf, gs, s))
        res[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "compulsory_bytes": 12 * params, "achieved_TBps": 12 * params / (med * 1e-3) / 1e12}
    p, g, m, v = (torch.zeros(params, device=dev) for _ in range(4))
    step = [0]

    def adam():
        step[0] += 1
        ops.adam_step_hip(p, g, m, v, 0.03, 0.9, 0.999, 1e-8, step[0])

    med, lo, hi = median_ms(adam)
    res["adam_step"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "bytes": 28 * params, "achieved_TBps": 28 * params / (med * 1e-3) / 1e12}
    del p, g, m, v
    for name, tv in (("train_step_without_tv", False), ("train_step_with_tv", True), ("train_step_without_tv_again", False)):
        med, lo, hi = step_ms(dev, G, F, a.storage, a.steps, tv)
        res[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi}
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
