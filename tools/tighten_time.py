"""Time rf_node_bounds and rf_resample_grid, and A/B the progressive schedule with and without box tightening.

    python tools/tighten_time.py [--grids 128 256] [--degree 2] [--skip_ab] [--out profiles/tighten_time.json]

Kernels (HIP events, median of 20 runs): at grid^3 / SH degree on all three storages, a blob field that fills 40 % of each axis,
  * rf_node_bounds (threshold 0) -- reads one density per node;
  * rf_resample_grid grid^3 -> grid^3 with the map of a tightening to the blob's box (scale 0.4): writes the whole destination;
  * rf_resample_grid as an exact crop to the blob's box.
A/B (--ab_grid / --ab_stages / --ab_iterations / --ab_size): the synthetic scene of scripts/train_sh_based_voxel_grid.py trained by
the trainer function without and with tighten_threshold=0 (same seed): held-out PSNR, final dims and box, wall time of the call.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def median_ms(fn, repeats=20, warmup=3):
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


def blob_grid(dev, G, F, storage):
    """positive density inside the middle 40 % of each axis, negative outside"""
    import torch

    import thr3ed_atom_amd as rf

    torch.manual_seed(0)
    ax = ((torch.arange(G, device=dev, dtype=torch.float32) + 0.5) / G * 2.0 - 1.0).abs()
    r = torch.maximum(torch.maximum(ax[:, None, None], ax[None, :, None]), ax[None, None, :])
    dens = (0.4 - r)[..., None].contiguous()
    feat = torch.empty((G, G, G, F), device=dev).uniform_(-1, 1)
    return rf.VoxelGrid(dens, feat, rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False, storage=storage)


def time_kernels(dev, G, degree):
    import torch

    import thr3ed_atom_amd as rf
    from thr3ed_atom_amd import ops

    F = 3 * (degree + 1) ** 2
    out = {}
    for storage in ("reference", "split", "bricked"):
        grid = blob_grid(dev, G, F, storage)
        lo, hi, count = rf.content_bounds(grid, 0.0)
        bounds = torch.tensor([G, G, G, -1, -1, -1], dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        r = {"content": [list(lo), list(hi), count], "node_bounds": median_ms(lambda: ops.node_bounds_raw(grid, 0.0, bounds, cnt))}
        dst = rf.VoxelGrid(torch.empty((G, G, G, 1), device=dev), torch.empty((G, G, G, F), device=dev), rf.VoxelSize(1.0, 1.0, 1.0),
                           density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), storage=storage)
        n = hi[0] - lo[0] + 1
        scale = n / G
        offset = lo[0] + 0.5 * scale - 0.5
        r["resample_full"] = median_ms(lambda: ops.resample_grid_raw(grid, dst, (scale,) * 3, (offset,) * 3, 0.0))
        r["resample_full"]["bytes_written"] = G**3 * (F + 1) * 4
        del dst
        crop = rf.VoxelGrid(torch.empty((n, n, n, 1), device=dev), torch.empty((n, n, n, F), device=dev), rf.VoxelSize(1.0, 1.0, 1.0),
                            density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), storage=storage)
        r["resample_crop"] = median_ms(lambda: ops.resample_grid_raw(grid, crop, (1.0,) * 3, (float(lo[0]),) * 3, 0.0))
        r["resample_crop"]["dims"] = [n, n, n]
        out[storage] = r
        del grid, crop
        torch.cuda.empty_cache()
    return out


def train_ab(dev, a):
    import torch

    import thr3ed_atom_amd as rf
    from train_sh_based_voxel_grid import load_datasets
    from thr3ed_atom_amd.trainers import train_sh_vox_grid_vol_mod_with_posed_images

    config = {"synthetic": True, "data_path": None, "synthetic_size": a.ab_size, "train_num_samples_per_ray": a.ab_samples, "data_downsample_factor": 1.0}
    train, test = load_datasets(config, dev)
    G, F = a.ab_grid, 3 * (a.degree + 1) ** 2
    res = {"grid": G, "stages": a.ab_stages, "iterations_per_stage": a.ab_iterations, "image_size": a.ab_size, "samples_per_ray": a.ab_samples, "legs": {}}
    for leg, threshold in (("plain", None), ("tighten", 0.0)):
        torch.manual_seed(42)
        grid = rf.VoxelGrid(torch.empty((G, G, G, 1), device=dev).uniform_(-1, 1), torch.empty((G, G, G, F), device=dev).uniform_(-1, 1),
                            rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), tunable=True, density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(),
                            expected_density_scale=rf.compute_expected_density_scale_for_relu_field_grid((3.0, 3.0, 3.0)))
        cfg = rf.SHVoxGridRenderConfig(a.ab_samples, train.camera_bounds, white_bkgd=True, render_num_samples_per_ray=a.ab_samples)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)
        history = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = train_sh_vox_grid_vol_mod_with_posed_images(model, train, None, test_dataset=test, ray_batch_size=a.ab_rays, num_stages=a.ab_stages,
                                                            num_iterations_per_stage=a.ab_iterations, test_freq=10**9, summary_freq=10**9, save_freq=10**9,
                                                            log=lambda s: None, history=history, tighten_threshold=threshold)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        g = model.thre3d_repr
        res["legs"][leg] = {"test_psnr_per_stage": [h["test_psnr"] for h in history if "test_psnr" in h], "final_dims": list(g.grid_dims),
                            "final_aabb": [list(r) for r in g.aabb], "voxel_size": list(g.voxel_size), "wall_seconds": wall,
                            "tighten_rows": [{k: (list(v) if isinstance(v, tuple) else v) for k, v in h.items() if k in ("stage", "old_dims", "new_dims", "passing_nodes")}
                                             for h in history if "new_dims" in h]}
        del model, grid
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--skip_ab", action="store_true")
    ap.add_argument("--skip_kernels", action="store_true")
    ap.add_argument("--ab_grid", type=int, default=128)
    ap.add_argument("--ab_stages", type=int, default=4)
    ap.add_argument("--ab_iterations", type=int, default=500)
    ap.add_argument("--ab_size", type=int, default=200)
    ap.add_argument("--ab_samples", type=int, default=256)
    ap.add_argument("--ab_rays", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/tighten_time.py needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "sh_degree": a.degree}
    if not a.skip_kernels:
        res["kernels"] = {str(G): time_kernels(dev, G, a.degree) for G in a.grids}
    if not a.skip_ab:
        res["ab"] = train_ab(dev, a)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
