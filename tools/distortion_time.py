"""Time rf_distortion and a training step with the distortion term (HIP events, median of 20 runs each).

    python tools/distortion_time.py [--grid 128] [--degree 2] [--rays 16384] [--samples 256] [--out profiles/distortion_time.json]

At grid^3 / SH degree / split storage, rays x samples, for a U(-1,1) grid (the first training steps) and a sparse blob (a trained
field), on rays of a camera circle:
  * rf_distortion loss-only against rf_node_max_weight on the same batch (the same walk, no second pass) -- the yardstick;
  * rf_distortion with the gradient (both passes and the atomic scatter);
  * the bench-sized TrainStepper(fuse_optimizer=False) step without the term, with it, and without it again: the without-legs are
    the code path of a stepper built without the argument (weight 0 changes nothing), and two of them bracket the drift of the box.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, before=None, repeats=20, warmup=3):
    import torch

    times = []
    for i in range(warmup + repeats):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}


def make_grid(dev, G, F, scene, tunable=False):
    import torch

    import thr3ed_atom_amd as rf

    torch.manual_seed(0)
    if scene == "uniform":
        dens = torch.empty((G, G, G, 1), device=dev).uniform_(-1, 1)
    else:  # a blob of radius ~0.75 in the [-1.5, 1.5]^3 world, negative outside
        ax = ((torch.arange(G, device=dev, dtype=torch.float32) + 0.5) / G * 3.0 - 1.5) / 1.5
        r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
        dens = (3.0 * (0.5 - r))[..., None].contiguous()
    feat = torch.empty((G, G, G, F), device=dev).uniform_(-1, 1)
    return rf.VoxelGrid(dens, feat, rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=tunable, storage="split")


def batch_rays(dev, n):
    """n rays: a square crop of a frame's pixel rays from a pose on the usual camera circle"""
    import thr3ed_atom_amd as rf

    side = int(round(n**0.5))
    assert side * side == n, "--rays must be a square number"
    flat = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(side, side, side * 1.39), rf.pose_spherical(40.0, -30.0, 4.0311), dev))
    return flat.origins.contiguous(), flat.directions.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--weight", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import thr3ed_atom_amd as rf
    from thr3ed_atom_amd import ops
    from thr3ed_atom_amd.trainers import TrainStepper

    if not torch.cuda.is_available():
        raise SystemExit("tools/distortion_time.py needs a GPU")
    dev = torch.device("cuda:0")
    G, F, S, n = a.grid, 3 * (a.degree + 1) ** 2, a.samples, a.rays
    near, far = 1.8, 6.6
    o, d = batch_rays(dev, n)
    res = {"grid": G, "sh_degree": a.degree, "rays": n, "samples_per_ray": S, "storage": "split", "device": torch.cuda.get_device_name(0), "scenes": {}}
    for scene in ("uniform", "blob"):
        grid = make_grid(dev, G, F, scene)
        first, _ = grid.kernel_tensors()
        batch = ops.RayBatch(o, d, S, near, far, t_rand=ops.KeyedJitter(1234, 0))
        M = torch.zeros((G, G, G), device=dev)
        loss = torch.empty(n, device=dev)
        grad = torch.zeros_like(first)
        r = {
            "node_max_weight_same_batch": median_ms(lambda: ops.node_max_weight_raw(grid, batch, 0, M), before=M.zero_),
            "distortion_loss_only": median_ms(lambda: ops.distortion_raw(grid, batch, 0, 0.0, None, loss, None)),
            "distortion_with_gradient": median_ms(lambda: ops.distortion_raw(grid, batch, 0, 1.0 / n, None, loss, grad)),
        }
        r["mean_loss"] = float(loss.mean())
        del grid, M, grad
        # the training step, bench-sized: fused, binned, both renders, the gradient bucket kept
        pixels = torch.rand((n, 3), device=dev)
        rays = rf.Rays(o, d)
        cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=True, white_bkgd=True)
        for leg, weight in (("step_without_a", 0.0), ("step_with", a.weight), ("step_without_b", 0.0)):
            tgrid = make_grid(dev, G, F, scene, tunable=True)
            model = rf.VolumetricModel(tgrid, rf.render_sh_voxel_grid, cfg, device=dev)
            stepper = TrainStepper(model, n, learning_rate=0.03, data_parallel=False, fuse_optimizer=False, distortion_weight=weight)
            r[leg] = median_ms(lambda: stepper.step_on(rays, pixels))
            stepper.flat.detach()
            del stepper, model, tgrid
        res["scenes"][scene] = r
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
