"""Time rf_render_geometry beside the per-ray forward render of the same frame (HIP events around windows of back-to-back frames, the
two legs alternating, median over the rounds).

    python tools/geometry_time.py [--frames 10] [--rounds 7] [--hw 800] [--out profiles/geometry_time.json]

Two frames of a sparse blob on split storage at SH degree 0, pose_spherical(30, -30, 4.0311), keyed jitter:
  * 128^3, 256 samples per ray, no mask;
  * 256^3, 512 samples per ray, occupancy mask (the bench's configs[4]).
The yardstick is rf_render_forward's per-ray kernel ($RF_FRAME_TILES=0) at SH degree 0: the same walk and the same 8 base records per
sample, plus the colour.  The geometry pass gathers the same records and no feature, so it should cost no more.  Also printed: that
the pass's accumulated weight is the forward's, bit for bit, on that frame.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(fn, frames):
    """ms per call of ``frames`` calls enqueued back to back between two events"""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(frames):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / frames


def make_grid(dev, G):
    """a blob of radius ~0.75 in the [-1.5, 1.5]^3 world, negative outside, with a little noise; F = 3, split storage"""
    import torch

    import thr3ed_atom_amd as rf

    torch.manual_seed(0)
    ax = ((torch.arange(G, device=dev, dtype=torch.float32) + 0.5) / G * 3.0 - 1.5) / 1.5
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    dens = (0.5 - r + 0.05 * torch.empty((G, G, G), device=dev).uniform_(-1, 1))[..., None].contiguous()
    feat = torch.empty((G, G, G, 3), device=dev).uniform_(-1, 1)
    return rf.VoxelGrid(dens, feat, rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=False, storage="split")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10, help="frames per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="windows per leg, the legs alternating")
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import thr3ed_atom_amd as rf
    from thr3ed_atom_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("tools/geometry_time.py needs a GPU")
    keep_env = os.environ.get("RF_FRAME_TILES")
    os.environ["RF_FRAME_TILES"] = "0"  # the yardstick is the per-ray forward kernel (restored below)
    dev = torch.device("cuda:0")
    H = W = a.hw
    focal = 1111.111 * a.hw / 800.0
    near, far = 1.8, 6.6
    pose = rf.pose_spherical(30.0, -30.0, 4.0311)
    n = H * W
    res = {"frame": f"{H}x{W}", "storage": "split", "sh_degree": 0, "frames_per_window": a.frames, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, G, S, mask in (("128^3, 256 samples", 128, 256, False), ("256^3, 512 samples, occupancy mask (configs[4])", 256, 512, True)):
        grid = make_grid(dev, G)
        if mask:
            grid.build_occupancy()
        flags = ops.render_flags(True, False, False, mask)
        jitter = ops.KeyedJitter(1234, 0)
        batch = ops.RayBatch(None, None, S, near, far, t_rand=jitter, camera=(H, W, focal, pose.rotation, pose.translation))
        normal, depth, acc = torch.empty((n, 3), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
        geometry = lambda: ops.render_geometry_raw(grid, batch, flags, 0.5, normal, depth, acc)  # noqa: E731
        forward = lambda: ops.render_frame_raw(grid, H, W, focal, pose.rotation, pose.translation, S, near, far, flags, jitter)  # noqa: E731
        assert lib_frame_kernel(grid, H, W, focal, pose, flags) == 0, "the yardstick must be the per-ray kernel"
        for fn in (geometry, forward):  # warm-up of both shapes
            window_ms(fn, 2)
        legs = {"geometry": [], "forward_per_ray": []}
        for _ in range(a.rounds):
            legs["geometry"].append(window_ms(geometry, a.frames))
            legs["forward_per_ray"].append(window_ms(forward, a.frames))
        fwd_acc = forward()[2].reshape(-1)
        geometry()
        torch.cuda.synchronize()
        r = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in legs.items()}
        r["ratio_geometry_over_forward"] = r["geometry"]["ms_median"] / r["forward_per_ray"]["ms_median"]
        r["ray_samples_per_s_geometry"] = n * S / (r["geometry"]["ms_median"] * 1e-3)
        r["acc_bit_identical_to_forward"] = bool(torch.equal(acc, fwd_acc))
        r["pixels_with_a_median_depth"] = int((depth != 0).sum())
        res["configs"][name] = r
        del grid, normal, depth, acc
        torch.cuda.empty_cache()
    if keep_env is None:
        del os.environ["RF_FRAME_TILES"]
    else:
        os.environ["RF_FRAME_TILES"] = keep_env
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def lib_frame_kernel(grid, H, W, focal, pose, flags):
    """rf_frame_render_kernel's choice for this frame: 0 = the per-ray kernel"""
    import ctypes as C

    from thr3ed_atom_amd import _lib, ops

    cam = ops._camera_struct(H, W, focal, pose.rotation, pose.translation)
    g = grid.to_rf_grid(use_occupancy=bool(flags & _lib.FLAG_OCCUPANCY_SKIP))
    return _lib.load().rf_frame_render_kernel(C.byref(g), C.byref(cam), flags)


if __name__ == "__main__":
    main()
