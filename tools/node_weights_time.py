"""Time rf_node_max_weight and rf_prune_grid (HIP events, median of 20 launches each).

    python tools/node_weights_time.py [--grid 128] [--degree 2] [--samples 256] [--size 800] [--out profiles/node_weights_time.json]

At grid^3 / SH degree / samples per ray / size x size pixels on split storage, for a U(-1,1) grid (the first training steps) and a
sparse blob (a trained field):
  * one rf_node_max_weight view on a zeroed buffer, and the 100th view on a warm buffer (views on a circle; almost every update is
    then rejected by the guard's plain load);
  * one rf_render_forward of the same rays at RF_FLAG_RENDER_DIFFUSE (the per-ray kernel, rays given as a list): the yardstick --
    the same walk plus the colour;
  * the guard off / on and the lane dedupe off / on.  These are compile-time switches of the kernel (RF_NMW_GUARD, RF_NMW_DEDUPE),
    not environment variables of the library: the tool compiles one copy of the library per variant into tools/exp_nmw_g<G>d<D>.so
    (if it is not there yet) and times each in a child process of its own with $RF_LIB_PATH pointing at it;
  * rf_prune_grid at dilate 0 / 1 / 2 against rf_adam_step on as many parameters as the grid has nodes (7 x 4 B each).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = [(1, 0), (0, 0), (1, 1), (0, 1)]  # (guard, dedupe); the first is what the library ships


def variant_path(guard, dedupe):
    return os.path.join(ROOT, "tools", f"exp_nmw_g{guard}d{dedupe}.so")


def build_variants():
    from thr3ed_atom_amd import _lib

    for guard, dedupe in VARIANTS:
        path = variant_path(guard, dedupe)
        srcs = [os.path.join(_lib.CSRC_DIR, s) for s in _lib.SOURCES]
        if os.path.exists(path) and os.path.getmtime(path) >= max(os.path.getmtime(s) for s in srcs):
            continue
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + _lib.HIPCC_FLAGS + [f"-DRF_NMW_GUARD={guard}", f"-DRF_NMW_DEDUPE={dedupe}", "-I", _lib.INCLUDE_DIR] + srcs + ["-o", path]
        print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)


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


def make_grid(dev, G, F, scene):
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
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, storage="split")


def measure(a):
    """the measurements of ONE library (whatever $RF_LIB_PATH names), as a dict"""
    import torch

    import thr3ed_atom_amd as rf
    from thr3ed_atom_amd import _lib, ops

    if not torch.cuda.is_available():
        raise SystemExit("tools/node_weights_time.py needs a GPU")
    dev = torch.device("cuda:0")
    G, F, S, hw = a.grid, 3 * (a.degree + 1) ** 2, a.samples, a.size
    near, far = 1.8, 6.6
    res = {}
    poses = [rf.pose_spherical(360.0 * k / 100, -30.0, 4.0311) for k in range(100)]
    camera = lambda p: (hw, hw, hw * 1.39, p.rotation, p.translation)  # noqa: E731
    for scene in ("uniform", "blob"):
        grid = make_grid(dev, G, F, scene)
        M = torch.zeros((G, G, G), device=dev)
        view = lambda k: ops.node_max_weight_raw(grid, ops.RayBatch(None, None, S, near, far, camera=camera(poses[k])), 0, M)  # noqa: E731
        r = {"first_view_zeroed_buffer": median_ms(lambda: view(0), before=M.zero_)}
        M.zero_()
        for k in range(99):
            view(k)
        r["view_100_warm_buffer"] = median_ms(lambda: view(99))
        if a.yardstick:
            flat = rf.flatten_rays(rf.cast_rays(rf.CameraIntrinsics(hw, hw, hw * 1.39), poses[0], dev))
            flags = _lib.FLAG_RENDER_DIFFUSE
            r["render_forward_diffuse_same_rays"] = median_ms(lambda: ops.render_forward_raw(grid, flat.origins, flat.directions, None, S, near, far, flags, save=False))
            for dilate in (0, 1, 2):
                r[f"prune_grid_dilate_{dilate}"] = median_ms(lambda: ops.prune_grid_raw(grid, M, 1e-3, dilate, 0.0))
        res[scene] = r
    if a.yardstick:
        n = G**3
        p, g, m, v = (torch.zeros(n, device=dev) for _ in range(4))
        step = [0]

        def adam():
            step[0] += 1
            ops.adam_step_hip(p, g, m, v, 0.03, 0.9, 0.999, 1e-8, step[0])

        res["adam_step_one_parameter_per_node"] = dict(median_ms(adam), bytes=28 * n)
        res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", default=None, help="(internal) measure the library in $RF_LIB_PATH and print one JSON line")
    ap.add_argument("--yardstick", type=int, default=0, help="(internal) also time the render, the prune kernel and rf_adam_step")
    a = ap.parse_args()
    if a.variant is not None:
        print("RESULT " + json.dumps(measure(a)))
        return
    build_variants()
    res = {"grid": a.grid, "sh_degree": a.degree, "samples_per_ray": a.samples, "image": [a.size, a.size], "storage": "split", "variants": {}}
    for i, (guard, dedupe) in enumerate(VARIANTS):
        env = dict(os.environ, RF_LIB_PATH=variant_path(guard, dedupe))
        cmd = [sys.executable, os.path.abspath(__file__), "--grid", str(a.grid), "--degree", str(a.degree), "--samples", str(a.samples), "--size", str(a.size),
               "--variant", f"g{guard}d{dedupe}", "--yardstick", "1" if i == 0 else "0"]
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
        line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1]
        res["variants"][f"guard={guard},dedupe={dedupe}"] = json.loads(line[len("RESULT "):])
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
