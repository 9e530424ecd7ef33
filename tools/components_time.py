"""Time rf_label_components against a torch restatement on the GPU and scipy.ndimage.label on the host.

    python tools/components_time.py [--grids 128 256] [--out profiles/components_time.json]

Split storage, SH degree 0, ReLU, threshold 0.  Fields:
  * uniform: raw densities U(-1, 1) -- half the nodes occupied, far above the percolation threshold: one giant ragged component
    through every tile plus thousands of specks;
  * blobs:   64 balls of radius grid / 16 at random centres, negative elsewhere -- sparse, a few dozen components;
  * full:    every node occupied -- one component (the common case after training: one wave, one root).
HIP events around the whole call (three launches), median of 20 runs after 3 warm-up runs, for connectivity 6, 18 and 26; the time
of each launch comes from torch.profiler's device-side kernel records over 10 further calls (mean per launch; "NOT MEASURED" when
the profiler reports no kernel of the unit).
Yardsticks on the same device, connectivity 26:
  * torch: the obvious restatement -- every occupied node starts with its own index, one max_pool3d sweep (3 x 3 x 3) takes the
    neighbourhood minimum, sweeps repeat until nothing changes (checked on the host every 16 sweeps); timed once per field with
    wall-clock around a synchronised run, the sweep count reported;
  * scipy.ndimage.label on the host INCLUDING the copy of the density tensor to the host and of the labels back (skipped when scipy
    is not importable).
Both yardsticks are checked to give the labelling of the kernel (after canonicalisation) before their time is reported.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def field(dev, G, kind):
    import torch

    gen = torch.Generator(device="cpu").manual_seed(7)
    if kind == "uniform":
        dens = torch.rand((G, G, G), generator=gen) * 2.0 - 1.0
    elif kind == "full":
        dens = torch.ones((G, G, G))
    else:
        centres = torch.rand((64, 3), generator=gen) * G
        ax = torch.arange(G, dtype=torch.float32)
        dens = torch.full((G, G, G), -1.0)
        for c in centres:
            r2 = (ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2
            dens = torch.where(r2 <= (G / 16.0) ** 2, torch.tensor(1.0), dens)
    return dens[..., None].contiguous().to(dev)


def per_launch_us(fn, calls=10):
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for name in ("component_local_kernel", "component_merge_kernel", "component_flatten_kernel"):
                if name in e.key:
                    total = getattr(e, "device_time_total", None)
                    if total is None:
                        total = e.cuda_time_total
                    out[name] = out.get(name, 0.0) + float(total) / calls
        return out if len(out) == 3 else "NOT MEASURED"
    except Exception as exc:  # the profiler is a convenience here, not a dependency
        return f"NOT MEASURED ({type(exc).__name__})"


def torch_sweeps(occ):
    """labels by iterated neighbourhood-minimum sweeps (26-connectivity); (int32 labels, sweeps)"""
    import torch

    n = occ.numel()
    # max_pool3d takes the maximum: carry n - index, so that the maximum is the smallest index (exact in float32 up to 2^24 nodes)
    x = torch.where(occ, (n - torch.arange(n, device=occ.device, dtype=torch.float32)).view(occ.shape), torch.zeros((), device=occ.device))[None, None]
    mask = occ[None, None]
    sweeps = 0
    while True:
        before = x
        for _ in range(16):
            x = torch.where(mask, torch.nn.functional.max_pool3d(x, 3, stride=1, padding=1), x)
        sweeps += 16
        if torch.equal(before, x):
            break
    return torch.where(occ, n - x[0, 0], torch.tensor(-1.0, device=occ.device)).to(torch.int32), sweeps


def scipy_label(dens_dev, dev):
    """scipy.ndimage.label with both copies; (canonical int32 labels on the device, seconds) or None without scipy"""
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        return None
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = dens_dev[..., 0].cpu().numpy()
    lab, count = ndimage.label(host > 0.0, structure=np.ones((3, 3, 3), dtype=bool))
    lab_dev = torch.from_numpy(lab.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    # canonicalise (not timed): scipy numbers the pieces in the order of their first node, which is the order of their smallest index
    flat = lab.reshape(-1)
    first = np.full(count + 1, -1, dtype=np.int64)
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1]
    return torch.from_numpy(np.where(lab > 0, first[lab], -1).astype(np.int32)).to(dev), seconds, int(count)


def time_grid(dev, G):
    import torch

    import thr3ed_atom_amd as rf
    from thr3ed_atom_amd import ops

    out = {}
    for kind in ("uniform", "blobs", "full"):
        dens = field(dev, G, kind)
        grid = rf.VoxelGrid(dens, torch.zeros((G, G, G, 3), device=dev), rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                            density_postactivation=torch.nn.ReLU(), expected_density_scale=1.0, tunable=False, storage="split")
        labels = torch.empty((G, G, G), dtype=torch.int32, device=dev)
        sizes = torch.empty(G**3, dtype=torch.int32, device=dev)
        r = {"occupied_fraction": float((dens > 0).float().mean())}
        for connectivity in (6, 18, 26):
            call = lambda: ops.label_components_raw(grid, 0.0, connectivity, labels, sizes)  # noqa: E731
            r[str(connectivity)] = median_ms(call)
            r[str(connectivity)]["components"] = int((sizes > 0).sum())
            r[str(connectivity)]["largest"] = int(sizes.max())
            r[str(connectivity)]["per_launch_us"] = per_launch_us(call)
        # the yardsticks, connectivity 26 (labels / sizes hold that result now)
        occ = dens[..., 0] > 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        swept, sweeps = torch_sweeps(occ)
        torch.cuda.synchronize()
        r["torch_sweeps"] = {"ms": 1e3 * (time.perf_counter() - t0), "sweeps": sweeps, "equal": bool(torch.equal(swept, labels))}
        found = scipy_label(dens, dev)
        if found is None:
            r["scipy_with_copies"] = "NOT MEASURED (scipy is not importable)"
        else:
            r["scipy_with_copies"] = {"ms": 1e3 * found[1], "components": found[2], "equal": bool(torch.equal(found[0], labels))}
        out[kind] = r
        del grid, dens, labels, sizes
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/components_time.py needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "storage": "split", "threshold": 0.0, "grids": {str(G): time_grid(dev, G) for G in a.grids}}
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
