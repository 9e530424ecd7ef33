"""Vector quantisation on the GPU: rf_vq_assign against the assignment bound of tests/vq_model.py on every row,
rf_vq_centroids against float64 weighted means within the bound of its own summation order, vq_kmeans (reproducible, monotone,
exact when every vector is its own code) and compress_voxel_grid end to end -- class counts, stored values, bit-identical renders of
a field that is kept whole, and a compact checkpoint written by the command-line tool.

Measured (MI355X; docs/vq_errors.md): the worst excess of rf_vq_assign over all cases is far inside the bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import vq_model as vm
from tests.helpers import hotdog_like_camera
from tests.test_hip_tighten import S, STORAGES, blob_field, hip_render, make_grid
from thr3ed_atom_amd import _lib

pytestmark = pytest.mark.gpu

U = vm.U
ROWS = (1, 63, 65, 257, 1000)
CODES = (1, 2, 33, 257, 4096)
DIMS = (3, 5, 12, 27, 48, 64)


def device_excess(x, c, index, chunk=128):
    """tests/vq_model.assignment_excess in float64 on the device (the 1000 x 4096 x 64 differences do not fit a quick CPU test):
    per row (d_j - min_i [d_i + E_i]) / E_j, which has to be <= 1; and the true distance to the returned code"""
    x, c = x.double(), c.double()
    D = x.shape[1]
    cn, ca = (c * c).sum(-1), c.abs()
    excess, dj = [], []
    for lo in range(0, x.shape[0], chunk):
        xs, j = x[lo:lo + chunk], index[lo:lo + chunk].long()
        d = ((xs[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        E = (D + 4) * U * ((xs * xs).sum(-1)[:, None] + 2.0 * xs.abs() @ ca.T + cn[None, :])
        rows = torch.arange(xs.shape[0], device=x.device)
        gap, Ej = d[rows, j] - (d + E).min(1).values, E[rows, j]
        excess.append(torch.where(Ej > 0, gap / torch.where(Ej > 0, Ej, torch.ones_like(Ej)), torch.where(gap <= 0, torch.zeros_like(gap), torch.full_like(gap, float("inf")))))
        dj.append(d[rows, j])
    return torch.cat(excess), torch.cat(dj)


def check_assignment(x, c, index, dist):
    """every row inside the bound; the reported distance within (D + 2) u of the true distance to the RETURNED code"""
    D = x.shape[1]
    assert index.dtype == torch.int32 and dist.dtype == torch.float32 and int(index.min()) >= 0 and int(index.max()) < c.shape[0]
    excess, dj = device_excess(x, c, index)
    assert bool((excess <= 1.0).all()), float(excess.max())
    assert bool(((dist.double() - dj).abs() <= (D + 2) * U * dj).all())
    return float(excess.max())


@pytest.mark.parametrize("D", DIMS)
def test_assign_satisfies_the_bound_on_every_row(hip_device, D):
    worst = {}
    for kind in vm.INPUT_KINDS:
        for C in CODES:
            xs, cs = vm.make_inputs(kind, max(ROWS), C, D, 1000 * D + C)
            c = torch.from_numpy(cs).to(hip_device)
            for M in ROWS:
                x = torch.from_numpy(xs[:M]).to(hip_device)
                index, dist = rf.vq_assign(x, c)
                worst[kind] = max(worst.get(kind, -np.inf), check_assignment(x, c, index, dist))
                if kind == "duplicated":  # code j + C // 2 repeats code j < C // 2: the upper twin is never returned
                    assert not bool(((index >= C // 2) & (index < 2 * (C // 2))).any())
                again = rf.vq_assign(x, c)
                assert torch.equal(again[0], index) and torch.equal(again[1].view(torch.int32), dist.view(torch.int32))
    print(f"rf_vq_assign D={D}: worst (d_j - min_i [d_i + E_i]) / E_j per input kind: " + ", ".join(f"{k} {v:+.3f}" for k, v in worst.items()))


def test_random_assignments_fail_the_check(hip_device):
    """the check above can fail: on the centred inputs a uniformly random assignment violates it on at least 95 % of rows"""
    for kind in vm.CENTRED_KINDS:
        xs, cs = vm.make_inputs(kind, 600, 512, 27, 5)
        x, c = torch.from_numpy(xs).to(hip_device), torch.from_numpy(cs).to(hip_device)
        index = torch.from_numpy(np.random.default_rng(9).integers(0, 512, 600).astype(np.int32)).to(hip_device)
        assert float((device_excess(x, c, index)[0] > 1.0).double().mean()) >= 0.95


def test_assign_strided_rows_and_untouched_neighbours(hip_device):
    """rows row_stride > D apart; the outputs written inside larger buffers whose other elements keep their bits"""
    M, C, D, pad = 257, 33, 27, 64
    xs, cs = vm.make_inputs("uniform", M, C, D, 77)
    wide = torch.full((M, D + 5), 1e30, device=hip_device)
    wide[:, :D] = torch.from_numpy(xs).to(hip_device)
    x, c = wide[:, :D], torch.from_numpy(cs).to(hip_device)
    assert x.stride(0) == D + 5
    index, dist = rf.vq_assign(x, c)
    dense = rf.vq_assign(x.contiguous(), c)
    assert torch.equal(index, dense[0]) and torch.equal(dist, dense[1])
    check_assignment(x.contiguous(), c, index, dist)
    ibuf = torch.full((M + 2 * pad,), -12345, dtype=torch.int32, device=hip_device)
    dbuf = torch.full((M + 2 * pad,), -7.5, dtype=torch.float32, device=hip_device)
    stream = torch.cuda.current_stream(hip_device).cuda_stream
    rc = _lib.load().rf_vq_assign(x.data_ptr(), M, D, D + 5, c.data_ptr(), C, ibuf.data_ptr() + 4 * pad, dbuf.data_ptr() + 4 * pad, stream)
    assert rc == 0
    assert torch.equal(ibuf[pad:pad + M], index) and torch.equal(dbuf[pad:pad + M], dist)
    for buf, fill in ((ibuf, -12345), (dbuf, -7.5)):
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + M:] == fill).all())
    assert bool((wide[:, D:] == 1e30).all())
    # no vectors: nothing happens
    empty = rf.vq_assign(torch.zeros((0, D), device=hip_device), c)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)


SEGMENTS = (0, 1, 63, 64, 65, 1000, 5, 0, 17)  # the 5: a segment whose weights are all zero


@pytest.mark.parametrize("D", [3, 27, 64])
def test_centroids_against_float64_weighted_means(hip_device, D):
    """Bound from the kernel's own order: a segment of n vectors is dealt out in 16 sequential streams of
    L = ceil(n / 16) terms, each term one rounded product and one rounded addition, then 4 levels of pairwise additions; the weight
    sum likewise without the product; one division.  |centroid_k - exact_k| <= (2 L + 10) u sum w |x_k| / sum w."""
    rng = np.random.default_rng(40 + D)
    index = np.repeat(np.arange(len(SEGMENTS)), SEGMENTS)
    rng.shuffle(index)
    M = index.size
    x = rng.uniform(-1.0, 1.0, (M, D)).astype(np.float32) + np.float32(0.5)
    w = rng.uniform(0.05, 1.0, M).astype(np.float32)
    w[index == 6] = 0.0
    before = rng.uniform(-1.0, 1.0, (len(SEGMENTS), D)).astype(np.float32)
    xd, wd, idx = torch.from_numpy(x).to(hip_device), torch.from_numpy(w).to(hip_device), torch.from_numpy(index.astype(np.int32)).to(hip_device)
    code = torch.from_numpy(before).to(hip_device)
    sums = rf.vq_update_centroids(xd, wd, idx, code)
    got, worst = code.cpu().numpy(), 0.0
    for cidx, n in enumerate(SEGMENTS):
        members = np.flatnonzero(index == cidx)
        if n == 0 or cidx == 6:
            assert (got[cidx].view(np.int32) == before[cidx].view(np.int32)).all()  # an empty segment, a zero weight sum: untouched
            assert float(sums[cidx]) == 0.0
            continue
        want, scale = vm.weighted_centroid(x, w, members)
        bound = (2 * -(-n // 16) + 10) * U * scale
        err = np.abs(got[cidx].astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (cidx, n, float((err / bound).max()))
        assert abs(float(sums[cidx]) - w[members].astype(np.float64).sum()) <= (-(-n // 16) + 4) * U * w[members].astype(np.float64).sum()
    print(f"rf_vq_centroids D={D}: worst error / bound {worst:.3f}")
    again = torch.from_numpy(before).to(hip_device)
    rf.vq_update_centroids(xd, wd, idx, again)
    assert torch.equal(again.view(torch.int32), code.view(torch.int32))


@pytest.mark.parametrize("D", [12, 27])
def test_kmeans_is_reproducible_and_monotone(hip_device, D):
    rng = np.random.default_rng(60 + D)
    centres = rng.uniform(-1.0, 1.0, (40, D))
    x = torch.from_numpy((centres[rng.integers(0, 40, 3000)] + 0.1 * rng.normal(size=(3000, D))).astype(np.float32)).to(hip_device)
    w = torch.from_numpy(rng.uniform(0.01, 1.0, 3000).astype(np.float32)).to(hip_device)
    codebook, index, distortions = rf.vq_kmeans(x, w, 64, iterations=8, seed=3)
    assert codebook.shape == (64, D) and index.shape == (3000,) and distortions.shape == (9,) and distortions.dtype == torch.float64
    again = rf.vq_kmeans(x, w, 64, iterations=8, seed=3)
    assert torch.equal(again[0].view(torch.int32), codebook.view(torch.int32)) and torch.equal(again[1], index) and torch.equal(again[2], distortions)
    other = rf.vq_kmeans(x, w, 64, iterations=8, seed=4)
    assert not torch.equal(other[0], codebook)
    d = distortions.cpu().numpy()
    print(f"vq_kmeans D={D}: distortions " + " ".join(f"{v:.5e}" for v in d))
    assert (d[1:] <= d[:-1] * (1.0 + 2 * (D + 2) * U)).all() and d[-1] < 0.9 * d[0]
    # the returned index belongs to the returned codebook
    final = rf.vq_assign(x, codebook)
    assert torch.equal(final[0], index)
    assert abs(float((w.double() * final[1].double()).sum() / w.double().sum()) - d[-1]) <= 1e-12 * d[-1]


def test_kmeans_with_a_code_per_vector(hip_device):
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (100, 12)).astype(np.float32)).to(hip_device)
    w = torch.from_numpy(rng.uniform(0.1, 1.0, 100).astype(np.float32)).to(hip_device)
    codebook, index, distortions = rf.vq_kmeans(x, w, 4096, iterations=3, seed=0)
    assert codebook.shape == (100, 12)  # capped at M
    assert sorted(index.tolist()) == list(range(100))
    assert bool(((codebook[index.long()] - x).abs() <= 4 * U * x.abs()).all())
    assert float(distortions.max()) <= (4 * U) ** 2 * 12


# ---- compress_voxel_grid end to end ----------------------------------------------------------------------------------------
def _views():
    cam = hotdog_like_camera()
    poses = [rf.pose_spherical(40.0 + 90.0 * k, -35.0, cam["radius"]) for k in range(4)]
    return poses, rf.CameraIntrinsics(8, 8, 14.0), rf.CameraBounds(cam["near"], cam["far"])


def _importance(grid):
    poses, intrinsics, bounds = _views()
    return rf.node_max_weights(grid, poses, intrinsics, bounds, S)


def test_compress_partitions_stores_and_quantises(hip_device):
    dens, feat = blob_field()
    F = feat.shape[-1]
    grid = make_grid(hip_device, dens, feat, "split")
    importance = _importance(grid)
    classes = vm.partition_by_shares(importance.cpu().numpy(), 0.01, 0.3)
    counts = tuple(int((classes == k).sum()) for k in (vm.PRUNED, vm.KEPT, vm.QUANTISED))
    print(f"compress 16^3: pruned / kept / quantised = {counts}")
    assert min(counts) > 0 and counts[2] > 16
    field = rf.compress_voxel_grid(grid, importance, prune_share=0.01, keep_share=0.3, num_codes=16, iterations=4, value_dtype="float32")
    stats = field.stats
    assert (stats["pruned"], stats["kept"], stats["quantised"]) == counts and (field.node_classes() == classes).all()
    assert stats["num_codes"] == 16 and len(stats["distortions"]) == 5 and stats["distortion"] == stats["distortions"][-1] > 0.0
    back = rf.CompressedField.from_bytes(field.to_bytes(), config=field.config).decompress(device=hip_device, storage="bricked")
    cls = torch.from_numpy(classes).to(hip_device)
    d0, f0 = grid.densities.reshape(-1), grid.features.reshape(-1, F)
    d1, f1 = back.densities.reshape(-1), back.features.reshape(-1, F)
    assert bool((d1[cls == vm.PRUNED] == 0).all()) and bool((f1[cls == vm.PRUNED] == 0).all())
    assert torch.equal(d1[cls != vm.PRUNED], d0[cls != vm.PRUNED]) and torch.equal(f1[cls == vm.KEPT], f0[cls == vm.KEPT])
    codebook = torch.from_numpy(field.codebook).to(hip_device)
    index = torch.from_numpy(field.indices.astype(np.int32)).to(hip_device)
    assert torch.equal(f1[cls == vm.QUANTISED], codebook[index.long()])
    x = f0[cls == vm.QUANTISED].contiguous()
    excess, _ = device_excess(x, codebook, index)
    assert bool((excess <= 1.0).all())
    # the default float16 values: the stored numbers are the float16 roundings
    half = rf.compress_voxel_grid(grid, importance, prune_share=0.01, keep_share=0.3, num_codes=16, iterations=4).decompress(device=hip_device)
    assert torch.equal(half.features.reshape(-1, F)[cls == vm.KEPT], f0[cls == vm.KEPT].half().float())
    assert torch.equal(half.features.reshape(-1, F)[cls == vm.QUANTISED], codebook.half().float()[index.long()])


@pytest.mark.parametrize("storage", STORAGES)
def test_a_field_kept_whole_renders_bit_identically(hip_device, storage):
    dens, feat = blob_field()
    grid = make_grid(hip_device, dens, feat, storage)
    importance = _importance(grid) + 1e-3  # all positive
    field = rf.compress_voxel_grid(grid, importance, prune_share=0.0, keep_share=1.0, value_dtype="float32")
    assert field.stats["kept"] == 16**3
    back = field.decompress(device=hip_device, storage=storage)
    a, b = hip_render(grid, hip_device), hip_render(back, hip_device)
    assert a["acc"].max() > 0.5
    for k in a:
        assert (a[k] == b[k]).all(), k


def test_cli_writes_a_compact_checkpoint_the_loader_reads(hip_device, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dens, feat = blob_field()
    poses, intrinsics, bounds = _views()
    cfg = rf.SHVoxGridRenderConfig(S, bounds, perturb_sampled_points=False, white_bkgd=False)
    grid = make_grid(hip_device, dens, feat, "reference")
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    src, dst, data = tmp_path / "model.pth", tmp_path / "model_vq.pth", tmp_path / "views.npz"
    torch.save(model.get_save_info(extra_info={"note": "kept"}), src)
    # the last two views of a data file are held out: the statistic sees the four of _views()
    mats = np.stack([torch.cat([p.rotation, p.translation], dim=1).cpu().numpy() for p in poses + poses[:2]]).astype(np.float32)
    np.savez(data, images=np.zeros((6, 3, 8, 8), np.float32), poses=mats, focal=14.0, near=bounds.near, far=bounds.far)
    options = ["--prune_share", "0.01", "--keep_share", "0.3", "--num_codes", "16", "--iterations", "4", "--seed", "2"]
    r = subprocess.run([sys.executable, "scripts/compress_sh_based_voxel_grid.py", "-i", str(src), "-o", str(dst), "-d", str(data)] + options,
                       cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    field = rf.compress_voxel_grid(model, _importance(grid), prune_share=0.01, keep_share=0.3, num_codes=16, iterations=4, seed=2)
    stats = field.stats
    assert f"pruned nodes: {stats['pruned']}  kept nodes: {stats['kept']}  quantised nodes: {stats['quantised']}  codes: 16" in r.stdout
    assert "distortion per assignment:" in r.stdout and f"file size: {os.path.getsize(src)} -> {os.path.getsize(dst)} bytes" in r.stdout
    assert os.path.getsize(dst) < os.path.getsize(src) / 4
    loaded, extra = rf.create_volumetric_model_from_saved_model(dst, rf.create_voxel_grid_from_saved_info_dict, device=hip_device)
    want = field.decompress(device=hip_device)
    got = loaded.thre3d_repr
    assert extra == {"note": "kept"} and torch.equal(got.densities, want.densities) and torch.equal(got.features, want.features)
    a, b = hip_render(got, hip_device), hip_render(want, hip_device)
    assert a["acc"].max() > 0.5
    for k in a:
        assert (a[k] == b[k]).all(), k
