"""GPU: iso-surface extraction (thr3ed_atom_amd.extract_mesh, csrc/mesh_kernels.hip) against the CPU oracle of the contract
(tests/mesh_oracle.py): identical faces, identical vertex order, positions / colours / normals within tolerance, on every storage,
every density mode, SH degrees 0 and 2, subdivisions 1-3, non-cubic dims, unequal voxel sizes and an offset grid; closed oriented
2-manifolds on a 128^3 sparse scene; empty results; determinism; the CLI on the reference-written and a freshly trained checkpoint."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_oracle as mo
from tests.helpers import REPO_ROOT, procedural_grid, sparse_scene_grid
from thr3ed_atom_amd.mesh import read_ply

pytestmark = pytest.mark.gpu

MODES = {
    "relu": (torch.nn.Identity(), torch.nn.ReLU()),
    "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
    "abs": (torch.abs, torch.nn.Identity()),
    "identity": (torch.nn.Identity(), torch.nn.Identity()),
}


def make_grid(dens, feat, mode, storage, voxel=(0.2, 0.2, 0.2), loc=(0.0, 0.0, 0.0), scale=3.0, device=None):
    pre, post = MODES[mode]
    return rf.VoxelGrid(dens.to(device), feat.to(device), rf.VoxelSize(*voxel), rf.VoxelGridLocation(*loc), density_preactivation=pre,
                        density_postactivation=post, expected_density_scale=scale, storage=storage)


def pick_level(sigma, quantile):
    """a level near the quantile of the interior lattice values that is at least 1e-4 max|sigma| away from EVERY lattice value"""
    vals = np.unique(sigma)
    gap = 1e-4 * max(float(np.abs(vals).max()), 1e-30)
    target = float(np.quantile(sigma[1:-1, 1:-1, 1:-1], quantile))
    mids = (vals[1:] + vals[:-1]) / 2
    ok = (vals[1:] - vals[:-1]) >= 2 * gap
    assert ok.any()
    tau = float(mids[ok][np.argmin(np.abs(mids[ok] - target))])
    assert np.abs(vals - np.float32(tau)).min() >= gap
    return tau


def compare(mesh, ref, aabb, what=""):
    V, T = len(ref["keys"]), len(ref["faces"])
    assert mesh.vertices.shape == (V, 3) and mesh.faces.shape == (T, 3), (what, mesh.vertices.shape, V, mesh.faces.shape, T)
    assert mesh.faces.dtype == torch.int64 and mesh.vertices.dtype == torch.float32
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(ref["faces"])), what
    extent = max(hi - lo for lo, hi in aabb)
    assert np.abs(mesh.vertices.cpu().numpy() - ref["vertices"]).max(initial=0) <= 1e-6 * extent, what
    assert np.abs(mesh.colours.cpu().numpy() - ref["colours"]).max(initial=0) <= 1e-6, what
    n, rn = mesh.normals.cpu().numpy().astype(np.float64), ref["normals"].astype(np.float64)
    big = ref["grad_norm"] > 1e-3 * ref["grad_norm"].max(initial=0)
    cos = np.clip((n[big] * rn[big]).sum(1), -1, 1)
    assert (np.arccos(cos) <= 1e-3).all(), (what, np.arccos(cos).max(initial=0))
    assert np.abs(np.linalg.norm(n[big], axis=1) - 1).max(initial=0) <= 1e-5


CASES = [
    # storage, mode, F, m, dims, voxel, location, density shift, quantile
    ("reference", "relu", 3, 1, (8, 8, 8), (0.2, 0.2, 0.2), (0.0, 0.0, 0.0), 0.0, 0.7),
    ("split", "relu", 27, 2, (13, 9, 17), (0.2, 0.3, 0.15), (0.4, -1.0, 2.5), 0.0, 0.7),
    ("bricked", "relu", 27, 3, (13, 9, 17), (0.2, 0.3, 0.15), (0.0, 0.0, 0.0), 0.0, 0.8),
    ("reference", "softplus", 27, 2, (10, 12, 7), (0.25, 0.25, 0.4), (1.0, 0.5, -0.25), 0.0, 0.6),
    ("bricked", "softplus", 3, 1, (9, 17, 11), (0.2, 0.2, 0.2), (0.0, 0.0, 0.0), 0.0, 0.5),
    ("split", "abs", 3, 3, (7, 9, 6), (0.3, 0.2, 0.25), (0.0, 0.0, 0.0), 0.0, 0.6),
    ("reference", "abs", 27, 1, (13, 9, 17), (0.2, 0.2, 0.2), (0.0, 0.0, 0.0), 0.0, 0.4),
    ("split", "identity", 27, 2, (9, 10, 11), (0.2, 0.2, 0.2), (0.0, 0.0, 0.0), -0.2, 0.3),
    ("reference", "identity", 3, 1, (13, 9, 17), (0.2, 0.3, 0.15), (0.0, 0.0, 0.0), -0.5, 0.2),
    ("bricked", "identity", 27, 3, (6, 11, 9), (0.3, 0.2, 0.2), (-0.5, 0.0, 0.0), 0.3, 0.6),
]


@pytest.mark.parametrize("storage,mode,F,m,dims,voxel,loc,shift,quantile", CASES)
def test_matches_the_oracle(hip_device, storage, mode, F, m, dims, voxel, loc, shift, quantile):
    dens, feat = procedural_grid(dims, F, 7 + F + m)
    dens = dens + np.float32(shift)
    grid = make_grid(dens, feat, mode, storage, voxel, loc, device=hip_device)
    aabb = grid.aabb
    sigma, _ = mo.lattice_sigma(dens, aabb, 3.0, mode, m)
    tau = pick_level(sigma, quantile)
    if mode == "identity" and shift < 0:
        assert tau < 0  # the guards (sigma = 0) are inside
    ref = mo.extract(dens, feat, aabb, 3.0, mode, tau, m)
    mesh = rf.extract_mesh(grid, tau, subdivisions=m)
    torch.cuda.synchronize()
    assert len(ref["faces"]) > 0
    compare(mesh, ref, aabb, f"{storage}/{mode}/F{F}/m{m}")
    two, once, _ = mo.manifold_report(mesh.faces.cpu().numpy(), len(mesh.vertices))
    assert two and once


def test_sparse_scene_128_closed_oriented_and_equal_to_the_oracle(hip_device):
    G, m = 128, 2
    dens, feat = sparse_scene_grid((G, G, G), 27, 11)
    grid = make_grid(dens, feat, "relu", "split", voxel=(3.0 / G,) * 3, scale=10.0, device=hip_device)
    aabb = grid.aabb
    sigma, _ = mo.lattice_sigma(dens, aabb, 10.0, "relu", m)
    tau = pick_level(sigma, 0.9)
    assert tau > 0
    mesh = rf.extract_mesh(grid, tau, subdivisions=m)
    f = mesh.faces.cpu().numpy()
    two, once, chi = mo.manifold_report(f, len(mesh.vertices))
    assert len(f) > 1000 and two and once and chi % 2 == 0
    # oriented outward: on a closed mesh the signed volume is positive
    v = mesh.vertices.cpu().double()[mesh.faces.cpu()]
    assert torch.linalg.det(v).sum().item() > 0
    ref = mo.extract(dens, feat, aabb, 10.0, "relu", tau, m)
    compare(mesh, ref, aabb, "sparse 128^3")


def test_empty_and_deterministic(hip_device):
    dens, feat = sparse_scene_grid((24, 20, 28), 27, 3)
    grid = make_grid(dens, feat, "relu", "bricked", voxel=(0.1, 0.12, 0.09), scale=10.0, device=hip_device)
    empty = rf.extract_mesh(grid, 1e6, subdivisions=2)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.colours.shape == (0, 3) and empty.normals.shape == (0, 3)
    assert empty.vertices.device.type == "cuda"
    a = rf.extract_mesh(grid, 0.7, subdivisions=3)
    b = rf.extract_mesh(grid, 0.7, subdivisions=3)
    assert len(a.faces) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    bare = rf.extract_mesh(grid, 0.7, subdivisions=3, colours=False, normals=False)
    assert bare.colours is None and bare.normals is None
    assert torch.equal(bare.vertices, a.vertices) and torch.equal(bare.faces, a.faces)
    with pytest.raises(ValueError):
        rf.extract_mesh(grid, float("nan"))
    with pytest.raises(ValueError):
        rf.extract_mesh(grid, 0.5, subdivisions=9)


def _run(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    return subprocess.run([sys.executable] + args, cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _check_ply(path):
    v, n, c, f = read_ply(path)
    assert len(v) > 0 and len(f) > 0 and np.isfinite(v).all()
    two, once, _ = mo.manifold_report(f, len(v))
    assert two and once


def test_cli_on_reference_and_trained_checkpoints(hip_device, tmp_path):
    ref_ckpt = os.path.join(REPO_ROOT, "tests", "golden", "reference_checkpoint.pth")
    out = tmp_path / "ref.ply"
    r = _run(["scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", ref_ckpt, "-o", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "V = " in r.stdout and "T = " in r.stdout
    _check_ply(out)

    run = tmp_path / "run"
    r = _run(["scripts/train_sh_based_voxel_grid.py", "-o", str(run), "--synthetic", "True", "--synthetic_size", "48", "--grid_dims", "32", "32", "32",
              "--sh_degree", "0", "--ray_batch_size", "2048", "--train_num_samples_per_ray", "64", "--render_num_samples_per_ray", "64",
              "--num_stages", "1", "--num_iterations_per_stage", "20", "--save_frequency", "1000", "--test_frequency", "1000",
              "--summary_frequency", "10", "--num_workers", "2", "--feedback_frequency", "1000", "--fast_debug_mode", "False"])
    assert r.returncode == 0, r.stderr[-2000:]
    ckpt = run / "saved_models" / "model_final.pth"
    out = tmp_path / "own.ply"
    r = _run(["scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", str(ckpt), "-o", str(out), "--subdivisions", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    _check_ply(out)
