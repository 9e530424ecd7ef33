"""CPU checks of the iso-surface contract: the oracle (tests/mesh_oracle.py) on analytic lattices, the PLY writer, and the
argument checks of the mesh entry points of the C ABI (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mesh_oracle as mo
from thr3ed_atom_amd import _lib
from thr3ed_atom_amd.mesh import Mesh, read_ply, to8b, write_ply


def analytic(fn, n=24, lo=-1.0, hi=1.0):
    """sigma = fn(p) on the lattice of an n^3 grid over [lo, hi]^3 with m = 1 (guards 0)"""
    aabb = ((lo, hi),) * 3
    coords = mo.lattice_coords(aabb, (n, n, n), 1)
    X, Y, Z = np.meshgrid(*coords, indexing="ij")
    sig = fn(X, Y, Z).astype(np.float32)
    sig[0], sig[-1], sig[:, 0], sig[:, -1], sig[:, :, 0], sig[:, :, -1] = 0, 0, 0, 0, 0, 0
    return sig, coords


def sphere(c, r):
    return lambda X, Y, Z: r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)


def test_sphere_is_closed_oriented_genus_zero():
    sig, coords = analytic(sphere((0.05, -0.02, 0.03), 0.6))
    keys, pos, faces = mo.triangulate(sig, coords, 0.0)
    assert len(faces) > 100 and (np.diff(keys) > 0).all()
    two, once, chi = mo.manifold_report(faces, len(pos))
    assert two and once and chi == 2
    # on the surface within one lattice step
    h = 2.0 / 24
    r = np.linalg.norm(pos - np.array([0.05, -0.02, 0.03], np.float32), axis=1)
    assert np.abs(r - 0.6).max() <= h
    # face normals point outward
    v = pos[faces]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    area = np.linalg.norm(n, axis=1)
    out = np.einsum("ij,ij->i", n, v.mean(1) - np.array([0.05, -0.02, 0.03]))
    assert (out[area > 1e-9] > 0).all()


def test_two_spheres_and_torus():
    two = lambda X, Y, Z: np.maximum(sphere((-0.45, 0, 0), 0.3)(X, Y, Z), sphere((0.45, 0.0, 0.0), 0.3)(X, Y, Z))
    sig, coords = analytic(two)
    _, pos, faces = mo.triangulate(sig, coords, 0.0)
    assert mo.manifold_report(faces, len(pos)) == (True, True, 4)

    torus = lambda X, Y, Z: 0.22 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2)
    sig, coords = analytic(torus, n=32)
    _, pos, faces = mo.triangulate(sig, coords, 0.0)
    assert mo.manifold_report(faces, len(pos)) == (True, True, 0)


def test_negative_level_makes_the_guards_inside():
    """identity densities may be negative: with tau < 0 the guards (sigma = 0) are inside and the mesh still closes"""
    sig, coords = analytic(lambda X, Y, Z: -1.0 + 0.0 * X + np.where(X ** 2 + Y ** 2 + Z ** 2 < 0.25, -1.0, 0.0), n=16)
    _, pos, faces = mo.triangulate(sig, coords, -0.5)
    two, once, chi = mo.manifold_report(faces, len(pos))
    assert two and once and len(faces) > 0


def test_oracle_on_a_voxel_grid_matches_the_lattice():
    """m = 1: interior lattice sigma are the activated node values (to float32 rounding of the node positions)"""
    torch.manual_seed(0)
    dens = torch.rand(5, 4, 6, 1) - 0.3
    aabb = ((-1.0, 1.5), (0.0, 2.0), (-3.0, -1.0))
    sig, coords = mo.lattice_sigma(dens, aabb, 2.0, "relu", 1)
    assert sig.shape == (7, 6, 8)
    np.testing.assert_allclose(sig[1:-1, 1:-1, 1:-1], torch.relu(dens[..., 0] * 2.0).numpy(), rtol=0, atol=1e-5)  # (float32 normalisation: nodes up to an ulp off)
    assert coords[0][0] == np.float32(-1.0) and coords[0][-1] == np.float32(1.5)


def test_write_ply_round_trip(tmp_path):
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int64)
    col = torch.tensor([[0.0, 0.5, 1.0], [0.999, 1.2, -0.1], [0.25, 0.75, 0.1], [1.0, 1.0, 1.0]])
    nrm = torch.nn.functional.normalize(v - 0.25, dim=1)
    path = os.path.join(tmp_path, "t.ply")
    write_ply(Mesh(v, f, col, nrm), path)
    pv, pn, pc, pf = read_ply(path)
    assert (pv == v.numpy()).all() and (pn == nrm.numpy()).all() and (pf == f.numpy()).all()
    assert (pc == to8b(col.numpy())).all()
    assert pc[1].tolist() == [254, 255, 0]  # truncation, clipping
    header = open(path, "rb").read(400).split(b"end_header")[0].decode()
    assert "property list uchar int vertex_indices" in header and "property uchar red" in header
    write_ply(Mesh(v[:0], f[:0], None, None), path)  # empty mesh
    pv, pn, pc, pf = read_ply(path)
    assert pv.shape == (0, 3) and pf.shape == (0, 3)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_mesh_entry_points_check_arguments_without_gpu(lib):
    assert lib.rf_mesh_tiles(None, 1) == -1
    assert lib.rf_mesh_count(None, 1, 0.0, None, None) == -1
    g = _lib.RFGrid()
    assert lib.rf_mesh_tiles(C.byref(g), 1) == -1  # null densities
    g.densities_dev, g.features_dev = 16, 16
    g.dims[0], g.dims[1], g.dims[2] = 4, 5, 6
    g.num_features, g.density_stride, g.feature_stride = 27, 1, 27
    assert lib.rf_mesh_tiles(C.byref(g), 1) == (6 * 7 * 8 + 255) // 256
    assert lib.rf_mesh_tiles(C.byref(g), 2) == (10 * 12 * 14 + 255) // 256
    for m in (0, 9, -1):
        assert lib.rf_mesh_tiles(C.byref(g), m) == -2
        assert lib.rf_mesh_count(C.byref(g), m, 0.0, 16, None) == -2
    assert lib.rf_mesh_count(C.byref(g), 1, float("nan"), 16, None) == -2
    assert lib.rf_mesh_count(C.byref(g), 1, float("inf"), 16, None) == -2
    assert lib.rf_mesh_count(C.byref(g), 1, 0.0, None, None) == -1
    assert lib.rf_mesh_emit(C.byref(g), 1, 0.0, None, 0, 0, None, None, None, None, None, None) == -1
    assert lib.rf_mesh_emit(C.byref(g), 1, 0.0, 16, 4, 0, None, None, None, None, None, None) == -1
    assert lib.rf_mesh_emit(C.byref(g), 1, 0.0, 16, -1, 0, 16, 16, None, None, 16, None) == -2
    g.dims[1] = 0
    assert lib.rf_mesh_tiles(C.byref(g), 1) == -2
    g.dims[1], g.num_features = 5, 5
    assert lib.rf_mesh_tiles(C.byref(g), 1) == -3


def test_extract_mesh_rejects_bad_arguments():
    from thr3ed_atom_amd import extract_mesh

    for bad in (0, 9, 1.5, True):
        with pytest.raises(ValueError):
            extract_mesh(None, 0.0, subdivisions=bad)
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            extract_mesh(None, bad)
