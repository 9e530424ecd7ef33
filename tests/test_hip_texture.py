"""GPU: rf.bake_texture (csrc/texture_kernels.hip) against the float64 model of tests/texture_model.py within the per-texel bound of
docs/texture_errors.md, on the smallest inputs at which it can go wrong (tests/texture_model.py CASES: every storage, SH degree,
density mode, diffuse on and off, T = 1, 2, 3, 7, patch 2, 3, 8, samples 1, 5, 16, reach 0, half a voxel and three voxels, a partly
empty last row; triangles inside, across, outside and larger than the box and of zero area); unowned texels, determinism, bad
faces, argument errors; and the export chain end to end on a ball of one colour.

Measured on an MI355X: see docs/texture_errors.md for the worst ratio of error to bound over these cases."""
import os

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import texture_model as tm

pytestmark = pytest.mark.gpu

MODES = {
    "relu": (torch.nn.Identity(), torch.nn.ReLU()),
    "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
    "abs": (torch.abs, torch.nn.Identity()),
    "identity": (torch.nn.Identity(), torch.nn.Identity()),
}


def grid_of(made, device):
    pre, post = MODES[made["mode"]]
    return rf.VoxelGrid(torch.from_numpy(made["densities"]).to(device), torch.from_numpy(made["features"]).to(device), rf.VoxelSize(*made["voxel"]),
                        rf.VoxelGridLocation(*made["loc"]), density_preactivation=pre, density_postactivation=post, expected_density_scale=made["rho"],
                        storage=made["storage"])


def mesh_of(made, device):
    return rf.Mesh(torch.from_numpy(made["vertices"]).to(device), torch.from_numpy(made["faces"]).to(device), None, None)


@pytest.mark.parametrize("case", tm.CASES, ids=tm.case_id)
def test_matches_the_model(hip_device, case):
    made = tm.make_case(case)
    ref = tm.bake_case(made)
    grid, mesh = grid_of(made, hip_device), mesh_of(made, hip_device)
    assert tuple(tuple(float(x) for x in r) for r in grid.aabb) == tuple(tuple(float(x) for x in r) for r in made["aabb"])
    kwargs = dict(reach=made["reach"], samples=made["samples"], diffuse=made["diffuse"], cols=made["cols"])
    bake = rf.bake_texture(mesh, grid, made["patch"], **kwargs)
    again = rf.bake_texture(mesh, grid, made["patch"], **kwargs)
    lay = ref["layout"]
    assert (bake.patch, bake.block, bake.cols, bake.rows) == (lay["patch"], lay["block"], lay["cols"], lay["rows"])
    assert bake.texture.shape == (lay["height"], lay["width"], 3) and bake.opacity.shape == (lay["height"], lay["width"])
    assert bake.texture.dtype == torch.float32 and bake.texture.device.type == "cuda"
    assert torch.equal(bake.texture, again.texture) and torch.equal(bake.opacity, again.opacity)  # bitwise
    assert np.array_equal(bake.uvs.cpu().numpy(), tm.uvs(len(made["faces"]), made["patch"], made["cols"]).astype(np.float32))
    texture, opacity = bake.texture.cpu().numpy().astype(np.float64), bake.opacity.cpu().numpy().astype(np.float64)
    owned, bound = ref["owned"], ref["bound"]
    assert (texture[~owned] == 0).all() and (opacity[~owned] == 0).all()
    assert not ref["near_boundary"].any() and bound[owned].max() < tm.HALF_STEP
    err_t = np.abs(texture - ref["texture"]).max(-1)
    err_o = np.abs(opacity - ref["opacity"])
    ratio = max((err_t[owned] / bound[owned]).max(), (err_o[owned] / bound[owned]).max())
    print(f"texture bake {tm.case_id(case)}: worst error {max(err_t.max(), err_o.max()):.3e}, worst bound {bound.max():.3e}, worst error / bound {ratio:.4f}")
    assert (err_t[owned] <= bound[owned]).all() and (err_o[owned] <= bound[owned]).all(), ratio
    if made["reach"] == 0.0:
        assert (opacity == 0).all()
    bare = rf.bake_texture(mesh, grid, made["patch"], opacity=False, **kwargs)
    assert bare.opacity is None and torch.equal(bare.texture, bake.texture)


def test_bad_faces_and_argument_errors(hip_device):
    made = tm.make_case(tm.CASES[2])
    grid, mesh = grid_of(made, hip_device), mesh_of(made, hip_device)
    good = rf.bake_texture(mesh, grid, 3, reach=made["reach"], samples=5)
    V = mesh.vertices.shape[0]
    for bad_index in (V, -1, 2**40):
        faces = mesh.faces.clone()
        faces[1, 2] = bad_index
        with pytest.raises(ValueError, match="faces index outside"):
            rf.bake_texture(mesh._replace(faces=faces), grid, 3, reach=made["reach"], samples=5)
    # the raw call: the bad face's texels are 0, the others what they were, the status word says so
    from thr3ed_atom_amd import _lib, texture as tx
    import ctypes as C
    faces = mesh.faces.clone()
    faces[1, 2] = V
    lay = tx.atlas_layout(3, 3)
    out = torch.full((lay.height, lay.width, 3), 7.0, device=hip_device)
    op = torch.full((lay.height, lay.width), 7.0, device=hip_device)
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    rf_grid = grid.to_rf_grid()
    rc = _lib.load().rf_texture_bake(C.byref(rf_grid), mesh.vertices.data_ptr(), V, faces.data_ptr(), 3, 3, lay.cols, lay.rows, made["reach"], 5, 0,
                                     out.data_ptr(), op.data_ptr(), status.data_ptr(), torch.cuda.current_stream(hip_device).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and int(status.item()) == 1
    face = torch.from_numpy(tm.texel_table(3, 3)["face"]).to(hip_device)
    assert (out[face == 1] == 0).all() and (op[face == 1] == 0).all() and (out[face == -1] == 0).all()
    assert torch.equal(out[(face == 0) | (face == 2)], good.texture[(face == 0) | (face == 2)]) and torch.isfinite(out).all()
    # argument errors of the Python layer
    for kwargs in (dict(patch=1), dict(patch=65), dict(samples=0), dict(samples=257), dict(reach=-0.1), dict(reach=float("nan")), dict(cols=0)):
        with pytest.raises(ValueError):
            rf.bake_texture(mesh, grid, **{"patch": 3, **kwargs})
    with pytest.raises(ValueError, match="not finite"):
        rf.bake_texture(mesh._replace(vertices=mesh.vertices.clone().index_fill_(0, torch.tensor([0], device=hip_device), float("inf"))), grid, 3)
    with pytest.raises(ValueError, match="HIP device"):
        rf.bake_texture(rf.Mesh(mesh.vertices.cpu(), mesh.faces.cpu(), None, None), grid, 3)
    cpu_grid = rf.VoxelGrid(torch.zeros(2, 2, 2, 1), torch.zeros(2, 2, 2, 3), rf.VoxelSize(1, 1, 1))
    with pytest.raises(ValueError, match="HIP device"):
        rf.bake_texture(mesh, cpu_grid, 3)
    empty = rf.bake_texture(rf.Mesh(mesh.vertices, mesh.faces[:0], None, None), grid, 8)
    assert empty.texture.shape == (0, 0, 3) and empty.opacity.shape == (0, 0) and empty.uvs.shape == (0, 3, 2) and (empty.cols, empty.rows) == (0, 0)
    # the default reach is twice the largest voxel edge, and a VolumetricModel-like wrapper is unwrapped
    class Wrapper:
        thre3d_repr = grid
    a = rf.bake_texture(mesh, Wrapper(), 3, samples=5)
    b = rf.bake_texture(mesh, grid, 3, reach=2.0 * max(made["voxel"]), samples=5)
    assert torch.equal(a.texture, b.texture)


def test_export_chain_on_a_ball_of_one_colour(hip_device, tmp_path):
    """extract_mesh -> simplify_mesh -> bake_texture -> write_obj on a 16^3 ball field of one constant colour; the three files parsed back"""
    G = 16
    ax = (np.arange(G, dtype=np.float32) + 0.5) / G * 2.0 - 1.0
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    dens = torch.from_numpy((0.6 - r).astype(np.float32)[..., None])
    coeff = np.array([1.2, -0.4, 0.3], np.float32)
    feat = torch.from_numpy(np.broadcast_to(coeff, (G, G, G, 3)).copy())
    voxel = 2.0 / G
    grid = rf.VoxelGrid(dens.to(hip_device), feat.to(hip_device), rf.VoxelSize(voxel, voxel, voxel), density_preactivation=MODES["relu"][0],
                        density_postactivation=MODES["relu"][1], expected_density_scale=20.0, storage="split")
    mesh = rf.simplify_mesh(rf.extract_mesh(grid, 1.0, subdivisions=2), 2 * voxel)
    T, V = mesh.faces.shape[0], mesh.vertices.shape[0]
    assert T > 50
    bake = rf.bake_texture(mesh, grid, 4, reach=0.5 * voxel, samples=4)  # (the reach stays inside the box, where the zero padding of the colour does not reach)
    stem = str(tmp_path / "ball")
    rf.write_obj(mesh, bake, stem)
    lines = open(stem + ".obj").read().splitlines()
    kinds = {k: [ln.split()[1:] for ln in lines if ln.startswith(k + " ")] for k in ("v", "vt", "vn", "f", "mtllib", "usemtl")}
    assert len(kinds["v"]) == V and len(kinds["vn"]) == V and len(kinds["vt"]) == 3 * T and len(kinds["f"]) == T
    assert kinds["mtllib"] == [["ball.mtl"]] and kinds["usemtl"] == [["ball"]]
    uv = np.array(kinds["vt"], dtype=np.float64)
    assert (uv > 0).all() and (uv < 1).all()
    assert np.abs(np.array(kinds["v"], dtype=np.float64) - mesh.vertices.cpu().numpy()).max() <= 1e-6
    corner = np.array([[[int(x) for x in c.split("/")] for c in f] for f in kinds["f"]])  # [T, 3, (v, vt, vn)]
    assert np.array_equal(corner[..., 0] - 1, mesh.faces.cpu().numpy()) and np.array_equal(corner[..., 2], corner[..., 0])
    assert np.array_equal(corner[..., 1].reshape(-1), np.arange(1, 3 * T + 1))
    mtl = open(stem + ".mtl").read().splitlines()
    try:  # (write_obj stores the uint8 array as .npy where PIL is absent)
        from PIL import Image
        name, image = "ball.png", np.asarray(Image.open(stem + ".png"))
    except ImportError:
        name, image = "ball.npy", np.load(stem + ".npy")
    assert "newmtl ball" in mtl and f"map_Kd {name}" in mtl
    assert image.shape == (bake.rows * bake.block, bake.cols * bake.block, 3) and image.dtype == np.uint8
    want = 255.0 / (1.0 + np.exp(-0.28209479177387814 * coeff.astype(np.float64)))
    owned = torch.from_numpy(tm.texel_table(T, 4)["face"] >= 0)
    assert owned.sum() > 0 and np.abs(image[owned.numpy()].astype(np.float64) - want).max() <= 1.0
    assert (image[~owned.numpy()] == 0).all()
    assert os.path.getsize(os.path.join(str(tmp_path), name)) > 0
