"""GPU: rf_mesh_face_pseudonormals, rf_mesh_signed_distance, rf.MeshSignGrid, rf.point_mesh_signed_distance, rf.mesh_to_sdf and
rf.signed_mesh_distance on the fixtures of tests/mesh_sign_model.py -- the cube (A), the cube with a cavity (B), the icosphere (C), the
L-shaped prism with a reflex edge and a thin spike (D) -- with 4096 random queries each plus every vertex, edge midpoint and face
centroid and their offsets to both sides (more than one block, every feature kind with both signs), and on the extraction of a ball
on 12^3 nodes (E).  |signed| has the forward's bits, the feature is the float32 model's, the sign is the float64 model's wherever |s|
exceeds the decision margin of docs/mesh_sign_errors.md, and nothing depends on the cell size or the run.

Measured on an MI355X: docs/mesh_sign_errors.md has the worst ratios of error to bound."""
import warnings

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_distance_model as M
from tests import mesh_sign_model as SM
from thr3ed_atom_amd import mesh_sign

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = sorted(SM.MESHES)
_cache = {}


def on(device, array, dtype=None):
    return torch.from_numpy(np.array(array, dtype=dtype)).to(device)


def mesh_on(device, v, f):
    return rf.Mesh(on(device, v, f32), on(device, f, np.int64), None, None)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


def run(device, name, cell_size=None):
    """numpy dict of one MeshSignGrid.signed_distance(..., return_features=True) over the fixture's queries"""
    v, f, q, _ = SM.fixture(name)
    grid = rf.MeshSignGrid(mesh_on(device, v, f), cell_size)
    found = grid.signed_distance(on(device, q, f32), return_features=True)
    out = {k: t.cpu().numpy() for k, t in found._asdict().items()}
    out["normals"], out["vertex_normals"] = grid.normals.cpu().numpy(), grid.vertex_normals.cpu().numpy()
    out["unsigned"] = grid.grid.closest(on(device, q, f32))
    return out


def result(device, name):
    """per fixture, computed once and left unchanged"""
    if name not in _cache:
        _cache[name] = run(device, name)
        for a in _cache[name].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_magnitude_face_and_point_are_the_forwards(hip_device, name):
    got = result(hip_device, name)
    d, face, point = (t.cpu().numpy() for t in got["unsigned"])
    assert (bits(np.abs(got["distance"])) == bits(d)).all()
    assert (got["face"] == face).all() and (bits(got["point"]) == bits(point)).all()
    assert np.isfinite(got["distance"]).all() and (face >= 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_the_feature_is_the_float32_models(hip_device, name):
    v, f, q, _ = SM.fixture(name)
    got = result(hip_device, name)
    model = SM.signed_distance(q, v, f, got["face"], np.float32)
    assert (got["feature"][:, 0] == model["kind"]).all(), np.nonzero(got["feature"][:, 0] != model["kind"])[0][:10]
    assert (got["feature"][:, 1] == model["index"]).all()
    assert (bits(np.abs(got["distance"])) == bits(np.sqrt(model["d2"]))).all()
    seen = {(int(k), bool(s)) for k, s in zip(got["feature"][:, 0], got["distance"] < 0)}
    if name == "cavity":
        assert seen == {(k, s) for k in (0, 1, 2) for s in (False, True)}


@pytest.mark.parametrize("name", NAMES)
def test_the_sign_is_the_float64_models_above_the_decision_margin(hip_device, name):
    v, f, q, groups = SM.fixture(name)
    got, ref = result(hip_device, name), SM.reference(name)
    decided = np.abs(ref["result"]["s"]) > ref["margin"]
    assert decided[groups["random"]].mean() >= 0.99 and decided[groups["off"]].all()
    want = ref["result"]["signed"] < 0
    assert ((got["distance"] < 0) == want)[decided].all(), np.nonzero(decided & ((got["distance"] < 0) != want))[0][:10]
    # the kernel's own s, through the normal it reports, against the float64 s of the SAME face and feature
    same = SM.signed_distance(q, v, f, got["face"], np.float64, region=SM.signed_distance(q, v, f, got["face"], np.float32)["region"])
    s32 = M._dot((q - got["point"]).astype(f32), got["normal"])
    margin = SM.decision_margin(q, v, f, got["face"], same)
    agree = same["kind"] == got["feature"][:, 0]
    ratio = np.abs(s32.astype(np.float64) - same["s"])[agree] / margin[agree]
    print(f"{name}: worst |s32 - s64| / margin {ratio.max():.4f} over {int(agree.sum())} queries")
    assert ratio.max() <= 1.0
    # on the surface: +0, never -0
    zero = got["distance"] == 0
    assert not np.signbit(got["distance"][zero]).any()
    at_vertices = slice(groups["on"].start, groups["on"].start + len(v))
    assert zero[at_vertices].all() and (got["feature"][at_vertices, 0] == SM.VERTEX).all()
    if name in ("cube", "cavity"):  # dyadic coordinates: every feature point is on the surface exactly
        assert zero[groups["on"]].all()


@pytest.mark.parametrize("name", ["cube", "prism"])
def test_identical_bits_for_every_cell_size_and_every_run(hip_device, name):
    first = result(hip_device, name)
    v = SM.fixture(name)[0]
    single = float(4.0 * (v.max(0) - v.min(0)).max())  # one cell holds the whole mesh
    for cell_size in (None, 0.37, single):
        again = run(hip_device, name, cell_size)
        for key in ("distance", "feature", "normal", "face", "point", "normals", "vertex_normals"):
            assert (bits(again[key]) == bits(first[key])).all(), (cell_size, key)
    assert rf.MeshSignGrid(mesh_on(hip_device, *SM.fixture(name)[:2]), single).grid.lattice.cells.prod() == 1


@pytest.mark.parametrize("name", NAMES)
def test_the_tables_lie_within_their_bounds(hip_device, name):
    v, f, _, _ = SM.fixture(name)
    got, model = result(hip_device, name), SM.tables(v, f)
    e_normal, _, e_vertex = SM.table_bounds(v, f)
    r_normal = (np.abs(got["normals"] - model["normals"]).max(1) / e_normal).max()
    r_vertex = (np.abs(got["vertex_normals"] - model["vertex_normals"]).max(1) / e_vertex).max()
    print(f"{name}: worst error / bound: normals {r_normal:.4f}, vertex normals {r_vertex:.4f}")
    assert r_normal <= 1.0 and r_vertex <= 1.0
    # the raw launch fills both tables; the vertex table is the gather's sum of the float32 records
    T, dev = len(f), hip_device
    normals, records = torch.full((T, 3), 7.0, device=dev), torch.full((T, 9), 7.0, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mesh_sign.face_pseudonormals_raw(on(dev, v, f32), on(dev, f, np.int64), normals, records, status)
    assert int(status.item()) == 0 and (bits(normals.cpu().numpy()) == bits(got["normals"])).all()
    rec = records.cpu().numpy()
    assert (np.abs(rec.reshape(T, 3, 3) - model["records"].reshape(T, 3, 3)).max(2) <= SM.table_bounds(v, f)[1] + np.pi * e_normal[:, None] + 4 * SM.U * np.pi).all()


def ball_mesh(device, G=12, R=0.9):
    vox = 3.0 / G
    ax = (np.arange(G) + 0.5) * vox - 1.5
    dist = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    grid = rf.VoxelGrid(on(device, (R - dist)[..., None], f32), torch.zeros((G, G, G, 3), device=device), rf.VoxelSize(vox, vox, vox),
                        density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.Identity(), expected_density_scale=1.0, tunable=False)
    return rf.extract_mesh(grid, 0.0), R, vox


def test_the_extracted_ball_is_closed_and_its_sign_is_the_analytic_one(hip_device):
    mesh, R, vox = ball_mesh(hip_device)
    topology = rf.mesh_topology(mesh)
    assert topology.closed and topology.signed_volume > 0 and mesh.faces.shape[0] > 100
    assert abs(topology.signed_volume - 4.0 / 3.0 * np.pi * R ** 3) < 0.15 * 4.0 / 3.0 * np.pi * R ** 3
    q = np.random.default_rng(12).uniform(-1.5, 1.5, size=(4096, 3)).astype(f32)
    radius = np.linalg.norm(q.astype(np.float64), axis=1)
    clear = np.abs(radius - R) > vox
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a closed mesh does not warn
        inside = rf.mesh_contains(on(hip_device, q), mesh).cpu().numpy()
        found = rf.mesh_signed_distance(on(hip_device, q), mesh, orientation="auto")
    assert clear.sum() > 2500 and (inside[clear] == (radius < R)[clear]).all()
    assert ((found.distance.cpu().numpy() < 0) == inside).all()
    assert np.abs(np.abs(found.distance.cpu().numpy()) - np.abs(radius - R))[clear].max() < vox


def test_out_of_range_ids_set_the_status_and_raise(hip_device):
    v, f, q, groups = SM.fixture("cube")
    dev = hip_device
    grid = rf.MeshSignGrid(mesh_on(dev, v, f))
    points = on(dev, q[groups["off"]], f32)
    face = grid.grid.closest(points).face
    N, T = len(points), len(f)

    def launch(faces=grid.faces, partners=grid.topology.partners, face=face):
        signed = torch.full((N,), 7.0, device=dev)
        feature = torch.full((N, 2), 7, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        mesh_sign.signed_distance_raw(grid.vertices, faces, partners, grid.vertex_normals, points, face, signed, status, feature=feature)
        return signed.cpu().numpy(), feature.cpu().numpy(), int(status.item())

    good, kinds, status = launch()
    assert status == 0 and (good != 7).all() and (kinds[:, 0] == SM.EDGE).any()
    bad_face = face.clone()
    bad_face[5] = T  # the first id past the array, in an array that is itself in bounds
    signed, _, status = launch(face=bad_face)
    assert status == 1 and signed[5] == 7 and (bits(np.delete(signed, 5)) == bits(np.delete(good, 5))).all()
    bad_partners = grid.topology.partners.clone()
    bad_partners[:] = T
    signed, _, status = launch(partners=bad_partners)
    edge = kinds[:, 0] == SM.EDGE
    assert status == 2 and (signed[edge] == 7).all() and (bits(signed[~edge]) == bits(good[~edge])).all()
    bad_faces = grid.faces.clone()
    bad_faces[:, 1] = len(v)
    signed, _, status = launch(faces=bad_faces)
    assert status == 1 and (signed == 7).all()
    grid.topology = grid.topology._replace(partners=bad_partners)
    with pytest.raises(ValueError, match="outside its array"):
        grid.signed_distance(points)
    normals, records = torch.zeros((T, 3), device=dev), torch.zeros((T, 9), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mesh_sign.face_pseudonormals_raw(grid.vertices, bad_faces, normals, records, status)
    assert int(status.item()) == 1 and not normals.any() and not records.any()


@pytest.mark.parametrize("name", ["cube", "prism"])
def test_gradients_are_the_unsigned_ones_times_the_sign(hip_device, name):
    v, f, q, groups = SM.fixture(name)
    dev = hip_device
    rows = np.concatenate([np.arange(700), np.arange(groups["off"].start, groups["off"].stop)])
    weight = on(dev, np.random.default_rng(3).uniform(0.5, 2.0, size=len(rows)), f32)

    def gradients(function, sign=None):
        points, vertices = on(dev, q[rows], f32).requires_grad_(True), on(dev, v, f32).requires_grad_(True)
        value = function(points, vertices, on(dev, f, np.int64))
        ((value if sign is None else sign * value) * weight).sum().backward()
        return value.detach(), points.grad.cpu().numpy(), vertices.grad.cpu().numpy()

    signed, gp, gv = gradients(rf.point_mesh_signed_distance)
    sign = torch.where(signed < 0, -1.0, 1.0)
    assert (sign < 0).any() and (sign > 0).any()
    unsigned, up, uv = gradients(rf.point_mesh_distance, sign)
    assert (bits(signed.cpu().numpy()) == bits((sign * unsigned).cpu().numpy())).all()
    assert (bits(signed.cpu().numpy()) == bits(result(dev, name)["distance"][rows])).all()
    assert (bits(gp) == bits(up)).all() and (bits(gv) == bits(uv)).all()
    assert (bits(gp) == bits(sign.cpu().numpy()[:, None] * gradients(rf.point_mesh_distance)[1])).all()
    assert np.abs(gv).max() > 0


BOX = ((-0.2, -0.2, -0.2), (1.2, 1.2, 1.2))


@pytest.mark.parametrize("name", ["cavity", "cube"])
def test_the_truncated_volume_is_the_exact_one_clipped(hip_device, name):
    v, f = SM.MESHES[name]()
    mesh = mesh_on(hip_device, v, f)
    exact = rf.mesh_to_sdf(mesh, *BOX, (17, 17, 17))
    truncation = 3.0 * 1.4 / 17
    cut = rf.mesh_to_sdf(mesh, *BOX, (17, 17, 17), truncation=truncation)
    e, c, known = exact.sdf.cpu().numpy(), cut.sdf.cpu().numpy(), cut.known.cpu().numpy()
    assert exact.known.all() and exact.truncation is None and np.isfinite(e).all()
    t32 = f32(truncation)
    assert (known == (np.abs(e) <= t32)).all() and 0 < (~known).sum() < known.size
    assert ((c < 0) == (e < 0)).all()
    assert (bits(c[known]) == bits(e[known])).all() and (np.abs(c[~known]) == t32).all()
    assert not known[8, 8, 8]  # the centre: the middle of the cavity (outside the solid) / of the cube (inside)
    assert (c[8, 8, 8] > 0) == (name == "cavity") and c[0, 0, 0] == t32
    # the nodes are a VoxelGrid's
    nodes = mesh_sign.node_coordinates(-0.2, 1.2, 17, hip_device).cpu().numpy()
    assert abs(nodes[8] - 0.5) < 1e-6 and abs(nodes[0] - (-0.2 + 0.7 / 17)) < 1e-6
    with pytest.raises(ValueError, match="truncation"):
        rf.mesh_to_sdf(mesh, *BOX, (17, 17, 17), truncation=1.4 * 1.4 / 17)


def test_remeshing_the_icosphere(hip_device):
    v, f = SM.icosphere()
    mesh = mesh_on(hip_device, v, f)
    low, high, G = -1.5, 1.5, 17
    volume = rf.mesh_to_sdf(mesh, (low,) * 3, (high,) * 3, (G,) * 3)
    remeshed = volume.extract_mesh()
    topology = rf.mesh_topology(remeshed)
    vox = (high - low) / G
    assert topology.closed and topology.signed_volume > 0 and abs(topology.signed_volume - SM.signed_volume(v, f)) < 0.1 * SM.signed_volume(v, f)
    distance = rf.mesh_distance(remeshed, mesh, samples=20_000)
    print(f"remeshed icosphere: {remeshed.faces.shape[0]} faces, hausdorff estimate {distance.hausdorff:.4f}, voxel diagonal {vox * 3 ** 0.5:.4f}")
    assert distance.hausdorff < vox * 3 ** 0.5
    # every vertex lies on an edge of the Kuhn tetrahedra -- node i to node i + d, d in {0, 1}^3 -- whose ends have opposite signs
    sdf = volume.sdf.cpu().numpy().astype(np.float64)
    t = (remeshed.vertices.cpu().numpy().astype(np.float64) - (low + 0.5 * vox)) / vox
    explained = np.zeros(len(t), bool)
    for d in [np.array(d) for d in np.ndindex(2, 2, 2)][1:]:
        base = np.where(d == 1, np.floor(t), np.round(t)).astype(np.int64)
        lam = t - base
        along = lam[:, d == 1]
        fits = (np.abs(lam[:, d == 0]) < 1e-3).all(1) & (np.abs(along - along[:, :1]) < 1e-3).all(1) & (along[:, 0] > -1e-3) & (along[:, 0] < 1 + 1e-3)
        inside = fits & (base >= 0).all(1) & (base + d < G).all(1)
        i, j = base[inside], base[inside] + d
        crossing = np.zeros(len(t), bool)
        crossing[inside] = (sdf[i[:, 0], i[:, 1], i[:, 2]] < 0) != (sdf[j[:, 0], j[:, 1], j[:, 2]] < 0)
        explained |= crossing
    assert explained.all(), int((~explained).sum())
    # the offset surface lies that much further out
    grown = rf.mesh_topology(volume.extract_mesh(offset=0.1))
    assert grown.closed and grown.signed_volume > topology.signed_volume


def test_signed_mesh_distance_says_which_cube_is_inside(hip_device):
    v, f = SM.cube()
    small = (0.5 + 0.9 * (v.astype(np.float64) - 0.5)).astype(f32)
    a, b = mesh_on(hip_device, v, f), mesh_on(hip_device, small, f)
    signed = rf.signed_mesh_distance(a, b, samples=5000, seed=4)
    assert signed.b_to_a.mean < 0 and signed.b_to_a.inside == 1.0 and np.isnan(signed.b_to_a.mean_outside) and signed.b_to_a.mean_inside == signed.b_to_a.mean
    assert signed.a_to_b.mean > 0 and signed.a_to_b.inside == 0.0 and np.isnan(signed.a_to_b.mean_inside)
    assert abs(signed.volume_a - 1.0) < 1e-12 and abs(signed.volume_b - 0.729) < 1e-6 and signed.samples == 5000
    plain = rf.mesh_distance(a, b, samples=5000, seed=4)
    assert abs(abs(signed.a_to_b.mean) - plain.a_to_b.mean) < 1e-12 and abs(abs(signed.b_to_a.mean) - plain.b_to_a.mean) < 1e-12
    assert abs(signed.b_to_a.mean + 0.05) < 1e-6  # every point of the small cube's surface is 0.05 under the large one's
    against = mesh_sign.signed_mean_against(b, a, samples=5000, seed=4)  # (what --distance_to_input of the scripts prints)
    assert abs(against.mean + 0.05) < 1e-6 and against.inside == 1.0
    assert mesh_sign.signed_mean_against(b, mesh_on(hip_device, v, f[1:]), samples=100) is None  # an open reference has no sign to give
    inward = rf.signed_mesh_distance(mesh_on(hip_device, v, f[:, [0, 2, 1]]), mesh_on(hip_device, small, f[:, [0, 2, 1]]), samples=5000, seed=4, orientation="auto")
    assert abs(inward.b_to_a.mean - signed.b_to_a.mean) < 1e-6 and inward.b_to_a.inside == 1.0 and inward.volume_a < 0


def test_an_open_mesh_warns_and_orientation_flips(hip_device):
    v, f, q, groups = SM.fixture("cube")
    points = on(hip_device, q[:300], f32)
    with pytest.warns(RuntimeWarning, match="not guaranteed"):
        rf.MeshSignGrid(mesh_on(hip_device, v, f[1:])).signed_distance(points)
    outward = rf.mesh_signed_distance(points, mesh_on(hip_device, v, f)).distance
    inward = rf.mesh_signed_distance(points, mesh_on(hip_device, v, f), orientation="inward").distance
    assert (bits(inward.cpu().numpy()) == bits((-outward).cpu().numpy())).all()
    limited = rf.mesh_signed_distance(points, mesh_on(hip_device, v, f), max_distance=0.1, return_features=True)
    far = limited.face.cpu().numpy() < 0
    assert far.any() and (~far).any() and np.isposinf(limited.distance.cpu().numpy()[far]).all() and (limited.feature.cpu().numpy()[far] == -1).all()
    assert (bits(limited.distance.cpu().numpy()[~far]) == bits(outward.cpu().numpy()[~far])).all()
    with pytest.raises(ValueError):
        rf.MeshSignGrid(mesh_on(hip_device, v, f), orientation="sideways")
    empty = rf.MeshSignGrid(rf.Mesh(on(hip_device, v, f32), torch.zeros((0, 3), dtype=torch.int64, device=hip_device), None, None))
    assert np.isposinf(empty.signed_distance(points).distance.cpu().numpy()).all()
