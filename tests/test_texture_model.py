"""CPU: the atlas layout of thr3ed_atom_amd/texture.py against its float64 restatement (tests/texture_model.py), the properties the
layout promises (one owner per texel, bilinear footprints inside the owner, the UV round trip), closed forms of the baked value, and
proof that the GPU comparison of tests/test_hip_texture.py can fail: two wrong models differ from the model by more than the bound
on that test's inputs."""
import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import texture_model as tm
from tests.helpers import hash_uniform
from thr3ed_atom_amd import texture as tx

C0 = 0.28209479177387814


def test_the_public_names_exist():
    assert rf.bake_texture is tx.bake_texture and rf.write_obj is tx.write_obj and rf.TextureBake is tx.TextureBake
    assert rf.TextureBake._fields == ("texture", "opacity", "uvs", "patch", "block", "cols", "rows")


@pytest.mark.parametrize("T,P,cols", [(0, 8, None), (1, 2, None), (2, 3, None), (7, 8, None), (7, 3, 3), (7, 8, 5), (33, 17, None), (10, 64, 1)])
def test_library_layout_equals_the_model(T, P, cols):
    lay, ref = tx.atlas_layout(T, P, cols), tm.layout(T, P, cols)
    assert (lay.patch, lay.block, lay.cols, lay.rows, lay.width, lay.height) == (ref["patch"], ref["block"], ref["cols"], ref["rows"], ref["width"], ref["height"])
    uv = tx.corner_uvs(lay, T)
    assert uv.dtype == np.float32 and uv.shape == (T, 3, 2)
    assert np.array_equal(uv, tm.uvs(T, P, cols).astype(np.float32))
    if T:
        assert (uv > 0).all() and (uv < 1).all()


def test_layout_errors():
    for bad in (1, 65, 0, -3, 2.5, True):
        with pytest.raises(ValueError):
            tx.atlas_layout(4, bad)
    with pytest.raises(ValueError):
        tx.atlas_layout(4, 8, cols=0)
    with pytest.raises(ValueError):
        tx.atlas_layout(2 * 1366 * 1366, 8)  # 1366 blocks of 12 texels: 16392 > 16384
    assert tx.atlas_layout(2 * 1365 * 1365, 8).width == 16380
    with pytest.raises(ValueError):
        tx.atlas_layout(100, 8, cols=1400)
    mesh = rf.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), None, None)
    with pytest.raises(ValueError, match="HIP device"):
        rf.bake_texture(mesh, None)


@pytest.mark.parametrize("P", [2, 3, 8, 17])
def test_every_texel_has_one_owner_and_footprints_stay_inside_it(P):
    B = P + 4
    owner = tm.block_owner(P)
    assert owner.shape == (B, B) and set(np.unique(owner)) == {0, 1}
    # the owner of (i, j) is the rule of the contract
    for j in range(B):
        for i in range(B):
            assert owner[j, i] == (1 if i + j > P + 3 else 0)
    table = tm.texel_table(2, P)
    assert (table["face"] >= 0).all() and ((table["face"] == 0) == (owner == 0)).all()
    odd = tm.texel_table(1, P)
    assert ((odd["face"] == -1) == (owner == 1)).all()  # T odd: the upper half of the last block has no owner
    # bilinear footprints of interior, edge and corner points of both patches
    r = hash_uniform((64, 2), 5 + P, 0.0, 1.0).astype(np.float64)
    bary = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    bary += [(1 - t, t, 0.0) for t in r[:16, 0]] + [(1 - t, 0.0, t) for t in r[16:32, 0]] + [(0.0, 1 - t, t) for t in r[32:48, 0]]
    bary += [(1 - b, a, b - a) for a, b in np.sort(r, axis=1)]  # interior
    for upper in (False, True):
        corners = tm.patch_corners(P, upper)
        for beta in bary:
            x, y = np.asarray(beta) @ corners  # texel-centre coordinates inside the block
            u, v = (x + 0.5) / B, 1.0 - (y + 0.5) / B
            for cx, cy, w in tm.bilinear_footprint(u, v, B, B):
                if abs(w) <= 1e-12:
                    continue  # (a tap without weight fetches nothing)
                assert 0 <= cx < B and 0 <= cy < B, (P, upper, beta)
                assert owner[int(cy), int(cx)] == int(upper), (P, upper, beta, cx, cy)


@pytest.mark.parametrize("T,P,cols", [(7, 2, None), (7, 3, 3), (5, 8, None), (4, 17, 1)])
def test_uv_round_trip_returns_the_point_of_the_face(T, P, cols):
    """bilinear fetch of the texel-point image at the UV of a barycentric point of a face = that face's 3-D point"""
    vertices = hash_uniform((3 * T, 3), 77 + P).astype(np.float64) * 2.0
    faces = np.arange(3 * T).reshape(T, 3)
    table = tm.texel_table(T, P, cols)
    points = tm.texel_points(vertices, faces, table)
    lay = table["layout"]
    uv = tm.uvs(T, P, cols)
    r = np.sort(hash_uniform((40, 2), 9 + T, 0.0, 1.0).astype(np.float64), axis=1)
    betas = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.0), (0.0, 0.5, 0.5)] + [(1 - b, a, b - a) for a, b in r]
    scale = np.abs(vertices).max()
    for t in range(T):
        for beta in betas:
            beta = np.asarray(beta)
            u, v = beta @ uv[t]
            want = beta @ vertices[faces[t]]
            got = np.zeros(3)
            for cx, cy, w in tm.bilinear_footprint(u, v, lay["width"], lay["height"]):
                if abs(w) <= 1e-12:
                    continue
                assert table["face"][int(cy), int(cx)] == t
                got += w * points[int(cy), int(cx)]
            assert np.abs(got - want).max() <= 1e-12 * scale, (t, beta)


def _constant_grid(dims, F, density, feature_values):
    dens = np.full((*dims, 1), density, np.float32)
    feat = np.broadcast_to(np.asarray(feature_values, np.float32), (*dims, F)).copy()
    return dens, feat


def _inside_triangle(aabb, scale=0.15):
    centre = np.array([(lo + hi) / 2 for lo, hi in aabb])
    return (centre + scale * np.array([[-1.0, -0.6, 0.2], [0.9, -0.4, -0.3], [0.1, 0.8, 0.4]])).astype(np.float32), np.array([[0, 1, 2]])


def test_closed_forms():
    dims, voxel = (12, 12, 12), (0.2, 0.2, 0.2)
    aabb = orc.make_aabb(dims, voxel)
    vertices, faces = _inside_triangle(aabb)
    # constant features: every owned texel is the colour of the constant, whatever the density (the points stay far inside the box,
    # where the zero padding does not reach)
    for degree, diffuse in ((0, False), (2, False), (3, True)):
        K = (degree + 1) ** 2
        values = hash_uniform((3 * K,), 31 + degree)
        dens = hash_uniform((*dims, 1), 3)
        feat = np.broadcast_to(values, (*dims, 3 * K)).copy()
        out = tm.bake(dens, feat, aabb, 3.0, "relu", vertices, faces, 8, 0.4, 16, diffuse=diffuse)
        e1, e2 = vertices[1].astype(np.float64) - vertices[0], vertices[2].astype(np.float64) - vertices[0]
        n = np.cross(e1, e2)
        n /= np.linalg.norm(n)
        coeff = torch.as_tensor(values.astype(np.float64)).reshape(1, 3, K)
        raw = coeff[..., 0] * C0 if diffuse else orc.evaluate_sh(degree, coeff, torch.as_tensor(-n)[None])
        want = torch.sigmoid(raw).numpy()[0]
        assert out["owned"].sum() > 0 and np.abs(out["texture"][out["owned"]] - want).max() <= 1e-12
        assert (out["texture"][~out["owned"]] == 0).all() and (out["opacity"][~out["owned"]] == 0).all()
    # constant density under the identity mode: opacity = 1 - exp(-2 reach sigma0)
    dens, feat = _constant_grid(dims, 3, 0.7, hash_uniform((3,), 4))
    for S in (1, 5, 16):
        out = tm.bake(dens, feat, aabb, 2.5, "identity", vertices, faces, 3, 0.3, S)
        assert np.abs(out["opacity"][out["owned"]] - (1 - np.exp(-2 * float(np.float32(0.3)) * float(np.float32(0.7)) * 2.5))).max() <= 1e-12
    # reach = 0 is c(p); a zero-area triangle bakes c(p) too (n = 0: every sample sits on p, and the weights sum against the background)
    dens, feat = hash_uniform((*dims, 1), 8), hash_uniform((*dims, 27), 9)
    out = tm.bake(dens, feat, aabb, 3.0, "relu", vertices, faces, 8, 0.0, 16)
    table = tm.texel_table(1, 8)
    p = tm.texel_points(vertices, faces, table)[out["owned"]]
    n = np.cross(vertices[1].astype(np.float64) - vertices[0], vertices[2].astype(np.float64) - vertices[0])
    n /= np.linalg.norm(n)
    cp, _, _ = tm.field_colour(feat, aabb, p, np.repeat(-n[None], len(p), 0), False)
    assert np.array_equal(out["texture"][out["owned"]], cp) and (out["opacity"] == 0).all()
    flat_faces = np.array([[0, 0, 2]])
    out = tm.bake(dens, feat, aabb, 3.0, "relu", vertices, flat_faces, 8, 0.4, 16)
    p = tm.texel_points(vertices, flat_faces, table)[out["owned"]]
    cp, _, _ = tm.field_colour(feat, aabb, p, np.zeros_like(p), False)
    assert np.abs(out["texture"][out["owned"]] - cp).max() <= 1e-12


def test_the_model_of_the_gpu_cases_stays_under_half_a_step_and_away_from_the_planes():
    kinds = set()
    for case in tm.CASES:
        made = tm.make_case(case)
        out = tm.bake_case(made)
        owned = out["owned"]
        assert owned.any() and not out["near_boundary"].any(), tm.case_id(case)
        assert out["bound"][owned].max() < tm.HALF_STEP and out["bound"][owned].min() > 0, (tm.case_id(case), out["bound"].max())
        assert (out["bound"][~owned] == 0).all()
        kinds |= {case[0], f"sh{case[1]}", case[2], f"diffuse{case[3]}", f"T{case[4]}", f"P{case[5]}", f"S{case[6]}", f"r{case[7]}"}
    assert {"reference", "split", "bricked", "sh0", "sh1", "sh2", "sh3", "relu", "softplus", "abs", "identity", "diffuseTrue", "diffuseFalse",
            "T1", "T2", "T3", "T7", "P2", "P3", "P8", "S1", "S5", "S16", "r0.0", "r0.5", "r3.0"} <= kinds
    assert any(case[8] is not None and -(-case[4] // 2) % case[8] for case in tm.CASES)  # a cols that leaves the last row partly empty


def test_the_comparison_can_fail():
    """d = +n and an ownership split at P + 2 differ from the model by more than the bound the GPU test uses, on its inputs"""
    flipped = split = 0
    for case in tm.CASES:
        made = tm.make_case(case)
        out = tm.bake_case(made)
        bound = out["bound"].max()
        if case[1] > 0 and not case[3]:  # the direction enters with SH degree >= 1 of a specular bake
            wrong = tm.bake_case(made, wrong="plus_normal")
            excess = (np.abs(wrong["texture"] - out["texture"]).max(-1) > out["bound"])[out["owned"]]
            assert excess.any(), tm.case_id(case)
            assert np.abs(wrong["texture"] - out["texture"]).max() > 10 * bound
            flipped += 1
        wrong = tm.bake_case(made, wrong="split_p2")
        moved = wrong["owned"] != out["owned"]
        diff = np.abs(wrong["texture"] - out["texture"]).max(-1)
        if case[4] % 2 == 1:
            assert moved.any(), tm.case_id(case)  # T odd: the anti-diagonal of the last block loses its owner
        if (diff > out["bound"]).any():
            assert diff.max() > 10 * bound
            split += 1
    assert flipped >= 6 and split >= 12
