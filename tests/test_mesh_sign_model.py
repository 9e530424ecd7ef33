"""The sign rule of docs/mesh_sign_errors.md against a truth that shares nothing with it, and ``rf.mesh_topology`` (no GPU needed): on
the cube (A), the cube with a cavity (B), the icosphere (C) and the L-shaped prism with a reflex edge and a thin spike (D) the float64
pseudonormal rule gives the sign of the float64 generalised winding number at EVERY query farther from the surface than the forward's
distance bound; the plane normal of the winning face alone does not (D shows it); and the random queries are a fair input -- at most 1 %
of them have an |s| under the decision margin, so the GPU test cannot hide behind the margin."""
import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_sign_model as SM

NAMES = sorted(SM.MESHES)


def mesh_of(v, f):
    return rf.Mesh(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f)), None, None)


@pytest.mark.parametrize("name", NAMES)
def test_the_fixtures_are_closed_and_wound_outward(name):
    v, f, q, groups = SM.fixture(name)
    assert len(f) == {"cube": 12, "cavity": 24, "icosphere": 320, "prism": 28}[name]
    partner = SM.partners(f)
    assert (partner >= 0).all() and (partner[partner, :] == np.arange(len(f))[:, None, None]).any(-1).all()
    expected = {"cube": 1.0, "cavity": 1.0 - 0.125, "prism": 3.0 + 0.05 ** 2 * 1.0 / 3.0}.get(name)
    volume = SM.signed_volume(v, f)
    assert volume > 0 and (expected is None or abs(volume - expected) < 1e-6)
    assert groups["random"].stop == 4096 and len(q) == 4096 + 3 * (len(v) + len(f) + 3 * len(f) // 2)


@pytest.mark.parametrize("name", NAMES)
def test_the_float64_rule_gives_the_winding_numbers_sign(name):
    ref = SM.reference(name)
    clear = ref["distance"] > ref["B"]
    assert clear.sum() > 4096  # (the on-surface queries are the ones left out)
    rule = np.where(ref["result"]["signed"] < 0, -1, 1)
    assert (rule[clear] == ref["truth"][clear]).all(), np.nonzero(clear & (rule != ref["truth"]))[0][:10]
    # the winding number is an integer away from the surface: the truth is not a near call
    w = SM.winding_number(SM.fixture(name)[2], *SM.fixture(name)[:2])[clear]
    assert np.abs(w - np.round(w)).max() < 1e-6 and set(np.round(w).astype(int)) <= {0, 1}


def test_the_plane_normal_of_the_winning_face_is_not_enough():
    v, f, q, _ = SM.fixture("prism")
    ref = SM.reference("prism")
    clear = ref["distance"] > ref["B"]
    wrong = clear & (SM.plane_sign(q, v, f, ref["face"]) != ref["truth"])
    assert wrong.sum() >= 1
    assert (ref["result"]["kind"][wrong] != SM.FACE).all()  # they are queries whose closest point is an edge or a vertex


def test_every_feature_kind_occurs_with_both_signs():
    seen = {name: {(int(k), int(s)) for k, s in zip(SM.reference(name)["result"]["kind"], np.where(SM.reference(name)["result"]["signed"] < 0, -1, 1))} for name in NAMES}
    everything = {(k, s) for k in (SM.FACE, SM.EDGE, SM.VERTEX) for s in (-1, 1)}
    assert set.union(*seen.values()) == everything
    assert seen["cavity"] == everything  # a concave corner: a vertex that is closest from inside the solid
    assert {(SM.EDGE, -1), (SM.EDGE, 1)} <= seen["prism"]  # the reflex edge


@pytest.mark.parametrize("name", NAMES)
def test_few_random_queries_lie_under_the_decision_margin(name):
    ref, groups = SM.reference(name), SM.fixture(name)[3]
    s, margin = np.abs(ref["result"]["s"][groups["random"]]), ref["margin"][groups["random"]]
    assert np.isfinite(margin).all() and (margin > 0).all()
    share = float((s <= margin).mean())
    print(f"{name}: {share:.4%} of the random queries under the margin; largest margin {margin.max():.3g}, median |s| {np.median(s):.3g}")
    assert share <= 0.01


@pytest.mark.parametrize("name", NAMES)
def test_the_float32_model_names_the_float64_models_features_away_from_ties(name):
    """the two forms of the model agree wherever nothing is decided by the last bit: the random queries"""
    v, f, q, groups = SM.fixture(name)
    ref = SM.reference(name)
    rows = groups["random"]
    d32, face32 = SM.brute(q[rows], v, f, np.float32)
    single = SM.signed_distance(q[rows], v, f, face32, np.float32)
    same = face32 == ref["face"][rows]
    assert same.mean() > 0.9
    assert (single["kind"][same] == ref["result"]["kind"][rows][same]).mean() > 0.99
    decided = np.abs(ref["result"]["s"][rows]) > ref["margin"][rows]
    assert ((single["signed"] < 0) == (ref["result"]["signed"][rows] < 0))[decided].all()


def test_topology_of_the_cube():
    v, f = SM.cube()
    t = rf.mesh_topology(mesh_of(v, f))
    assert t.closed and (t.boundary_edges, t.nonmanifold_edges, t.inconsistent_edges, t.degenerate_faces) == (0, 0, 0, 0)
    assert abs(t.signed_volume - 1.0) <= 1e-12
    assert t.partners.dtype == torch.int32 and tuple(t.partners.shape) == (12, 3)


@pytest.mark.parametrize("name", NAMES)
def test_partners_are_symmetric_and_the_models(name):
    v, f, _, _ = SM.fixture(name)
    t = rf.mesh_topology(mesh_of(v, f))
    partner = t.partners.numpy()
    assert (partner == SM.partners(f)).all() and t.closed
    for face in range(len(f)):
        for k in range(3):
            assert face in partner[partner[face, k]]
    assert abs(t.signed_volume - SM.signed_volume(v, f)) < 1e-12


def test_topology_counts_what_is_wrong_with_a_mesh():
    v, f = SM.cube()
    opened = rf.mesh_topology(mesh_of(v, f[1:]))
    assert not opened.closed and opened.boundary_edges == 3 and (opened.partners == -1).sum() == 3
    flipped = f.copy()
    flipped[0] = flipped[0][[0, 2, 1]]
    turned = rf.mesh_topology(mesh_of(v, flipped))
    assert not turned.closed and turned.inconsistent_edges == 3 and (turned.partners == -3).sum() == 6 and turned.boundary_edges == 0
    assert (turned.partners.numpy() == SM.partners(flipped)).all()
    fin_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)
    fin_f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)
    fin = rf.mesh_topology(mesh_of(fin_v, fin_f))
    assert not fin.closed and fin.nonmanifold_edges == 1 and (fin.partners == -2).sum() == 3 and fin.boundary_edges == 6
    assert (fin.partners.numpy() == SM.partners(fin_f)).all()
    flat = rf.mesh_topology(mesh_of(fin_v, np.array([[0, 1, 1], [0, 1, 2]], dtype=np.int64)))
    assert flat.degenerate_faces == 1
    empty = rf.mesh_topology(mesh_of(fin_v, np.zeros((0, 3), np.int64)))
    assert not empty.closed and tuple(empty.partners.shape) == (0, 3) and empty.signed_volume == 0.0
    with pytest.raises(ValueError):
        rf.mesh_topology(mesh_of(fin_v, np.array([[0, 1, 5]], dtype=np.int64)))
    with pytest.raises(ValueError):
        rf.mesh_topology(mesh_of(fin_v, np.array([[0, 1, -1]], dtype=np.int64)))


def test_propagated_signs_fill_every_unknown_node():
    from thr3ed_atom_amd import mesh_sign

    rng = np.random.default_rng(5)
    centre = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1) - 4.0
    inside = np.linalg.norm(centre, axis=-1) < 2.6
    sign = np.where(inside, -1, 1).astype(np.int8)
    boundary = np.zeros_like(inside)
    for axis in range(3):  # known: every node with a neighbour of the other sign
        for shift in (-1, 1):
            moved = np.roll(inside, shift, axis)
            edge = np.ones_like(inside)
            index = [slice(None)] * 3
            index[axis] = 0 if shift == 1 else -1
            edge[tuple(index)] = False
            boundary |= (moved != inside) & edge
    keep = boundary | (rng.uniform(size=inside.shape) < 0.02)
    filled = mesh_sign.propagate_signs(torch.from_numpy(np.where(keep, sign, 0).astype(np.int8)))
    assert (filled.numpy() == sign).all()
    nothing = mesh_sign.propagate_signs(torch.zeros((3, 4, 5), dtype=torch.int8))
    assert (nothing == 0).all()
