"""tests/mesh_distance_grad_model.py against what it has to restate (no GPU needed): central float64 differences of the float64
brute-force distance for queries and corners, the closed forms of the contract exactly, the envelope identity in every region, the
rejection of two broken models, and the float64 fit of an icosphere to a scaled and shifted copy."""
import numpy as np
import pytest

from tests import mesh_distance_grad_model as GM
from tests import mesh_distance_model as M

f32, f64 = np.float32, np.float64
H = 1e-6  # the step of the central differences
# name: (mesh, queries, the seed of the queries -- chosen so that at most 5 % of them change face or region within the stencil)
CASES = {
    "triangle": (GM.TRIANGLE, 60, 1),
    "cube": (M.cube(), 60, 1),
    "icosphere": (M.icosphere(), 40, 1),
    "perturbed": ((M.perturbed(M.icosphere()[0]), M.icosphere()[1]), 40, 1),
}


def case_queries(name, count, seed):
    """generic positions: the box of the small meshes grown by 30 %; off the surface of the fine ones, where a query far from the
    surface sees an edge that two faces share and the last bit decides which of them wins"""
    (v, f), _, _ = CASES[name]
    return GM.box_queries(v, count, seed, margin=0.3) if len(f) < 100 else GM.offset_queries(v, f, count, seed)


def finite_differences(v, f, q, variant=None):
    """(kept [N] bool, worst error / tolerance over the kept queries' 3 + 9 derivatives)"""
    v64 = v.astype(f64)
    d, face, region = GM.winners(q, v64, f)
    brute = M.brute_force(q, v64, f)  # the existing model's brute force: the reference distance is not this model's own
    assert (d == brute[0]).all() and (face == brute[1]).all()
    model = GM.query_gradients(q, v64, f, face, np.ones(len(q)), f64, variant=variant)
    kept, worst = np.ones(len(q), bool), 0.0
    for i, p in enumerate(q.astype(f64)):
        tolerance = 1e-8 + 10.0 * (H / max(d[i], 1e-30)) ** 2
        errors = []
        for j in range(3):
            step = np.zeros(3)
            step[j] = H
            (dp, fp, rp), (dm, fm, rm) = GM.winners(p + step, v64, f), GM.winners(p - step, v64, f)
            kept[i] &= fp[0] == face[i] and fm[0] == face[i] and rp[0] == region[i] and rm[0] == region[i]
            errors.append(abs((dp[0] - dm[0]) / (2 * H) - model["grad_points"][i, j]))
        for k in range(3):
            for j in range(3):
                out = []
                for sign in (1.0, -1.0):
                    moved = v64.copy()
                    moved[f[face[i], k], j] += sign * H
                    out.append(GM.winners(p, moved, f))
                kept[i] &= all(o[1][0] == face[i] and o[2][0] == region[i] for o in out)
                # the face's OTHER corners that name the same vertex move with it: the model's records of those corners add up
                same = [kk for kk in range(3) if f[face[i], kk] == f[face[i], k]]
                errors.append(abs((out[0][0][0] - out[1][0][0]) / (2 * H) - sum(model["records"][i, 3 * kk + j] for kk in same)))
        if kept[i]:
            worst = max(worst, max(errors) / tolerance)
    return kept, worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_float64_model_is_the_derivative_of_the_brute_force_distance(name):
    (v, f), count, seed = CASES[name]
    q = case_queries(name, count, seed)
    kept, worst = finite_differences(v, f, q)
    print(f"{name}: {int((~kept).sum())} of {count} queries left out, worst error / tolerance {worst:.3g}")
    assert (~kept).sum() <= 0.05 * count
    assert worst <= 1.0


def test_the_comparison_can_fail():
    (v, f), count, seed = CASES["cube"]
    q = GM.box_queries(v, count, seed, margin=0.3)
    for variant in ("corner order", "q for r"):
        kept, worst = finite_differences(v, f, q, variant)
        assert kept.any() and worst > 1e3, variant


@pytest.mark.parametrize("dtype", [f32, f64])
def test_closed_forms_exactly(dtype):
    v, f = GM.TRIANGLE
    a, b, c = v[0], v[1], v[2]
    q = np.array([[1, 1, 2], [2, -3, 0], [-1, -1, 0], [1, 1, 0]], dtype=dtype)
    G = np.array([1, 1, 1, 3], dtype=dtype)
    out = GM.gradients(q, a, b, c, G, dtype)
    assert out["beta"].dtype == dtype and out["records"].dtype == dtype
    assert out["region"].tolist()[:2] == [3, 0] and out["region"][3] == 3
    assert out["beta"][0].tolist() == [0.5, 0.25, 0.25] and out["u"][0].tolist() == [0, 0, 1]
    assert out["beta"][1].tolist() == [0.5, 0.5, 0] and out["u"][1].tolist() == [0, -1, 0]
    assert out["beta"][2].tolist() == [1, 0, 0] and np.allclose(out["u"][2], [-np.sqrt(0.5), -np.sqrt(0.5), 0], atol=1e-7)
    assert (out["u"][3] == 0).all() and (out["grad_points"][3] == 0).all() and (out["records"][3] == 0).all()  # on the surface: the subgradient 0
    assert out["records"][0].tolist() == [0, 0, -0.5, 0, 0, -0.25, 0, 0, -0.25] and out["grad_points"][0].tolist() == [0, 0, 1]
    assert out["records"][1].tolist() == [0, 0.5, 0, 0, 0.5, 0, 0, 0, 0]
    # a face (a, a, a): its point; a face with a zero-length edge (a, a, c): the segment a c
    p = np.array([[3, 4, 0]], dtype=dtype)
    point = GM.gradients(p, a, a, a, np.ones(1, dtype), dtype)
    assert point["region"][0] == 0 and point["beta"][0].tolist() == [1, 0, 0] and point["d2"][0] == 25
    assert np.isfinite(point["records"]).all() and point["u"][0].tolist() == [dtype(3) / dtype(5), dtype(4) / dtype(5), 0]
    edge = GM.gradients(np.array([[-1, 2, 0]], dtype=dtype), a, a, c, np.ones(1, dtype), dtype)
    assert np.isfinite(edge["records"]).all() and edge["d2"][0] == 1 and edge["q"][0].tolist() == [0, 2, 0] and edge["u"][0].tolist() == [-1, 0, 0]
    assert edge["region"][0] in (1, 2) and edge["beta"][0, 2] == 0.5 and edge["beta"][0].sum() == 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_envelope_identity_in_every_region(name):
    """the beta sum to 1 and sum_k beta_k corner_k = q, in float64 to rounding and in float32 within the derived bounds"""
    (v, f), _, seed = CASES[name]
    q = np.concatenate([case_queries(name, 300, seed + 100), GM.box_queries(v, 100, seed + 100, margin=0.5)])
    _, face, _ = GM.winners(q, v, f, f32)
    ones = np.ones(len(q))
    m32, m64 = GM.query_gradients(q, v, f, face, ones.astype(f32), f32), None
    m64 = GM.query_gradients(q, v, f, face, ones, f64, region=m32["region"])
    corners = v.astype(f64)[f[face]]
    if name != "icosphere":  # (from inside or near a fine convex mesh every query sees a face's interior)
        assert set(m32["region"].tolist()) == {0, 1, 2, 3}
    else:
        assert 3 in set(m32["region"].tolist())
    for m, tolerance in ((m64, 1e-12), (m32, None)):
        beta = m["beta"].astype(f64)
        length = np.sqrt(m64["d2"])
        e_u, e_beta, _, _ = GM.bounds(q, v, f, face, m32["region"], ones, length, m64["beta"])
        reach = np.abs(corners).max(axis=(1, 2))
        slack = 3 * e_beta + 4 * GM.U if tolerance is None else tolerance
        assert (np.abs(beta.sum(1) - 1) <= slack).all()
        rebuilt = (beta[:, :, None] * corners).sum(1)
        position = np.array([M.face_bounds(q[i], v, f[face[i]][None])[0, 0] for i in range(len(q))]) if tolerance is None else 1e-12
        assert (np.abs(rebuilt - m["q"].astype(f64)).max(axis=1) <= 3 * reach * slack + position).all()
    # and the float32 model against the float64 one under the same face and region, within the bounds
    assert (np.abs(m32["u"].astype(f64) - m64["u"]).max(axis=1) <= e_u).all()
    assert (np.abs(m32["beta"].astype(f64) - m64["beta"]).max(axis=1) <= e_beta).all()


def test_the_two_sums_in_the_gathers_order_against_a_plain_scatter():
    v, f, q = GM.fan()
    _, face, _ = GM.winners(q, v, f, f32)
    assert (face == 0).all() and len(q) == 40
    records = GM.query_gradients(q, v, f, face, np.ones(len(q), f32), f32)["records"]
    total, magnitude, count = GM.vertex_sums64(records, face, f, len(v))
    assert count[0] == 40 + 20  # the records that reach the apex and its corner slots
    for threshold in (4, 16):
        got = GM.vertex_sums32(records, face, f, len(v), threshold)
        assert got.dtype == f32 and (np.abs(got.astype(f64) - total) <= GM.sum_bound(count, magnitude)).all()


def test_the_fit_lowers_its_loss():
    v, f, tv = GM.sphere_pair()
    picked, bary, _ = GM.draws(v, f, 512, seed=1)
    _, _, target_points = GM.draws(tv, f, 512, seed=2)
    fitted, history = GM.fit(v, f, picked, bary, tv, f, target_points, iterations=30)
    print(f"float64 fit of an icosphere to its copy scaled by 1.2 and shifted by 0.1: loss {history[0]:.6g} -> {history[-1]:.6g}, ratio {history[-1] / history[0]:.4f}")
    assert history[-1] < history[0]
    # the model's gradient is the derivative of the model's loss
    loss = lambda x: GM.chamfer(x, f, picked, bary, tv, f, target_points)[0]  # noqa: E731
    _, grad = GM.chamfer(v.astype(f64), f, picked, bary, tv, f, target_points)
    rng = np.random.default_rng(0)
    direction = rng.normal(size=v.shape)
    numeric = (loss(v.astype(f64) + H * direction) - loss(v.astype(f64) - H * direction)) / (2 * H)
    assert abs(numeric - (grad * direction).sum()) <= 1e-6 * max(abs(numeric), 1.0)
