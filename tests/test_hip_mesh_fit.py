"""GPU: rf.MeshGeometryRenderer / rf.fit_mesh_to_views (rf_mesh_raster_coverage, rf_mesh_geometry_backward_pixels,
rf_mesh_geometry_backward_gather) on the smallest inputs at which they can go wrong (tests/mesh_fit_model.py CASES: one triangle in a
1 x 1, a 1 x 2 and a 5 x 7 image; silhouettes exactly through pixel centres, midpoints and quarters; a sub-pixel sliver; a quad; a closed
octahedron with culling off and on and both windings; 37 faces from 3 views of which one looks past the mesh; faces behind one another
with and without ``near``; a face that fills the frame; a vertex shared by 20 faces and a face over more than 4096 pixels, so that
both long-segment paths run).  The depth is ``render_mesh``'s bit for bit; coverage and vertex gradients lie within the bounds of
docs/mesh_fit_errors.md of the float64 model fed with the device's own face ids; both repeat their bits under every long-segment
threshold; the fits improve what they are meant to improve.

Measured on an MI355X: see docs/mesh_fit_errors.md for the worst ratios of error to bound and for the deviation of the first ten
losses of case A from the float64 model's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import mesh_fit_model as mfm
from thr3ed_atom_amd import _lib

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = _lib.MESH_FIT_LONG_SEGMENT  # 16
THRESHOLDS = (0, 1, DEFAULT - 1, DEFAULT, DEFAULT + 1, 63, 64, 65, 4096, 1 << 30)  # 0: the library's default; its neighbours; the wavefront's; all long; all short
# case A: the largest relative deviation of the first ten losses from the float64 model's measured on an MI355X was 6.987e-6
# (docs/mesh_fit_errors.md);
# the margin is 4 x that
LOSS_DEVIATION_MEASURED = 6.987e-6
LOSS_DEVIATION_MARGIN = 4.0 * LOSS_DEVIATION_MEASURED


def poses_of(case):
    return [rf.CameraPose(R, t.reshape(3, 1)) for R, t in case["views"]]


def intrinsics_of(case):
    return rf.CameraIntrinsics(case["H"], case["W"], case["focal"])


_RENDERED = {}


def rendered(name, device):
    """one renderer and one forward per case, shared by the tests: (case, renderer, vertices, depth, coverage, face ids)"""
    if name not in _RENDERED:
        case = mfm.make_case(name)
        renderer = rf.MeshGeometryRenderer(torch.from_numpy(case["faces"]).to(device), poses_of(case), intrinsics_of(case), near=case["near"], cull_backfaces=case["cull"])
        vertices = torch.from_numpy(case["vertices"]).to(device)
        depth, coverage = renderer(vertices)
        _RENDERED[name] = (case, renderer, vertices, depth, coverage, renderer.last_face_ids)
    return _RENDERED[name]


@pytest.mark.parametrize("name", mfm.CASES)
def test_forward_depth_is_render_mesh_and_coverage_lies_within_the_bound(hip_device, name):
    case, renderer, vertices, depth, coverage, face_ids = rendered(name, hip_device)
    N, H, W = len(case["views"]), case["H"], case["W"]
    assert depth.shape == coverage.shape == face_ids.shape == (N, H, W) and face_ids.dtype == torch.int32
    mesh = rf.Mesh(vertices, torch.from_numpy(case["faces"]).to(hip_device), None, None)
    for k, pose in enumerate(poses_of(case)):
        render = rf.render_mesh(mesh, pose, intrinsics_of(case), near=case["near"], cull_backfaces=case["cull"])
        assert torch.equal(depth[k], render.depth[..., 0]) and torch.equal(face_ids[k], render.face_ids), k  # bitwise
    again = renderer(vertices)
    assert torch.equal(again[0], depth) and torch.equal(again[1], coverage) and int(renderer.status.item()) == 0
    assert float(coverage.min()) >= 0.0 and float(coverage.max()) <= 1.0
    ids = face_ids.cpu().numpy()
    _, want, views = mfm.forward(case, case["vertices"].astype(np.float64), ids)
    got = coverage.cpu().numpy().astype(np.float64)
    hit = ids >= 0
    worst, skipped = 0.0, 0
    for k, view in enumerate(views):
        take = np.ones((H, W), bool) if case["exact"] else ~view["coverage_unsure"]
        skipped += int((~take).sum())
        err, bound = np.abs(got[k] - want[k]), view["coverage_bound"]
        assert (err[take] <= bound[take]).all(), (k, float((err - bound)[take].max()))
        if case["exact"]:
            assert np.array_equal(got[k], want[k])  # dyadic edge values: float32 computes the same numbers
        worst = max(worst, float((err[take & (bound > 0)] / bound[take & (bound > 0)]).max()) if (take & (bound > 0)).any() else 0.0)
        # the mask A > 0 holds every hit pixel that the rule leaves something (a hit pixel that loses a half to each of two neighbours is 0
        # by the rule itself), and nothing but hit pixels and their 4-neighbours
        assert (got[k] > 0)[hit[k] & (want[k] > bound) & take].all()
        near_hit = hit[k].copy()
        near_hit[1:] |= hit[k][:-1]; near_hit[:-1] |= hit[k][1:]; near_hit[:, 1:] |= hit[k][:, :-1]; near_hit[:, :-1] |= hit[k][:, 1:]  # noqa: E702
        assert not (got[k] > 0)[~near_hit].any()
    assert skipped <= mfm.MAX_AMBIGUOUS * N * H * W + 1
    print(f"mesh fit (forward) {name}: {int(hit.sum())} hit pixels, {sum(len(v['pairs']['a']) for v in views)} pairs, worst coverage error / bound {worst:.4f}, "
          f"{skipped} pixels skipped as ambiguous")


def backward_all_thresholds(renderer, vertices, face_ids, coverage, gD, gA):
    out = {}
    for threshold in THRESHOLDS:
        renderer.long_segment = threshold
        try:
            out[threshold] = renderer._backward(vertices, face_ids, coverage, gD, gA)
            assert torch.equal(renderer._backward(vertices, face_ids, coverage, gD, gA), out[threshold]), threshold  # two calls: equal bits
        finally:
            renderer.long_segment = 0
    return out


@pytest.mark.parametrize("name", mfm.CASES)
def test_backward_lies_within_the_bound_of_the_model_on_the_devices_face_ids(hip_device, name):
    case, renderer, vertices, depth, coverage, face_ids = rendered(name, hip_device)
    gD_np, gA_np = mfm.upstream(case)
    gD, gA = torch.from_numpy(gD_np).to(hip_device), torch.from_numpy(gA_np).to(hip_device)
    grads = backward_all_thresholds(renderer, vertices, face_ids, coverage, gD, gA)
    assert torch.equal(grads[0], grads[DEFAULT])  # 0 selects the default
    ids = face_ids.cpu().numpy()
    ref, bound, doubt, _ = mfm.backward(case, case["vertices"].astype(np.float64), ids, gD_np.astype(np.float64), gA_np.astype(np.float64))
    keep = np.ones(len(ref), bool) if case["exact"] else ~doubt
    used = np.zeros(len(ref), bool)
    if (ids >= 0).any():
        used[np.unique(case["faces"][np.unique(ids[ids >= 0])])] = True
    worst = 0.0
    for threshold, grad in grads.items():
        got = grad.cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape and np.isfinite(got).all()
        err = np.abs(got - ref)
        assert (err[keep] <= bound[keep]).all(), (threshold, float((err - bound)[keep].max()))
        assert (got[~used] == 0.0).all()  # every vertex is written, 0 for the untouched ones
        nz = keep[:, None] & (bound > 0)
        worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
    if name in ("fan20", "big-face-72x72"):
        assert not torch.equal(grads[1], grads[1 << 30])  # the two paths add in different orders: both were run
    # autograd through the Function is the raw entry point; a second backward raises
    leaf = vertices.clone().requires_grad_(True)
    d, a = renderer(leaf)
    (through,) = torch.autograd.grad([d, a], leaf, [gD, gA])
    assert torch.equal(through, grads[0])
    d, a = renderer(leaf)
    (once,) = torch.autograd.grad([d, a], leaf, [gD, gA], create_graph=True)
    with pytest.raises(RuntimeError):
        once.sum().backward()
    assert int(renderer.status.item()) == 0
    print(f"mesh fit (backward) {name}: {int(used.sum())} vertices touched, {int((~keep).sum())} skipped as ambiguous, worst gradient error / bound {worst:.4f}")


@pytest.mark.parametrize("name", ["exact-quarters"])
def test_directional_derivative_of_the_float32_forward(hip_device, name):
    """no gradcheck in float32: a central difference of the device's forward along one direction with a dyadic step that moves no
    crossing over a kink (tau 1/4 -> at most 5/16, 3/4 -> at least 11/16), against the model's gradient.  The difference shares its
    truncation error with the same difference of the float64 model; what is left is float32 rounding, bounded through the forward bounds."""
    case, renderer, vertices, _, _, face_ids = rendered(name, hip_device)
    gD_np, gA_np = mfm.upstream(case)
    gD, gA = gD_np.astype(np.float64), gA_np.astype(np.float64)
    ids = face_ids.cpu().numpy()
    start = case["vertices"].astype(np.float64)
    direction = np.array([[1.0, 0.5, 0.25], [-0.5, 1.0, -0.25], [0.25, -0.75, 0.5]])  # dyadic
    h = 2.0 ** -8  # x 4 pixels per world unit at this depth: the silhouette moves by at most 1/64 + of a pixel
    grad = mfm.backward(case, start, ids, gD, gA)[0]
    analytic = float((grad * direction).sum())

    def objective32(sign):
        moved = torch.from_numpy((start + sign * h * direction).astype(np.float32)).to(hip_device)
        d, a = renderer(moved)
        assert torch.equal(renderer.last_face_ids, face_ids)  # no pixel changes hands
        return float((gD * d.cpu().numpy().astype(np.float64)).sum() + (gA * a.cpu().numpy().astype(np.float64)).sum())

    def objective64(sign):
        d, a, views = mfm.forward(case, start + sign * h * direction, ids)
        noise = sum(float((np.abs(gA[k]) * v["coverage_bound"]).sum() + (np.abs(gD[k]) * 16 * mfm.UNIT * np.abs(v["depth"])).sum()) for k, v in enumerate(views))
        return float((gD * d).sum() + (gA * a).sum()), noise

    fd32 = (objective32(+1) - objective32(-1)) / (2 * h)
    (up, noise_up), (down, noise_down) = objective64(+1), objective64(-1)
    fd64 = (up - down) / (2 * h)
    truncation = abs(fd64 - analytic)
    print(f"mesh fit (directional derivative) {name}: analytic {analytic:.6g}, float64 difference {fd64:.6g}, float32 difference {fd32:.6g}")
    assert truncation <= 0.05 * abs(analytic)  # (the step is small enough to mean something)
    assert abs(fd32 - fd64) <= (noise_up + noise_down) / (2 * h)
    assert abs(fd32 - analytic) <= truncation + (noise_up + noise_down) / (2 * h)


def test_zero_views_zero_faces_and_views_that_miss(hip_device):
    case = mfm.make_case("patch37-24x32-v3")
    faces, vertices, intr = torch.from_numpy(case["faces"]).to(hip_device), torch.from_numpy(case["vertices"]).to(hip_device), intrinsics_of(case)
    for renderer, n in ((rf.MeshGeometryRenderer(faces, [], intr), 0), (rf.MeshGeometryRenderer(faces, poses_of(case)[2:], intr), 1), (rf.MeshGeometryRenderer(faces[:0], poses_of(case), intr), 3)):
        leaf = vertices.clone().requires_grad_(True)
        depth, coverage = renderer(leaf)
        assert depth.shape == coverage.shape == (n, 24, 32) and not bool(depth.any()) and not bool(coverage.any())
        (grad,) = torch.autograd.grad(depth.sum() + coverage.sum() + 0.0 * leaf.sum(), leaf)
        assert grad.shape == leaf.shape and not bool(grad.any())
    with pytest.raises(ValueError, match="2\\^31"):  # 9 views of 16384 x 16384 pixels: refused before anything is allocated
        rf.MeshGeometryRenderer(faces, [poses_of(case)[0]] * 9, rf.CameraIntrinsics(16384, 16384, 60.0))
    with pytest.raises(ValueError, match="HIP device"):
        rf.MeshGeometryRenderer(faces.cpu(), poses_of(case), intr)
    with pytest.raises(ValueError, match="faces index outside"):
        rf.MeshGeometryRenderer(faces.clone().index_fill_(0, torch.tensor([0], device=hip_device), vertices.shape[0]), poses_of(case), intr)(vertices)
    with pytest.raises(ValueError, match="not finite"):
        rf.MeshGeometryRenderer(faces, poses_of(case), intr)(vertices.clone().index_fill_(0, torch.tensor([0], device=hip_device), float("inf")))
    with pytest.raises(ValueError):
        rf.MeshGeometryRenderer(faces, poses_of(case), intr)(vertices.double())
    # an entry outside its rows is skipped and reported, never dereferenced
    _, renderer, verts, depth, coverage, face_ids = rendered("quad", hip_device)
    hit_pixels, offsets = renderer.hit_lists(face_ids)
    records = torch.zeros((renderer.P, 9), device=hip_device)
    bad = hit_pixels.clone()
    bad[0], bad[1] = renderer.P, -1
    grad = renderer._gather(records, bad, offsets, verts.shape[0])
    assert int(renderer.status.item()) == 1 and bool(torch.isfinite(grad).all())
    renderer.status.zero_()


# ---------------------------------------------------------------------------------------------------------------------- the fit

def make_ball(device, density_scale, iso_level):
    """the 16^3 ball of tests/test_hip_texture_fit.py (raw density 0.6 - r, so sigma = density_scale (0.6 - r)), extracted at ``iso_level`` and
    simplified to cells of 2 voxels, with poses around it"""
    G = 16
    ax = (np.arange(G, dtype=np.float32) + 0.5) / G * 2.0 - 1.0
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    dens = torch.from_numpy((0.6 - r).astype(np.float32)[..., None])
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    feat = torch.from_numpy(np.stack([4.0 * np.sin(5.0 * x + 1.0), 4.0 * np.cos(4.0 * y - z), 4.0 * np.sin(3.0 * z + 2.0 * x * y)], axis=-1).astype(np.float32))
    voxel = 2.0 / G
    grid = rf.VoxelGrid(dens.to(device), feat.to(device), rf.VoxelSize(voxel, voxel, voxel), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=density_scale, storage="split")
    mesh = rf.simplify_mesh(rf.extract_mesh(grid, iso_level, subdivisions=2), 2 * voxel)
    assert mesh.faces.shape[0] > 50 and mesh.normals is not None and mesh.colours is not None
    cfg = rf.SHVoxGridRenderConfig(num_samples_per_ray=128, camera_bounds=rf.CameraBounds(0.5, 5.0), perturb_sampled_points=False, render_num_samples_per_ray=128)
    vol_mod = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=device)
    poses = [rf.pose_spherical(yaw, pitch, 3.0) for yaw, pitch in ((0.0, -20.0), (90.0, 25.0), (180.0, -30.0), (270.0, 20.0), (45.0, -80.0), (200.0, 75.0), (135.0, 5.0))]
    return dict(grid=grid, vol_mod=vol_mod, mesh=mesh, poses=poses, voxel=voxel)


@pytest.fixture(scope="module")
def ball(hip_device):
    return make_ball(hip_device, 20.0, 1.0)


def iou(a, b):
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def test_fit_case_a_pulls_a_swollen_ball_back(hip_device, ball):
    mesh, poses, voxel = ball["mesh"], ball["poses"][:4], ball["voxel"]
    intr = rf.CameraIntrinsics(32, 32, 50.0)
    renderer = rf.MeshGeometryRenderer(mesh.faces, poses, intr)
    with torch.no_grad():
        target_depth, _ = renderer(mesh.vertices)
        target_mask = renderer.last_face_ids >= 0
    outward = mesh.vertices / mesh.vertices.norm(dim=1, keepdim=True)  # the ball sits at the origin
    swollen = mesh._replace(vertices=(mesh.vertices + 1.5 * voxel * outward).contiguous())
    iterations, seen = 60, []
    fit = rf.fit_mesh_to_views(swollen, target_depth, target_mask.float(), poses, intr, iterations=iterations, callback=lambda it, value: seen.append(it))
    assert seen == list(range(iterations)) and fit.history.shape == (iterations,) and fit.history.device.type == "cuda"
    history = fit.history.cpu().numpy().astype(np.float64)

    def score(m):
        with torch.no_grad():
            renderer(m.vertices)
            return iou((renderer.last_face_ids >= 0).cpu().numpy(), target_mask.cpu().numpy()), float((m.vertices - mesh.vertices).norm(dim=1).mean())

    (iou0, dist0), (iou1, dist1) = score(swollen), score(fit.mesh)
    print(f"mesh fit (case A): loss {history[0]:.6g} -> {history[9]:.6g} -> {history[-1]:.6g}; mask IoU {iou0:.4f} -> {iou1:.4f}; mean vertex distance to the original "
          f"{dist0:.5f} -> {dist1:.5f} ({dist0 / voxel:.2f} -> {dist1 / voxel:.2f} voxels)")
    assert history[-1] < history[0] and iou1 > iou0 and dist1 < dist0  # strict improvements
    assert torch.equal(fit.mesh.faces, mesh.faces) and fit.mesh.colours is mesh.colours and fit.mesh.normals.shape == mesh.normals.shape
    assert torch.allclose(fit.moved, (fit.mesh.vertices - swollen.vertices).norm(dim=1))
    # the first ten losses against the float64 model's Adam run (its own rasteriser, its own adjoint, its own Adam)
    case = dict(faces=mesh.faces.cpu().numpy(), views=[(np.asarray(p.rotation, np.float32).reshape(3, 3), np.asarray(p.translation, np.float32).reshape(3)) for p in poses],
                H=32, W=32, focal=50.0, near=0.0, cull=False)
    edges = mfm.edge_list(case["faces"])
    start = swollen.vertices.cpu().numpy().astype(np.float64)
    lr = rf.mesh_fit.DEFAULT_LR_FRACTION * float(np.float32(np.linalg.norm(start[edges[:, 0]] - start[edges[:, 1]], axis=1).mean()))
    model, _ = mfm.adam_fit(case, start, target_depth.cpu().numpy(), target_mask.float().cpu().numpy(), 10, lr, laplacian_weight=rf.mesh_fit.DEFAULT_LAPLACIAN_WEIGHT)
    deviation = float(np.abs(history[:10] / model - 1.0).max())
    print(f"mesh fit (case A): the first ten losses deviate from the float64 model's by up to {deviation:.3e} (relative; margin {LOSS_DEVIATION_MARGIN:.3e})")
    assert deviation <= LOSS_DEVIATION_MARGIN
    again = rf.fit_mesh_to_views(swollen, target_depth, target_mask.float(), poses, intr, iterations=iterations)
    assert torch.equal(again.mesh.vertices, fit.mesh.vertices) and torch.equal(again.history, fit.history)  # bitwise


def held_out_scores(ball, mesh, intr):
    scores = rf.evaluate_mesh_against_field(mesh, None, ball["vol_mod"], ball["poses"][4:], intr)
    return scores["mask_iou"], scores["depth_l1"]


def test_fit_case_b_against_a_field(hip_device, ball):
    """``fit_mesh_to_field_views`` on the small ball field, sigma = 20 (0.6 - r), meshed at iso 1 (r = 0.55) and simplified; 4 poses fit, 3
    others score.  On this fuzzy ball the two targets are two surfaces: the accumulated weight passes 1/2 on the chord at distance
    0.514 from the centre (20 x the chord integral of 0.6 - r = ln 2), 0.28 voxel inside the mesh, and the median depth of a central ray
    lies where 10 x^2 = ln 2, x = 0.263 inside r = 0.6: r = 0.337, 1.7 voxels inside the mesh.  Both lie INSIDE the mesh, so a vertex that
    moves inward by less than the nearer of the two gaps improves both scores; ``max_move`` is the parameter that says so, and the
    test passes a quarter of a voxel.  (Left free to move 2 voxels the fit follows the depth term past the alpha silhouette: held-out
    depth L1 0.250 -> 0.107 but mask IoU 0.871 -> 0.783, measured on an MI355X at a step of 0.02 x the edge length)"""
    mesh, vol_mod, voxel = ball["mesh"], ball["vol_mod"], ball["voxel"]
    intr = rf.CameraIntrinsics(48, 64, 60.0)
    iou0, depth0 = held_out_scores(ball, mesh, intr)
    fit = rf.fit_mesh_to_field_views(mesh, vol_mod, ball["poses"][:4], intr, iterations=60, max_move=0.25 * voxel)
    iou1, depth1 = held_out_scores(ball, fit.mesh, intr)
    history = fit.history.cpu().numpy()
    print(f"mesh fit (case B): loss {history[0]:.6g} -> {history[-1]:.6g}; on held-out poses mask IoU {iou0:.4f} -> {iou1:.4f}, depth L1 {depth0:.5f} -> {depth1:.5f} "
          f"({depth1 / voxel:.3f} voxels), vertices moved {float(fit.moved.mean()) / voxel:.3f} voxels on average, at most {float(fit.moved.max()) / voxel:.3f}")
    assert iou1 > iou0 and depth1 < depth0  # strict improvements
    assert float(fit.moved.max()) <= 0.25 * voxel * (1 + 1e-5)  # max_move holds for every vertex
    assert torch.equal(fit.mesh.faces, mesh.faces) and fit.mesh.normals is not None


def test_fit_on_a_crisp_ball_meshed_one_voxel_too_deep(hip_device):
    """beside case B: a ball with a crisp surface (sigma = 400 (0.6 - r): half the opacity within half a voxel of r = 0.6, so that median
    depth and accumulated weight describe ONE surface) whose mesh was extracted at an iso level of 50, one voxel inside it (r = 0.475);
    here the vertices may move 2 voxels, and have to move outward"""
    ball = make_ball(hip_device, 400.0, 50.0)
    mesh, voxel = ball["mesh"], ball["voxel"]
    intr = rf.CameraIntrinsics(48, 64, 60.0)
    iou0, depth0 = held_out_scores(ball, mesh, intr)
    fit = rf.fit_mesh_to_field_views(mesh, ball["vol_mod"], ball["poses"][:4], intr, iterations=60, max_move=2 * voxel)
    iou1, depth1 = held_out_scores(ball, fit.mesh, intr)
    print(f"mesh fit (crisp ball): on held-out poses mask IoU {iou0:.4f} -> {iou1:.4f}, depth L1 {depth0:.5f} -> {depth1:.5f} ({depth1 / voxel:.3f} voxels), "
          f"farthest vertex moved {float(fit.moved.max()) / voxel:.3f} voxels")
    assert iou1 > iou0 and depth1 < depth0
    assert float(fit.moved.max()) <= 2 * voxel * (1 + 1e-5)


def test_iterations_zero_max_move_and_argument_errors(hip_device, ball):
    mesh, poses = ball["mesh"], ball["poses"][:2]
    intr = rf.CameraIntrinsics(24, 32, 40.0)
    depths, alphas = torch.full((2, 24, 32), 2.5, device=hip_device), torch.ones((2, 24, 32), device=hip_device)
    none = rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, iterations=0)
    assert none.mesh is mesh and none.history.shape == (0,) and not bool(none.moved.any())
    tight = rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, iterations=5, lr=0.05, max_move=0.01)
    moved = (tight.mesh.vertices - mesh.vertices).norm(dim=1)
    assert float(moved.max()) <= 0.01 * (1 + 1e-5) and float(moved.max()) > 0.005 and torch.equal(tight.mesh.faces, mesh.faces)
    bare = rf.fit_mesh_to_views(mesh._replace(normals=None, colours=None), [depths[0], depths[1]], alphas[..., None], poses, intr, iterations=1)
    assert bare.mesh.normals is None and bare.mesh.colours is None
    for kwargs in (dict(iterations=-1), dict(iterations=1.5), dict(lr=0.0), dict(lr=float("nan")), dict(max_move=0.0), dict(max_move=float("inf")), dict(depth_weight=-1.0),
                   dict(mask_weight=float("nan")), dict(laplacian_weight=-0.1), dict(near=-0.5)):
        with pytest.raises(ValueError):
            rf.fit_mesh_to_views(mesh, depths, alphas, poses, intr, **{"iterations": 1, **kwargs})
    for d, a, p in ((depths[:1], alphas, poses), (depths, alphas[:1], poses), (depths, alphas, poses[:1]), (depths[:, :-1], alphas, poses), (depths, alphas[:, :, :-1], poses)):
        with pytest.raises(ValueError):
            rf.fit_mesh_to_views(mesh, d, a, p, intr, iterations=1)
    with pytest.raises(ValueError, match="HIP device"):
        rf.fit_mesh_to_views(rf.Mesh(mesh.vertices.cpu(), mesh.faces.cpu(), None, None), depths, alphas, poses, intr, iterations=1)


# ------------------------------------------------------------------------------------------------------------------ the script

def test_the_fit_mesh_script_end_to_end(hip_device, tmp_path):
    """one run of scripts/fit_mesh.py on the reference checkpoint fixture, in a fresh process under its own time limit"""
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    checkpoint = os.path.join(REPO_ROOT, "tests", "golden", "reference_checkpoint.pth")
    small = tmp_path / "small.ply"
    r = subprocess.run([sys.executable, "scripts/extract_mesh_from_sh_based_voxel_grid.py", "-i", checkpoint, "-o", str(small), "--target_faces", "200",
                        "--geometry_fit_iterations", "2", "--geometry_fit_views", "3"], cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "geometry: fitted to 3 views of the field, loss " in r.stdout and " in 2 iterations" in r.stdout and small.exists()
    fitted = tmp_path / "fitted.ply"
    r = subprocess.run([sys.executable, "scripts/fit_mesh.py", "-i", checkpoint, "--mesh", str(small), "-o", str(fitted), "--views", "3", "--iterations", "4", "--view_height", "48",
                        "--view_width", "64", "--view_focal", "60"], cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "mesh fit: loss " in r.stdout and " in 4 iterations over 3 views" in r.stdout and fitted.exists()
    from thr3ed_atom_amd.mesh import read_ply

    assert np.array_equal(read_ply(str(fitted))[3], read_ply(str(small))[3])  # the faces are the input's
