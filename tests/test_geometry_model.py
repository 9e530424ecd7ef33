"""The float64 model of rf_render_geometry (tests/geometry_model.py) on the CPU: its weights against the oracle, its normals against
an analytic field, the conditions of the kernel comparison's case table (tests/test_hip_geometry.py), and that the comparison can
fail.  No GPU: the argument validation goes through the library, which returns every error before any device access."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import relu_field_oracle as orc
from tests import geometry_model as gm
from tests import node_weights_model as nm
from thr3ed_atom_amd import _lib

CASES = gm.kernel_cases()


def test_the_case_table_meets_every_value_of_every_factor():
    for col, values in ((0, gm.DIMS), (1, gm.STORAGES), (2, gm.SAMPLES), (3, gm.FEATURES), (4, gm.MODES), (5, gm.OPTIONS)):
        assert {c[col] for c in CASES} == set(values), col
    assert len(set(CASES)) == len(CASES) == len(gm.DIMS) * len(gm.STORAGES) * len(gm.SAMPLES)


def test_the_rays_of_the_table_miss_the_box_and_start_inside_it():
    for dims in gm.DIMS:
        aabb = orc.make_aabb(dims, gm.voxel_of(dims))
        for option in ("plain", "camera"):
            o, d, near, far = gm.case_rays(dims, 65, option)
            assert o.shape == d.shape == (gm.RAYS, 3)
            _, _, inside, _ = nm.sample_geometry(o, d, aabb, near, far, 65)
            miss = (~inside.any(-1)).float().mean()
            assert 0.15 <= float(miss) <= 0.40, (dims, option, float(miss))
            if option == "plain":  # the origins of the last 8 rays lie inside the box
                assert bool(orc.inside_aabb(o[88:], aabb).all()) and not bool(orc.inside_aabb(o[:88], aabb).any())


MODEL_CASES = sorted({(dims, S, F, mode, option) for dims, _, S, F, mode, option in CASES})  # (the storage does not enter the model)


@pytest.mark.parametrize("dims,S,F,mode,option", MODEL_CASES, ids=gm.case_id)
def test_sum_of_weights_equals_the_oracle_accumulated_weight(dims, S, F, mode, option):
    """the model's sum_i w_i against the accumulated weight of the oracle's own render (relu_field_oracle.render: its sampler,
    interpolation, activation and accumulation in float32), per ray, on every case of the table"""
    dens, feat = gm.blob_grid(dims, F, mode)
    o, d, near, far = gm.case_rays(dims, S, option)
    ref = gm.case_reference(dims, F, mode, S, option)
    out = orc.render(dens, feat, o, d, orc.make_aabb(dims, gm.voxel_of(dims)), near, far, S, gm.rho_of(mode), mode,
                     optimized_sampling=(option == "aabb"), t_rand=gm.case_jitter(S, option))
    acc = out["acc"].numpy()[:, 0].astype(np.float64)
    assert np.isfinite(acc).all() and acc.max() > 0.5
    assert np.abs(ref["acc"] - acc).max() <= gm.TOL, np.abs(ref["acc"] - acc).max()


def test_normals_of_a_linear_field_are_the_analytic_unit_vector():
    """D = a x + b y + c z + d in INDEX space: every sample whose 8 corners are nodes has n_i = -(a sx, b sy, c sz) / |.| with
    s = dims * norm_scale / 2, to 1e-12"""
    dims = (5, 6, 7)
    a, b, c, d0 = 0.7, -0.4, 0.25, 0.3
    ix, iy, iz = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij")
    dens = torch.from_numpy((a * ix + b * iy + c * iz + d0)[..., None])
    aabb = orc.make_aabb(dims, gm.voxel_of(dims))
    o, d, near, far = gm.case_rays(dims, 65, "plain")
    _, pts, inside, _ = nm.sample_geometry(o, d, aabb, near, far, 65)
    p = pts.reshape(-1, 3)
    g, _ = gm.gradient_terms(dens, aabb, 1.0, "identity", p)
    i0, _, _ = gm.cell_geometry(p, aabb, dims)
    interior = inside.reshape(-1).numpy() & np.all([(i0[k] >= 0) & (i0[k] + 1 < dims[k]) for k in range(3)], axis=0)
    assert interior.sum() > 500
    consts = orc.normalisation_constants(aabb)
    want = np.array([a, b, c]) * np.array([dims[k] * float(consts[k][0]) / 2.0 for k in range(3)])
    want = -want / np.linalg.norm(want)
    assert np.abs(gm.unit_normals(g)[interior] - want).max() <= 1e-12


def test_mirrored_densities_flip_the_composited_normal():
    """the field mirrored in all three axes, seen by the mirrored rays: N64 changes sign, acc stays"""
    dims, S = (5, 6, 7), 65
    dens, _ = gm.blob_grid(dims, 3, "relu")
    aabb = orc.make_aabb(dims, gm.voxel_of(dims))
    o, d, near, far = gm.case_rays(dims, S, "plain")
    one = gm.model(dens, aabb, gm.rho_of("relu"), "relu", o, d, near, far, S)
    two = gm.model(torch.flip(dens, (0, 1, 2)), aabb, gm.rho_of("relu"), "relu", -o, -d, near, far, S)
    assert np.abs(one["normal"]).max() > 0.5
    assert np.abs(one["normal"] + two["normal"]).max() <= 1e-9 and np.abs(one["acc"] - two["acc"]).max() <= 1e-9


@pytest.mark.parametrize("dims,S,F,mode,option", MODEL_CASES, ids=gm.case_id)
def test_float32_evaluation_stays_within_the_bound(dims, S, F, mode, option):
    """the kernel's formulas in float32 numpy against N64 at bound_r, on EVERY ray of EVERY case of the table; the model is finite"""
    ref = gm.case_reference(dims, F, mode, S, option)
    dens, _ = gm.blob_grid(dims, F, mode)
    o, d, near, far = gm.case_rays(dims, S, option)
    N32, acc32 = gm.emulate_float32(dens, orc.make_aabb(dims, gm.voxel_of(dims)), gm.rho_of(mode), mode, o, d, near, far, S,
                                    optimized_sampling=(option == "aabb"), t_rand=gm.case_jitter(S, option))
    for name in ("acc", "normal", "bound", "depth"):
        assert np.isfinite(ref[name]).all(), name
    err = np.abs(N32.astype(np.float64) - ref["normal"]).max(-1)
    print(f"{gm.case_id(dims)} S={S} {mode} {option}: max |N32 - N64| / bound = {(err / ref['bound']).max():.3f}, max bound {ref['bound'].max():.2e}")
    assert (err <= ref["bound"]).all(), float((err / ref["bound"]).max())
    assert np.abs(acc32 - ref["acc"]).max() <= gm.TOL


def test_exclusion_caps_hold_on_the_model_alone():
    """Over the case table: the rays whose bound exceeds BOUND_CAP are at most 2 % of the rays with acc64 > 0.01, the rays whose
    quantile crossing lies within QUANTILE_BAND of a sample's opacity at most 1 % of the rays -- per quantile the GPU tests use.  The
    sets are the MODEL's: what the kernel gives does not enter.  The statistic is not vacuous in any case."""
    loose = heavy = ambiguous = rays = 0
    for dims, storage, S, F, mode, option in CASES:
        ref = gm.case_reference(dims, F, mode, S, option)
        loose += int(((ref["bound"] > gm.BOUND_CAP) & (ref["acc"] > 0.01)).sum())
        heavy += int((ref["acc"] > 0.01).sum())
        ambiguous += int(ref["ambiguous"].sum())
        rays += gm.RAYS
        assert (np.linalg.norm(ref["normal"], axis=-1) > 0.5).any() and (ref["depth"] != 0).any(), (dims, S, mode, option)
    print(f"{loose} of {heavy} weighted rays above the bound cap, {ambiguous} of {rays} rays with an ambiguous crossing")
    assert loose <= 0.02 * heavy and ambiguous <= 0.01 * rays


@pytest.mark.parametrize("wrong", ["unnormalised", "plus_gradient", "drop_transmittance"])
def test_wrong_models_exceed_the_bound(wrong):
    """the comparison can fail: each wrong model leaves the bound on some ray of a case of the table"""
    dims, F, mode, S, option = (9, 10, 17), 27, "relu", 65, "plain"
    ref = gm.case_reference(dims, F, mode, S, option)
    dens, _ = gm.blob_grid(dims, F, mode)
    o, d, near, far = gm.case_rays(dims, S, option)
    bad = gm.model(dens, orc.make_aabb(dims, gm.voxel_of(dims)), gm.rho_of(mode), mode, o, d, near, far, S, wrong=wrong)
    err = np.abs(bad["normal"] - ref["normal"]).max(-1)
    tight = ref["bound"] <= gm.BOUND_CAP
    assert (err[tight] > ref["bound"][tight]).any()


def test_binding_declares_the_entry_point():
    assert "rf_render_geometry" in _lib.EXPORTED_SYMBOLS and _lib.ABI_STRUCTS[10] is _lib.RFGeometryOut
    lib = _lib.load()
    assert lib.rf_render_geometry.restype is C.c_int and lib.rf_abi_version() == 4
    assert lib.rf_abi_struct_size(10) == C.sizeof(_lib.RFGeometryOut) == 3 * C.sizeof(C.c_void_p)


def test_argument_errors_come_back_before_any_device_access():
    """every code of the contract, on a machine without a GPU; the non-NULL pointers are the small integers the neighbouring tests
    use and are never dereferenced"""
    lib = _lib.load()
    g, r, out = _lib.RFGrid(), _lib.RFRayBatch(), _lib.RFGeometryOut()
    call = lambda g_, r_, out_, flags=0, q=0.5: lib.rf_render_geometry(g_, r_, flags, q, out_, None)  # noqa: E731
    out.normal_dev = out.quantile_depth_dev = out.acc_dev = 0x6000
    assert call(None, C.byref(r), C.byref(out)) == -1
    assert call(C.byref(g), C.byref(r), C.byref(out)) == -1  # null grid tensors
    g.densities_dev, g.features_dev = 16, 16
    g.dims[0], g.dims[1], g.dims[2] = 4, 4, 4
    g.num_features, g.density_stride, g.feature_stride = 3, 1, 3
    assert call(C.byref(g), None, C.byref(out)) == -1
    assert call(C.byref(g), C.byref(r), C.byref(out)) == -2  # num_samples < 1
    r.num_rays, r.num_samples = 8, 16
    assert call(C.byref(g), C.byref(r), C.byref(out)) == -1  # rays without t_vals / origins
    r.t_vals_dev = r.origins_dev = r.directions_dev = 64
    assert call(C.byref(g), C.byref(r), None) == -1
    empty = _lib.RFGeometryOut()
    assert call(C.byref(g), C.byref(r), C.byref(empty)) == -1  # all three outputs NULL
    for q in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert call(C.byref(g), C.byref(r), C.byref(out), q=q) == -2, q
    assert call(C.byref(g), C.byref(r), C.byref(out), flags=_lib.FLAG_OCCUPANCY_SKIP) == -1  # the flag without a mask
    g.num_features, g.feature_stride = 5, 5
    assert call(C.byref(g), C.byref(r), C.byref(out)) == -3  # F = 5 is no SH degree
    g.num_features, g.feature_stride, g.density_mode = 3, 3, 7
    assert call(C.byref(g), C.byref(r), C.byref(out)) == -3  # no such density mode
    g.density_mode = 0
    r.num_rays = 0
    assert call(C.byref(g), C.byref(r), C.byref(out)) == 0  # zero rays: a no-op
    one = _lib.RFGeometryOut()
    one.acc_dev = 0x6000
    assert call(C.byref(g), C.byref(r), C.byref(one), flags=_lib.FLAG_WHITE_BKGD | _lib.FLAG_RENDER_DIFFUSE) == 0  # one output is enough


def test_host_layer_rejects_bad_arguments_without_a_gpu():
    import thr3ed_atom_amd as rf

    grid = rf.VoxelGrid(torch.zeros(2, 2, 2, 1), torch.zeros(2, 2, 2, 3), rf.VoxelSize(1, 1, 1))
    rays = rf.Rays(torch.zeros(3, 3), torch.ones(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rf.render_geometry(grid, rays, 4, (0.5, 4.0))
    for q in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="quantile"):
            rf.render_geometry(grid, rays, 4, (0.5, 4.0), quantile=q)
    cfg = rf.SHVoxGridRenderConfig(4, rf.CameraBounds(0.5, 4.0), perturb_sampled_points=False)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="Unknown render configuration field"):
        model.render_geometry(rf.pose_spherical(0.0, -30.0, 4.0), rf.CameraIntrinsics(4, 4, 4.0), no_such_field=1)
    assert rf.constants.EXTRA_NORMALS == "normals" and rf.constants.EXTRA_QUANTILE_DEPTH == "quantile_depth"


def test_point_cloud_ply_has_no_face_element(tmp_path):
    import thr3ed_atom_amd as rf

    pts = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    path = str(tmp_path / "cloud.ply")
    rf.write_point_cloud_ply(pts, torch.ones(5, 3), torch.full((5, 3), 0.5), path)
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii")
    assert "element vertex 5\n" in header and "element face" not in header
    vdt = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    assert len(data) - end == 5 * vdt.itemsize
    vert = np.frombuffer(data, vdt, count=5, offset=end)
    assert np.array_equal(vert["p"], pts.numpy()) and (vert["n"] == 1).all() and (vert["c"] == 127).all()
