"""The float64 model of rf_resample_grid / rf_node_bounds (tests/resample_model.py) against what it must restate, and the CPU
fallbacks of thr3ed_atom_amd.resampling against the model.  No GPU."""
import io

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import resample_model as rm
from tests.helpers import hash_uniform, procedural_grid
from thr3ed_atom_amd.resampling import resample_map, tightened_dims

MODES = ["relu", "softplus", "abs", "identity"]
ACTIVATIONS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
               "abs": (torch.abs, torch.nn.Identity()), "identity": (torch.nn.Identity(), torch.nn.Identity())}
STORAGES = ["reference", "split", "bricked"]
# float32 evaluation of an 8-term weighted sum with weights summing to 1: <= 3 roundings per weight + 8 of the accumulation
F32_SUM = 16 * 2.0**-24


def make_grid(dens, feat, voxel, location=(0.0, 0.0, 0.0), mode="relu", storage="reference", rho=2.0, tunable=False):
    return rf.VoxelGrid(dens.clone(), feat.clone(), rf.VoxelSize(*voxel), rf.VoxelGridLocation(*location), density_preactivation=ACTIVATIONS[mode][0],
                        density_postactivation=ACTIVATIONS[mode][1], expected_density_scale=rho, tunable=tunable, storage=storage)


@pytest.mark.parametrize("dims", [(5, 6, 7), (9, 8, 17)], ids=lambda d: "x".join(map(str, d)))
def test_model_crop_is_array_slicing(dims):
    dens, feat = (t.numpy() for t in procedural_grid(dims, 12, 3))
    off, out = (1, 2, 3), (3, 4, 4)
    d, f = rm.resample(dens, feat, out, (1.0, 1.0, 1.0), off)
    sl = tuple(slice(o, o + n) for o, n in zip(off, out))
    assert np.array_equal(d, dens[sl].astype(np.float64)) and np.array_equal(f, feat[sl].astype(np.float64))
    # an offset that pushes part of the destination outside: (fill, 0) there, the slice elsewhere
    d, f = rm.resample(dens, feat, dims, (1.0, 1.0, 1.0), (-2.0, 0.0, 3.0), fill=-7.0)
    out_mask = rm.outside_mask(dims, dims, (1.0, 1.0, 1.0), (-2.0, 0.0, 3.0))
    expect = np.zeros(dims, dtype=bool)
    expect[:2] = True
    expect[:, :, dims[2] - 3:] = True
    assert np.array_equal(out_mask, expect)
    assert (d[out_mask] == -7.0).all() and (f[out_mask] == 0.0).all()
    assert np.array_equal(d[2:, :, : dims[2] - 3], dens[: dims[0] - 2, :, 3:].astype(np.float64))


@pytest.mark.parametrize("src,dst", [((5, 6, 7), (10, 12, 14)), ((4, 4, 8), (16, 8, 8)), ((5, 6, 7), (8, 9, 11)), ((9, 8, 17), (5, 8, 6))], ids=str)
def test_model_at_the_upsample_parameters_agrees_with_the_oracle(src, dst):
    """scale = n_src / n_dst, offset = scale / 2 - 1 / 2 restates F.interpolate(trilinear, align_corners=False); the oracle is
    float32 ATen, hence 1e-6 of the volume's largest value and not less"""
    dens, feat = procedural_grid(src, 12, 5)
    vol = torch.cat([feat, dens], dim=-1)
    ref = orc.trilinear_upsample(vol, dst).numpy().astype(np.float64)
    scale = [np.float32(s) / np.float32(d) for s, d in zip(src, dst)]
    offset = [0.5 * float(sc) - 0.5 for sc in scale]
    d, f = rm.resample(dens.numpy(), feat.numpy(), dst, scale, offset)
    err = max(np.abs(f - ref[..., :-1]).max(), np.abs(d - ref[..., -1:]).max())
    print(f"model vs F.interpolate {src} -> {dst}: max abs {err:.3e}")
    assert err <= 1e-6 * float(vol.abs().max())


def test_bounds_model_on_crafted_volumes():
    dims = (5, 6, 7)
    for mode in MODES:
        empty_value = {"relu": -1.0, "softplus": -30.0, "abs": 0.0, "identity": -1.0}[mode]
        thr = 1e-6 if mode == "softplus" else 0.0
        d = np.full(dims, empty_value, dtype=np.float32)
        assert rm.node_bounds(d, 2.0, mode, thr) is None
        d[4, 0, 6] = 1.0  # a single node, in a corner
        assert rm.node_bounds(d, 2.0, mode, thr) == ((4, 0, 6), (4, 0, 6), 1)
        assert rm.node_bounds(d, 2.0, mode, 2.5) is None and rm.node_bounds(d, 2.0, mode, 1.5) is not None  # sigma = rho * D = 2 (softplus: 2.13)
        # a node on each face
        d[...] = empty_value
        faces = [(0, 2, 3), (4, 3, 3), (2, 0, 3), (2, 5, 2), (1, 2, 0), (3, 3, 6)]
        for k in range(6):
            d[faces[k]] = 0.75
            lo, hi, n = rm.node_bounds(d, 2.0, mode, thr)
            pts = np.array(faces[: k + 1])
            assert lo == tuple(pts.min(0)) and hi == tuple(pts.max(0)) and n == k + 1
        assert (lo, hi) == ((0, 0, 0), (4, 5, 6))
    # |.| passes negative densities, identity and ReLU do not; strictness at the threshold
    d = np.zeros(dims, dtype=np.float32)
    d[1, 1, 1] = -0.5
    assert rm.node_bounds(d, 1.0, "abs", 0.0) == ((1, 1, 1), (1, 1, 1), 1)
    assert rm.node_bounds(d, 1.0, "relu", 0.0) is None and rm.node_bounds(d, 1.0, "identity", 0.0) is None
    assert rm.node_bounds(d, 1.0, "abs", 0.5) is None
    assert rm.merge_bounds([5, 6, 7, -1, -1, -1], None) == [5, 6, 7, -1, -1, -1]
    assert rm.merge_bounds([2, 0, 3, 2, 4, 3], ((1, 1, 1), (1, 1, 1), 1)) == [1, 0, 1, 2, 4, 3]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", MODES)
def test_cpu_content_bounds_equals_the_model(mode, storage):
    dims = (9, 8, 17)
    dens, feat = procedural_grid(dims, 3, 9)
    u = hash_uniform(dims, 10, 0.0, 1.0)
    dens = torch.where(torch.from_numpy(u)[..., None] > 0.97, dens.abs() + 0.1, -dens.abs() - 0.1 if mode != "abs" else torch.zeros_like(dens))
    dens[0] = dens[0].clamp_max(-0.1) if mode != "abs" else 0.0  # the x = 0 face holds nothing
    if mode == "softplus":
        dens = dens * 10.0
    for thr in ((0.5,) if mode == "softplus" else (0.0, 0.5)):
        grid = make_grid(dens, feat, (0.1, 0.2, 0.3), mode=mode, storage=storage)
        want = rm.node_bounds(dens.numpy(), 2.0, mode, thr)
        assert want is not None and want[0][0] > 0 and want[2] < int(np.prod(dims))
        assert rf.content_bounds(grid, thr) == want
    assert rf.content_bounds(make_grid(torch.full_like(dens, -30.0 if mode != "abs" else 0.0), feat, (1, 1, 1), mode=mode, storage=storage), 0.25) is None
    if mode == "softplus":
        with pytest.raises(ValueError):
            rf.content_bounds(grid, 0.0)
    with pytest.raises(ValueError):
        rf.content_bounds(grid, float("nan"))


@pytest.mark.parametrize("storage", STORAGES)
def test_cpu_crop_and_resample_equal_the_model(storage):
    dims, F = (9, 8, 17), 12
    dens, feat = procedural_grid(dims, F, 13)
    voxel, loc = (0.25, 0.5, 0.125), (1.0, -2.0, 0.5)
    grid = make_grid(dens, feat, voxel, loc, storage=storage, tunable=True)
    crop = rf.crop_voxel_grid(grid, (2, 1, 8), (5, 6, 12), margin=2)
    assert crop.grid_dims == (8, 8, 9) and crop.storage == storage and tuple(crop.voxel_size) == voxel  # y is clipped to the grid
    assert torch.equal(crop.densities.detach(), dens[0:8, 0:8, 6:15]) and torch.equal(crop.features.detach(), feat[0:8, 0:8, 6:15])
    assert crop.get_config_dict()["tunable"] and crop.expected_density_scale == 2.0 and crop.density_mode == "relu"
    assert rf.crop_voxel_grid(grid, (0, 0, 0), (8, 7, 16), margin=0).grid_dims == dims
    with pytest.raises(ValueError):
        rf.crop_voxel_grid(grid, (5, 0, 0), (4, 7, 16), margin=0)
    # the general re-grid: a finer lattice that sticks out of the source box on one side
    new_voxel, new_loc, new_dims = (0.1, 0.3, 0.1), (1.2, -2.0, 1.0), (11, 9, 14)
    got = rf.resample_voxel_grid(grid, new_loc, new_voxel, new_dims, fill_density=-3.0)
    scale, offset = resample_map(grid.aabb, voxel, new_loc, new_voxel, new_dims)
    d64, f64, (sd, sf) = rm.resample(dens.numpy(), feat.numpy(), new_dims, scale, offset, fill=-3.0, return_slope=True)
    out = rm.outside_mask(new_dims, dims, scale, offset)
    assert out.any() and not out.all()
    # float32 evaluation + one float32 rounding of s (<= 2^-24 n) times the slope
    bound = lambda slope: F32_SUM * 1.0 + slope * 2.0**-23 * max(dims)  # noqa: E731  (|values| < 1)
    assert (np.abs(got.densities.detach().numpy() - d64) <= bound(sd)).all() and (np.abs(got.features.detach().numpy() - f64) <= bound(sf)).all()
    assert (got.densities.detach().numpy()[out] == -3.0).all() and (got.features.detach().numpy()[out] == 0.0).all()
    assert got.grid_dims == new_dims and tuple(got.voxel_size) == new_voxel and tuple(got.get_config_dict()["grid_location"]) == new_loc
    # the map itself, against the definition in float64
    for a in range(3):
        lo_src, lo_dst = loc[a] - dims[a] * voxel[a] / 2, new_loc[a] - new_dims[a] * new_voxel[a] / 2
        assert scale[a] == float(np.float32(new_voxel[a] / voxel[a]))
        assert offset[a] == float(np.float32((lo_dst - lo_src) / voxel[a] + 0.5 * new_voxel[a] / voxel[a] - 0.5))
    # softplus must name its fill
    soft = make_grid(dens, feat, voxel, loc, mode="softplus", storage=storage)
    with pytest.raises(ValueError):
        rf.resample_voxel_grid(soft, new_loc, new_voxel, new_dims)


def test_the_grid_location_formula_keeps_node_world_positions():
    dims = (9, 8, 17)
    dens, feat = procedural_grid(dims, 3, 17)
    voxel, loc = (0.3, 0.7, 0.11), (0.37, -1.9, 2.3)
    grid = make_grid(dens, feat, voxel, loc)
    old = rm.node_world_positions(grid.aabb, dims)
    for lo, hi, margin in (((2, 1, 8), (5, 6, 12), 1), ((0, 0, 0), (0, 0, 0), 0), ((8, 7, 16), (8, 7, 16), 3), ((3, 3, 3), (4, 4, 4), 0)):
        crop = rf.crop_voxel_grid(grid, lo, hi, margin)
        new = rm.node_world_positions(crop.aabb, crop.grid_dims)
        for a in range(3):
            first = max(lo[a] - margin, 0)
            assert crop.grid_dims[a] == min(hi[a] + margin, dims[a] - 1) - first + 1
            # float64 throughout: a few ulp of the box coordinates, 1e-9 of a voxel at most
            assert np.abs(new[a] - old[a][first: first + crop.grid_dims[a]]).max() <= 1e-12 * max(1.0, abs(loc[a]) + dims[a] * voxel[a])
        assert torch.equal(crop.densities, dens[tuple(slice(max(l - margin, 0), min(h + margin, n - 1) + 1) for l, h, n in zip(lo, hi, dims))])


@pytest.mark.parametrize("storage", STORAGES)
def test_cpu_tighten_follows_the_rule_and_keeps_an_empty_field(storage):
    dims = (16, 16, 16)
    dens, feat = procedural_grid(dims, 3, 21)
    dens = -dens.abs() - 0.01
    dens[5:11, 4:9, 6:8] = 0.5
    grid = make_grid(dens, feat, (0.25, 0.25, 0.25), (0.5, 0.0, -0.5), storage=storage)
    plain, stats = rf.tighten_voxel_grid(grid, 0.0, margin=1)
    assert stats.passing_nodes == 6 * 5 * 2 and stats.old_dims == dims and stats.new_dims == (8, 7, 4) == plain.grid_dims
    assert torch.equal(plain.densities, dens[4:12, 3:10, 5:9]) and stats.new_aabb == plain.aabb and stats.old_aabb == grid.aabb
    for (lo, hi), (olo, ohi) in zip(plain.aabb, grid.aabb):
        assert olo <= lo < hi <= ohi
    budget = 16**3
    tight, stats = rf.tighten_voxel_grid(grid, 0.0, margin=1, num_nodes=budget)
    extent = [8 * 0.25, 7 * 0.25, 4 * 0.25]
    edge = (extent[0] * extent[1] * extent[2] / budget) ** (1 / 3)
    want = tuple(max(2, int(np.floor(e / edge + 0.5))) for e in extent)
    assert tight.grid_dims == want == stats.new_dims == tightened_dims((8, 7, 4), (0.25,) * 3, budget)
    # within the rounding of the rule: every axis moves by at most half a voxel
    assert np.prod([(n - 0.5) for n in want]) <= budget <= np.prod([(n + 0.5) for n in want])
    for (lo, hi), (plo, phi) in zip(tight.aabb, plain.aabb):
        assert abs(lo - plo) <= 1e-12 and abs(hi - phi) <= 1e-12  # the resampling keeps the cropped box
    up = orc.trilinear_upsample(torch.cat([plain.features, plain.densities], dim=-1), want)
    assert torch.allclose(tight.densities, up[..., -1:], atol=1e-6) and torch.allclose(tight.features, up[..., :-1], atol=1e-6)
    assert tightened_dims((100, 1, 1), (1.0, 1.0, 1.0), 8) == (43, 2, 2)  # edge = cbrt(100 / 8) = 2.32; thin axes keep two nodes
    empty = make_grid(-dens.abs(), feat, (0.25,) * 3, storage=storage)
    same, stats = rf.tighten_voxel_grid(empty, 0.0, num_nodes=budget)
    assert same is empty and stats.passing_nodes == 0 and stats.new_dims == dims and stats.new_aabb == empty.aabb


@pytest.mark.parametrize("storage", STORAGES)
def test_a_cropped_grid_survives_the_checkpoint_round_trip(storage):
    dims = (9, 8, 17)
    dens, feat = procedural_grid(dims, 12, 23)
    grid = make_grid(dens, feat, (0.25, 0.5, 0.125), (1.0, -2.0, 0.5), storage=storage, tunable=True)
    crop = rf.crop_voxel_grid(grid, (2, 1, 8), (5, 6, 12), margin=1)
    cfg = rf.SHVoxGridRenderConfig(16, rf.CameraBounds(1.0, 5.0))
    model = rf.VolumetricModel(crop, rf.render_sh_voxel_grid, cfg, device=torch.device("cpu"))
    blob = io.BytesIO()
    torch.save(model.get_save_info(), blob)
    blob.seek(0)
    back = rf.create_voxel_grid_from_saved_info_dict(torch.load(blob, weights_only=False), storage=storage)
    assert back.grid_dims == crop.grid_dims and back.aabb == crop.aabb and tuple(back.voxel_size) == tuple(crop.voxel_size)
    assert tuple(back.get_config_dict()["grid_location"]) == tuple(crop.get_config_dict()["grid_location"])
    assert torch.equal(back.densities.detach(), crop.densities.detach()) and torch.equal(back.features.detach(), crop.features.detach())
    assert back.density_mode == "relu" and back.expected_density_scale == 2.0
