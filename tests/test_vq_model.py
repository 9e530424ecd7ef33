"""Vector quantisation without a GPU: the assignment bound of tests/vq_model.py holds for a float32 restatement of the expansion form
and fails for random assignments (so the GPU test can fail), the partition by importance shares at its edges, and the compact
container: bit packing with a ragged tail, bytes round trip, decompression, and a compact checkpoint through the ordinary loader."""
import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from tests import vq_model as vm
from thr3ed_atom_amd import compression
from thr3ed_atom_amd.constants import COMPRESSED_STATE, CONFIG_DICT, STATE_DICT, THRE3D_REPR

M, C = 600, 512


@pytest.mark.parametrize("D", [3, 27, 48])
@pytest.mark.parametrize("kind", vm.INPUT_KINDS)
def test_the_float32_expansion_form_satisfies_the_bound_on_every_row(kind, D):
    x, c = vm.make_inputs(kind, M, C, D, 100 + D)
    index = vm.expansion_assign_f32(x, c)
    excess = vm.assignment_excess(x, c, index)
    print(f"{kind} D={D}: worst excess {excess.max():.3f} E; differs from the float64 argmin on {(index != vm.sq_distances(x, c).argmin(1)).mean():.1%} of rows")
    assert (excess <= 1.0).all()
    if kind == "duplicated":
        assert (index < C // 2).all()  # equal values: the lower twin


@pytest.mark.parametrize("D", [3, 27, 48])
@pytest.mark.parametrize("kind", vm.CENTRED_KINDS)
def test_random_assignments_violate_the_bound(kind, D):
    x, c = vm.make_inputs(kind, M, C, D, 200 + D)
    index = np.random.default_rng(7).integers(0, C, M)
    assert (~vm.assignment_ok(x, c, index)).mean() >= 0.95


def test_partition_edge_cases():
    rng = np.random.default_rng(3)
    imp = rng.uniform(0.1, 1.0, 101).astype(np.float32)
    for fn in (vm.partition_by_shares, compression.partition_by_shares):
        assert (fn(np.zeros(17, np.float32), 0.001, 0.6) == vm.PRUNED).all()
        assert (fn(imp, 0.0, 1.0) == vm.KEPT).all()
        assert (fn(imp, 0.0, 0.0) == vm.QUANTISED).all() and not (fn(imp, 0.3, 0.0) == vm.KEPT).any()
        # zero importance is pruned even at prune_share 0
        with_zeros = imp.copy()
        with_zeros[::5] = 0.0
        assert ((fn(with_zeros, 0.0, 1.0) == vm.PRUNED) == (with_zeros == 0.0)).all()
        # ties: the lower node index ranks higher -- it is kept first and pruned last
        ties = np.ones(10, np.float32)
        assert fn(ties, 0.2, 0.3).tolist() == [vm.KEPT] * 3 + [vm.QUANTISED] * 5 + [vm.PRUNED] * 2
    for prune, keep in ((0.001, 0.6), (0.1, 0.3), (0.5, 0.9), (0.0, 0.5), (1.0, 1.0)):
        for values in (imp, with_zeros, np.round(imp * 4) / 4):
            assert (compression.partition_by_shares(values, prune, keep) == vm.partition_by_shares(values, prune, keep)).all()
    assert (compression.partition_by_shares(torch.from_numpy(imp).reshape(1, 101, 1), 0.1, 0.3) == vm.partition_by_shares(imp, 0.1, 0.3)).all()
    with pytest.raises(ValueError):
        compression.partition_by_shares(-imp, 0.1, 0.3)


DIMS, F = (3, 5, 7), 12  # 105 nodes: the node mask ends in a ragged byte


def _config():
    return dict(voxel_size=rf.VoxelSize(0.5, 0.25, 0.125), grid_location=rf.VoxelGridLocation(0.1, 0.0, -0.2), density_preactivation=torch.nn.Identity(),
                density_postactivation=torch.nn.ReLU(), feature_preactivation=torch.nn.Identity(), feature_postactivation=torch.nn.Identity(),
                radiance_transfer_function=None, expected_density_scale=7.0, tunable=False)


def _hand_made(dtype=np.float32, fill=-2.5):
    rng = np.random.default_rng(5)
    nodes = DIMS[0] * DIMS[1] * DIMS[2]
    classes = rng.integers(0, 3, nodes).astype(np.uint8)
    classes[-3:] = (vm.KEPT, vm.PRUNED, vm.QUANTISED)  # the last byte of both bit streams is in use
    alive = classes != vm.PRUNED
    assert nodes % 8 and int(alive.sum()) % 8
    densities = rng.normal(size=int(alive.sum())).astype(dtype)
    kept = rng.normal(size=(int((classes == vm.KEPT).sum()), F)).astype(dtype)
    codebook = rng.normal(size=(37, F)).astype(dtype)
    indices = rng.integers(0, 37, int((classes == vm.QUANTISED).sum())).astype(np.uint16)
    field = rf.CompressedField(DIMS, F, alive, classes[alive] == vm.QUANTISED, densities, kept, codebook, indices, fill, _config(), [0.5, 0.25])
    return field, classes, densities, kept, codebook, indices


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_container_round_trip(dtype):
    field, classes, densities, kept, codebook, indices = _hand_made(dtype)
    data = field.to_bytes()
    assert isinstance(data, bytes)
    back = rf.CompressedField.from_bytes(data, config=_config())
    assert back.dims == DIMS and back.num_features == F and back.value_dtype == np.dtype(dtype).name and back.fill_density == -2.5
    assert (back.node_classes() == classes).all()
    stats = back.stats
    assert (stats["pruned"], stats["kept"], stats["quantised"]) == tuple(int((classes == k).sum()) for k in (vm.PRUNED, vm.KEPT, vm.QUANTISED))
    assert stats["payload_bytes"] == len(data) and stats["distortion"] == 0.25 and stats["num_codes"] == 37
    grid = back.decompress(storage="split")
    assert isinstance(grid, rf.VoxelGrid) and grid.grid_dims == DIMS and grid.storage == "split" and grid.expected_density_scale == 7.0
    assert tuple(grid.voxel_size) == (0.5, 0.25, 0.125) and grid.density_mode == "relu"
    dens, feat = grid.densities.reshape(-1), grid.features.reshape(-1, F)
    cls = torch.from_numpy(classes)
    assert (dens[cls == vm.PRUNED] == -2.5).all() and (feat[cls == vm.PRUNED] == 0).all()
    # stored values come back bit for bit (float16 values widened exactly)
    assert torch.equal(dens[cls != vm.PRUNED], torch.from_numpy(densities.astype(np.float32)))
    assert torch.equal(feat[cls == vm.KEPT], torch.from_numpy(kept.astype(np.float32)))
    assert torch.equal(feat[cls == vm.QUANTISED], torch.from_numpy(codebook.astype(np.float32)[indices.astype(np.int64)]))
    for storage in ("reference", "bricked"):
        other = back.decompress(storage=storage)
        assert torch.equal(other.densities, grid.densities) and torch.equal(other.features, grid.features)


def test_container_refuses_what_it_cannot_read():
    field = _hand_made()[0]
    with pytest.raises(ValueError, match="configuration"):
        rf.CompressedField.from_bytes(field.to_bytes()).decompress()
    with pytest.raises(ValueError):
        rf.CompressedField(DIMS, F, np.ones(105, bool), np.zeros(104, bool), np.zeros(105, np.float32), np.zeros((105, F), np.float32), np.zeros((0, F), np.float32), [])
    import io
    import json

    with np.load(io.BytesIO(field.to_bytes())) as z:
        arrays = {k: z[k] for k in z.files}
    header = json.loads(bytes(arrays["header"]).decode())
    assert header["version"] == compression.FORMAT_VERSION
    header["version"] += 1
    arrays["header"] = np.frombuffer(json.dumps(header).encode(), dtype=np.uint8)
    buffer = io.BytesIO()
    np.savez_compressed(buffer, **arrays)
    with pytest.raises(ValueError, match="version"):
        rf.CompressedField.from_bytes(buffer.getvalue())


def test_compact_checkpoint_loads_through_the_ordinary_loader(tmp_path):
    field = _hand_made(np.float16, fill=0.0)[0]
    want = field.decompress()
    cfg = rf.SHVoxGridRenderConfig(16, rf.CameraBounds(0.5, 4.0), perturb_sampled_points=False)
    model = rf.VolumetricModel(want, rf.render_sh_voxel_grid, cfg, device=torch.device("cpu"))
    info = model.get_save_info(extra_info={"note": "kept"}, compressed=field)
    payload = info[THRE3D_REPR][COMPRESSED_STATE]  # the bytes as a uint8 tensor: torch.save writes those verbatim
    assert set(info[THRE3D_REPR]) == {COMPRESSED_STATE, CONFIG_DICT} and payload.dtype == torch.uint8 and payload.numpy().tobytes() == field.to_bytes()
    torch.save(info, tmp_path / "compact.pth")
    assert (tmp_path / "compact.pth").stat().st_size < len(field.to_bytes()) + 8192
    # (plain bytes in the entry load as well)
    info_bytes = dict(info, **{THRE3D_REPR: {COMPRESSED_STATE: field.to_bytes(), CONFIG_DICT: info[THRE3D_REPR][CONFIG_DICT]}})
    assert torch.equal(rf.create_voxel_grid_from_saved_info_dict(info_bytes).features, want.features)
    loaded, extra = rf.create_volumetric_model_from_saved_model(tmp_path / "compact.pth", rf.create_voxel_grid_from_saved_info_dict)
    got = loaded.thre3d_repr
    assert extra == {"note": "kept"} and got.grid_dims == DIMS and tuple(got.aabb) == tuple(want.aabb) and got.density_mode == want.density_mode
    assert torch.equal(got.densities, want.densities) and torch.equal(got.features, want.features)
    assert loaded.render_config == cfg
    # a plain checkpoint of the same model takes the state-dict path as before
    plain = model.get_save_info()
    assert set(plain[THRE3D_REPR]) == {STATE_DICT, CONFIG_DICT}
    torch.save(plain, tmp_path / "plain.pth")
    again, _ = rf.create_volumetric_model_from_saved_model(tmp_path / "plain.pth", rf.create_voxel_grid_from_saved_info_dict)
    assert torch.equal(again.thre3d_repr.features, want.features)
    with pytest.raises(ValueError):
        other = rf.VolumetricModel(rf.VoxelGrid(torch.zeros(2, 2, 2, 1), torch.zeros(2, 2, 2, F), rf.VoxelSize(1, 1, 1)), rf.render_sh_voxel_grid, cfg, device=torch.device("cpu"))
        other.get_save_info(compressed=field)


def test_compress_without_quantised_nodes_needs_no_gpu():
    """keep_share = 1: every node of positive importance is kept verbatim; nothing reaches the quantiser"""
    rng = np.random.default_rng(11)
    grid = rf.VoxelGrid(torch.from_numpy(rng.normal(size=(*DIMS, 1)).astype(np.float32)), torch.from_numpy(rng.normal(size=(*DIMS, F)).astype(np.float32)),
                        rf.VoxelSize(1, 1, 1), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU(), storage="bricked")
    importance = torch.from_numpy(rng.uniform(0.1, 1.0, DIMS).astype(np.float32))
    importance[0, :, 0] = 0.0
    field = rf.compress_voxel_grid(grid, importance, prune_share=0.0, keep_share=1.0, value_dtype="float32")
    assert field.stats["pruned"] == 5 and field.stats["quantised"] == 0 and field.stats["kept"] == 100
    back = field.decompress(storage="bricked")
    seen = importance > 0
    assert torch.equal(back.features[seen], grid.features[seen]) and torch.equal(back.densities[seen], grid.densities[seen])
    assert (back.densities[~seen] == 0).all() and (back.features[~seen] == 0).all()
    with pytest.raises(ValueError, match="softplus"):
        soft = rf.VoxelGrid(grid.densities, grid.features, rf.VoxelSize(1, 1, 1), density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.Softplus())
        rf.compress_voxel_grid(soft, importance)
    with pytest.raises(RuntimeError, match="HIP device"):
        rf.compress_voxel_grid(grid, importance, keep_share=0.5)  # quantising a CPU grid: no fallback
