"""Total-variation regularisation on the GPU: rf_tv_grad against the float64 model (tests/tv_model.py), ops.total_variation through
autograd, and TrainStepper with TV weights."""
import functools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from thr3ed_atom_amd import ops
from thr3ed_atom_amd.optim import FlatGrid
from thr3ed_atom_amd.trainers import TrainStepper
from thr3ed_atom_amd.voxels import brick_nodes, unpack_storage
from tests import tv_model
from tests.helpers import hash_uniform, load_golden, procedural_grid

pytestmark = pytest.mark.gpu

STORAGES = ["reference", "split", "bricked"]
DIMS = [(1, 1, 1), (2, 3, 5), (9, 8, 17), (16, 16, 24)]
ACTIVATIONS = {  # F -> density activations: every density_mode is met (TV reads the raw parameter: the mode must not matter)
    3: (torch.nn.Identity(), torch.nn.ReLU()), 12: (torch.nn.Identity(), torch.nn.Softplus()), 27: (torch.abs, torch.nn.Identity()),
    48: (torch.nn.Identity(), torch.nn.Identity()),
}
LAMBDA = (1e-2, 1e-3)
SENTINEL = 12345.0


def T(a):
    return torch.from_numpy(np.asarray(a))


def make_grid(dev, dens, feat, storage, tunable=True, activations=(torch.nn.Identity(), torch.nn.ReLU())):
    G = dens.shape[0]
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=activations[0],
                        density_postactivation=activations[1], expected_density_scale=100.0 / 3.0, tunable=tunable, storage=storage)


@functools.lru_cache(maxsize=None)
def reference(dims, F, seed=7, lam=LAMBDA, eps=1e-8):
    """(densities, features, float64 gradient of densities / features, float64 sums) -- computed once per case, never modified"""
    dens, feat = procedural_grid(dims, F, seed)
    _, gd, gf = tv_model.tv_loss_and_grad(dens, feat, lam[0], lam[1], eps)
    sd, sf = tv_model.tv_sums(dens.double(), feat.double(), eps)
    return dens, feat, gd, gf, (float(sd), float(sf))


def padding_mask(grid, like):
    """bool tensor of the shape of ``like`` (a bricked tensor): True on padding nodes"""
    X, Y, Z = grid.grid_dims
    real = brick_nodes(torch.ones((X, Y, Z, 1), device=like.device))
    return (real == 0).expand_as(like)


def pattern_scale(dims, F):
    """a power of two near the smallest per-element weight of the case: a pattern of that size is visibly changed by every
    gradient added to it (a pattern of magnitude 1 would swallow a gradient below its half ulp)"""
    return 2.0 ** np.floor(np.log2(min(tv_model.element_weights(dims, F, *LAMBDA))))


def prefilled(grid, fill_seed, poison_parameters=True, scale=1.0):
    """gradient buffers in the layout of the grid holding a known non-zero pattern (in [0.5, 1.5) x ``scale``); bricked storage:
    SENTINEL in the padding of the gradients and (``poison_parameters``) NaN in the padding of the parameters"""
    out = []
    for i, p in enumerate(grid.kernel_tensors()):
        if p is None:
            out.append(None)
            continue
        b = T(hash_uniform(tuple(p.shape), fill_seed + i, 0.5, 1.5)).to(p.device) * float(scale)
        if grid.storage == "bricked":
            pad = padding_mask(grid, p)
            b[pad] = SENTINEL
            if poison_parameters:
                p.data[pad] = float("nan")
        out.append(b)
    return out


def check_padding(grid, tensors):
    if grid.storage != "bricked":
        return
    for t in tensors:
        if t is not None:
            pad = padding_mask(grid, t)
            assert bool((t[pad] == SENTINEL).all()), "a padding node of the gradient was written"
            assert bool(torch.isfinite(t[~pad]).all()), "a padding node of the parameters was read"


def to_reference(grid, first, second):
    d, f = unpack_storage(first, second, grid.storage, grid.grid_dims)
    return d.cpu(), f.cpu()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("F", [3, 12, 27, 48])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_kernel_equals_the_float64_model(hip_device, dims, F, storage):
    """Per element |g - g64| <= 64 * 2^-24 * w (tv_model.grad_bound: six terms of magnitude <= 1, each a subtract, three FMAs, a
    square root, a division and a product, then a five-add sum and the scaling by w; the bound leaves ~1.5x headroom); the sums to
    1e-5 relative; accumulation into a pre-filled buffer is the float32 sum of the buffer and the gradient, bit for bit; padding of
    bricked storage is neither read (NaN in the parameters) nor written (sentinel in the gradients)."""
    dens, feat, gd64, gf64, sums64 = reference(dims, F)
    grid = make_grid(hip_device, dens, feat, storage, activations=ACTIVATIONS[F])
    wd, wf = tv_model.element_weights(dims, F, *LAMBDA)
    fills = prefilled(grid, 300, scale=pattern_scale(dims, F))
    # into zeros (sentinel padding): the gradient itself
    zeros = [None if b is None else torch.where(b == SENTINEL, b, torch.zeros_like(b)) for b in fills]
    sums = torch.zeros(2, device=hip_device)
    ops.tv_grad_raw(grid, LAMBDA[0], LAMBDA[1], zeros[0], zeros[1], sums)
    check_padding(grid, zeros)
    gd, gf = to_reference(grid, *zeros)
    err_d, err_f = tv_model.grad_error(gd, gd64), tv_model.grad_error(gf, gf64)
    print(f"tv_grad {dims} F={F} {storage}: max error {err_d / (tv_model.ULP * wd):.2f} ulp(w) density, {err_f / (tv_model.ULP * wf):.2f} ulp(w) features")
    assert tv_model.grad_within_bound(gd, gd64, wd), (err_d, tv_model.grad_bound(wd))
    assert tv_model.grad_within_bound(gf, gf64, wf), (err_f, tv_model.grad_bound(wf))
    np.testing.assert_allclose(sums.cpu().numpy().astype(np.float64), np.array(sums64), rtol=1e-5)
    # into the pattern: accumulated, not overwritten
    acc = [None if b is None else b.clone() for b in fills]
    ops.tv_grad_raw(grid, LAMBDA[0], LAMBDA[1], acc[0], acc[1])
    check_padding(grid, acc)
    for a, b, z in zip(acc, fills, zeros):
        if a is not None:
            real = b != SENTINEL
            assert torch.equal(a[real], (b + z)[real])
            assert bool((a[real] != b[real]).any()) or max(dims) == 1


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("F", [3, 27, 12])
def test_constant_grid_gives_sqrt_epsilon_and_a_zero_gradient(hip_device, F, storage):
    dims = (9, 8, 17)
    dens, feat = torch.full(dims + (1,), 0.375), torch.full(dims + (F,), -1.25)
    grid = make_grid(hip_device, dens, feat, storage)
    fills = prefilled(grid, 310)
    out = [None if b is None else b.clone() for b in fills]
    sums = torch.zeros(2, device=hip_device)
    eps = 4e-6
    ops.tv_grad_raw(grid, 0.5, 0.25, out[0], out[1], sums, epsilon=eps)
    for a, b in zip(out, fills):
        assert a is None or torch.equal(a, b)  # + (+-0) leaves every bit
    n = float(np.prod(dims))
    r = float(np.sqrt(np.float32(eps)))
    np.testing.assert_allclose(sums.cpu().numpy(), [n * r, n * F * r], rtol=1e-5)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("F", [3, 27, 48])
def test_a_zero_weight_leaves_its_channels_untouched(hip_device, F, storage):
    dims = (9, 8, 17)
    dens, feat, gd64, gf64, _ = reference(dims, F)
    grid = make_grid(hip_device, dens, feat, storage)
    has_second = grid.kernel_tensors()[1] is not None
    scale = pattern_scale(dims, F)
    for lam in ((LAMBDA[0], 0.0), (0.0, LAMBDA[1])):
        fills = prefilled(grid, 320, scale=scale)
        out = [None if b is None else b.clone() for b in fills]
        # the tensor no non-zero weight reaches may be missing altogether
        if storage == "reference":
            args = (out[0], None) if lam[1] == 0.0 else (None, out[1])
        else:
            args = (out[0], None) if (lam[1] == 0.0 or not has_second) else (out[0], out[1])
        ops.tv_grad_raw(grid, lam[0], lam[1], *args)
        check_padding(grid, out)
        bd, bf = to_reference(grid, *fills)
        od, of = to_reference(grid, *out)
        if lam[1] == 0.0:
            assert torch.equal(of, bf) and not torch.equal(od, bd)
        else:
            assert torch.equal(od, bd) and not torch.equal(of, bf)
        # ... and the other tensor still gets its gradient: pattern + gradient, rounded once (|sum| <= 1.5 scale + 6 w)
        wd, wf = tv_model.element_weights(dims, F, *LAMBDA)
        if lam[1] == 0.0:
            np.testing.assert_allclose((od.double() - bd.double()).numpy(), gd64.numpy(), rtol=0, atol=tv_model.ULP * (1.5 * scale + 6 * wd) + tv_model.grad_bound(wd))
        else:
            np.testing.assert_allclose((of.double() - bf.double()).numpy(), gf64.numpy(), rtol=0, atol=tv_model.ULP * (1.5 * scale + 6 * wf) + tv_model.grad_bound(wf))


@pytest.mark.parametrize("storage", STORAGES)
def test_two_launches_give_bit_identical_gradients(hip_device, storage):
    dims, F = (16, 16, 24), 27
    dens, feat, *_ = reference(dims, F)
    grid = make_grid(hip_device, dens, feat, storage)
    runs = []
    for _ in range(2):
        out = [None if p is None else torch.zeros_like(p) for p in grid.kernel_tensors()]
        ops.tv_grad_raw(grid, LAMBDA[0], LAMBDA[1], out[0], out[1], torch.zeros(2, device=hip_device))
        runs.append(out)
    for a, b in zip(*runs):
        assert a is None or torch.equal(a, b)


@pytest.mark.parametrize("bucket", [False, True])
@pytest.mark.parametrize("storage", STORAGES)
def test_total_variation_through_autograd(hip_device, storage, bucket):
    dims, F = (9, 8, 17), 27
    dens, feat, gd64, gf64, sums64 = reference(dims, F)
    grid = make_grid(hip_device, dens, feat, storage)
    flat = FlatGrid(grid) if bucket else None
    tvd, tvf = rf.total_variation(grid)
    assert tvd.dim() == 0 and tvf.dim() == 0
    n = float(np.prod(dims))
    np.testing.assert_allclose([float(tvd), float(tvf)], [sums64[0] / n, sums64[1] / (n * F)], rtol=1e-5)
    (LAMBDA[0] * tvd + LAMBDA[1] * tvf).backward()
    first, second = grid.kernel_tensors()
    if bucket:
        g_first, g_second = flat.views_for_accumulation()
        nd = first.numel()
        assert g_first.data_ptr() == flat.flat_grad.data_ptr() and torch.equal(flat.flat_grad[:nd].view_as(first), g_first)
        assert first.grad is g_first  # nothing was returned to autograd: the kernel added into the bucket
    else:
        g_first, g_second = first.grad, (None if second is None else second.grad)
    gd, gf = to_reference(grid, g_first, g_second)
    wd, wf = tv_model.element_weights(dims, F, *LAMBDA)
    # (the weights reach the kernel as float32 values of lambda: one more rounding of w, inside the bound's headroom)
    assert tv_model.grad_within_bound(gd, gd64, wd) and tv_model.grad_within_bound(gf, gf64, wf)
    if flat is not None:
        flat.detach()


def missing_rays(dev, n=64):
    """rays that start outside the volume and point away from it: the render gradient is exactly zero"""
    o = T(hash_uniform((n, 3), 41, 9.0, 10.0)).to(dev)
    d = T(hash_uniform((n, 3), 42, 0.5, 1.0)).to(dev)
    return rf.Rays(o, d), T(hash_uniform((n, 3), 43, 0.0, 1.0)).to(dev)


@functools.lru_cache(maxsize=None)
def trainer_reference():
    c = tv_model.TRAINER_CASE
    dens, feat = procedural_grid(c["dims"], c["num_features"], c["seed"])
    return (dens, feat) + tuple(tv_model.adam_trajectory(dens, feat, c["weight_density"], c["weight_features"], c["eps"], c["lr"], c["steps"]))


STEPPERS = {
    "fused-binned-merged": dict(fused=True, backward="binned"),
    "fused-binned-per-render": dict(fused=True, backward="binned", merge_bricks=False),
    "fused-binned-pieces": dict(fused=True, backward="binned"),  # with a kernel timer: the launches issued one by one
    "fused-atomic": dict(fused=True, backward="atomic"),
    "autograd": dict(fused=False),
}


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("config", list(STEPPERS))
def test_trainer_with_tv_alone_equals_float64_adam(hip_device, monkeypatch, config, storage):
    """Rays that miss the volume leave TV as the only gradient: three steps must equal torch.optim.Adam in float64 on the model's
    gradient to the tolerance of test_fused_adam_matches_torch_adam (2e-6), on the elements whose float64 gradient stays >= 100 x the
    kernel's gradient bound (at most 1 % left out; tests/test_tv_model.py checks the model's share on the CPU)."""
    c = tv_model.TRAINER_CASE
    dens, feat, ref_d, ref_f, keep_d, keep_f = trainer_reference()
    if config == "fused-binned-pieces":
        monkeypatch.setattr(ops, "KERNEL_TIMER", ops.KernelTimer())
    grid = make_grid(hip_device, dens, feat, storage)
    cfg = rf.SHVoxGridRenderConfig(16, rf.CameraBounds(1.8, 6.6), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, 64, learning_rate=c["lr"], data_parallel=False, tv_density_weight=c["weight_density"],
                           tv_feature_weight=c["weight_features"], tv_epsilon=c["eps"], **STEPPERS[config])
    assert stepper.fuse_optimizer is False and stepper.flat.deferred is False and stepper.exchange == "dense"
    assert stepper.merged_bricks == (config in ("fused-binned-merged", "fused-binned-pieces"))
    rays, pixels = missing_rays(hip_device)
    tv0 = tv_model.tv_values(dens, feat, c["eps"])
    for it in range(c["steps"]):
        stats = stepper.step_on(rays, pixels)
        if it == 0:  # the TV values of the step are those of the parameters it started from
            np.testing.assert_allclose([float(stats.tv_density), float(stats.tv_features)], tv0, rtol=1e-5)
    for got, ref, keep in ((grid.densities, ref_d, keep_d), (grid.features, ref_f, keep_f)):
        left_out = 1.0 - float(keep.double().mean())
        assert left_out <= 0.01
        err = (got.detach().double().cpu() - ref).abs()[keep]
        print(f"{config} {storage}: compared {1 - left_out:.4%}, max |param - float64 Adam| = {float(err.max()):.3e}")
        assert float(err.max()) <= 2e-6
    stepper.flat.detach()


@pytest.mark.parametrize("jitter", ["off", "keyed-seeded"])
def test_fused_and_autograd_steps_with_tv_stay_together(hip_device, jitter):
    """16^3 / SH degree 2 with real renders: the fused step (split storage) and the autograd step (reference storage), both with TV,
    for five iterations, to the tolerance of test_autograd_trainer_with_deferred_gradients_equals_the_fused_step.  The sample jitter
    is the same on both sides: none, or the keyed jitter of an equally seeded generator (the autograd step takes no t_rand tensor)."""
    g = load_golden("g9_trainer_trajectory.npz")
    G, _, hw, n_img, n_rays, steps, S = (int(v) for v in g["config"])
    F, iters, lr = 27, 5, float(g["lr"])
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(float(g["near"]), float(g["far"])), perturb_sampled_points=jitter != "off", white_bkgd=True)
    runs = []
    for storage, fused in (("reference", False), ("split", True)):
        grid = make_grid(hip_device, T(hash_uniform((G, G, G, 1), 901)), T(hash_uniform((G, G, G, F), 900 + F)), storage)
        model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
        stepper = TrainStepper(model, n_rays, learning_rate=lr, fused=fused, data_parallel=False, tv_density_weight=1e-2, tv_feature_weight=1e-3)
        assert not stepper.flat.deferred and not stepper.fuse_optimizer
        losses = []
        for it in range(iters):
            torch.manual_seed(5000 + it)
            rays = rf.Rays(T(g["origins"][it]).to(hip_device), T(g["directions"][it]).to(hip_device))
            st = stepper.step_on(rays, T(g["pixels"][it]).to(hip_device))
            losses.append((st.specular_loss.item(), st.diffuse_loss.item(), st.tv_density.item(), st.tv_features.item()))
        runs.append((losses, grid.densities.detach().clone(), grid.features.detach().clone(), stepper.optimizer.step_count))
        stepper.flat.detach()
    np.testing.assert_allclose(np.array(runs[0][0]), np.array(runs[1][0]), rtol=2e-5)
    assert runs[0][3] == runs[1][3] == iters
    for a, b in ((runs[0][1], runs[1][1]), (runs[0][2], runs[1][2])):
        err = (a - b).abs()
        assert float((err <= 2e-5).float().mean()) >= 0.999 and float(err.max()) <= lr * 2 * iters + 1e-6
    # TV took part: the same five steps without it end somewhere else
    assert np.array(runs[1][0])[:, 2].min() > 0.0


def _model(dev, storage="split", F=27, G=16):
    dens, feat = procedural_grid((G, G, G), F, 3)
    grid = make_grid(dev, dens, feat, storage)
    cfg = rf.SHVoxGridRenderConfig(16, rf.CameraBounds(1.8, 6.6), perturb_sampled_points=False, white_bkgd=True)
    return rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)


def test_tv_options_that_cannot_hold_a_gradient_bucket_raise(hip_device):
    with pytest.raises(ValueError, match="fuse_optimizer"):
        TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, tv_density_weight=0.1, fuse_optimizer=True)
    with pytest.raises(ValueError, match="owner"):
        TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, tv_density_weight=0.1, exchange="owner")
    with pytest.raises(ValueError):
        TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, tv_feature_weight=-1.0)
    with pytest.raises(ValueError):
        TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, tv_feature_weight=0.1, tv_epsilon=0.0)


@pytest.mark.parametrize("storage,fused", [("split", True), ("bricked", True), ("reference", True), ("reference", False), ("split", False)])
def test_zero_tv_weights_resolve_every_option_as_before(hip_device, storage, fused):
    """With both weights 0 the stepper is the stepper it was: same fuse_optimizer, brick_size, exchange, merged_bricks, backward and
    deferred bucket as a stepper built without the arguments, no TV ring, and StepStats without TV values."""
    plain = TrainStepper(_model(hip_device, storage), 64, 0.03, data_parallel=False, fused=fused)
    plain.flat.detach()
    zero = TrainStepper(_model(hip_device, storage), 64, 0.03, data_parallel=False, fused=fused, tv_density_weight=0.0, tv_feature_weight=0.0, tv_epsilon=1e-8)
    for name in ("fuse_optimizer", "brick_size", "exchange", "merged_bricks", "backward"):
        assert getattr(zero, name) == getattr(plain, name), name
    assert zero.flat.deferred == plain.flat.deferred and zero.flat.brick_size == plain.flat.brick_size
    # what those resolve to today, spelled out (single process, 16^3 / SH degree 2, binned on every grid under the tests' environment)
    if fused:
        assert zero.fuse_optimizer == (storage != "reference") and zero.exchange == "dense"
    else:
        assert zero.flat.deferred == (storage == "reference")
    rays, pixels = missing_rays(hip_device)
    stats = zero.step_on(rays, pixels)
    assert stats.tv_density is None and stats.tv_features is None and zero._tv_ring is None
    on = TrainStepper(_model(hip_device, storage), 64, 0.03, data_parallel=False, fused=fused, tv_density_weight=1e-3)
    assert on.fuse_optimizer is False and on.flat.deferred is False and on.exchange == "dense"
    zero.flat.detach()
    on.flat.detach()
