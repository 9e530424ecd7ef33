"""Distortion loss on the GPU: rf_distortion against the float64 model (tests/distortion_model.py) and its exact properties,
ops.distortion_loss through autograd, and TrainStepper(distortion_weight=...)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import thr3ed_atom_amd as rf
from oracle import relu_field_oracle as orc
from tests import distortion_model as dm
from tests.helpers import hash_uniform, procedural_grid
from thr3ed_atom_amd import _lib, ops
from thr3ed_atom_amd.optim import FlatGrid
from thr3ed_atom_amd.trainers import TrainStepper
from thr3ed_atom_amd.voxels import brick_nodes, unpack_storage

pytestmark = pytest.mark.gpu

ACTIVATIONS = {"relu": (torch.nn.Identity(), torch.nn.ReLU()), "softplus": (torch.nn.Identity(), torch.nn.Softplus()),
               "abs": (torch.abs, torch.nn.Identity()), "identity": (torch.nn.Identity(), torch.nn.Identity())}
WORST = {"loss": 0.0, "grad": 0.0}  # the largest errors met, relative to their bars (printed per case)


def T(a):
    return torch.from_numpy(np.asarray(a))


def make_grid(dev, dens, feat, dims, storage, mode, rho, tunable=False):
    return rf.VoxelGrid(dens.clone().to(dev), feat.clone().to(dev), rf.VoxelSize(*dm.voxel_of(dims)), density_preactivation=ACTIVATIONS[mode][0],
                        density_postactivation=ACTIVATIONS[mode][1], expected_density_scale=rho, tunable=tunable, storage=storage)


def padding_mask(grid, like):
    X, Y, Z = grid.grid_dims
    real = brick_nodes(torch.ones((X, Y, Z, 1), device=like.device))
    return (real == 0).expand_as(like)


def poison_padding(grid):
    if grid.storage == "bricked":
        for t in grid.kernel_tensors():
            if t is not None:
                t.data[padding_mask(grid, t)] = float("nan")


def density_gradient(grid, gfirst):
    """the density part of a gradient tensor in the grid's layout, as float64 numpy [X,Y,Z]"""
    second = None if grid.storage == "reference" else grid.kernel_tensors()[1]
    d, _ = unpack_storage(gfirst, None if second is None else torch.zeros_like(second), grid.storage, grid.grid_dims)
    return d.cpu().numpy().astype(np.float64)[..., 0]


def batch_of(dev, o, d, S, near, far, option, t_rand, first_ray=0):
    """(RayBatch, flags) of a case's option; the two flags the term must ignore ride along on odd S"""
    flags, jitter = 0, None
    if option == "aabb":
        flags |= _lib.FLAG_AABB_SAMPLING
    if option == "occupancy":
        flags |= _lib.FLAG_OCCUPANCY_SKIP
    if option == "t_rand":
        jitter = t_rand.to(dev).contiguous()
    if option == "keyed":
        jitter = ops.KeyedJitter(dm.JITTER_KEY, 5 + first_ray)
    flags |= (_lib.FLAG_WHITE_BKGD | _lib.FLAG_RENDER_DIFFUSE) if S % 2 else 0
    return ops.RayBatch(o.to(dev).contiguous(), d.to(dev).contiguous(), S, near, far, t_rand=jitter), flags


@pytest.mark.parametrize("dims,storage,S,F,mode,option,count", dm.kernel_cases(), ids=dm.case_id)
def test_kernel_equals_the_float64_model(hip_device, dims, storage, S, F, mode, option, count):
    """|l - l64| <= 2e-5 max(1, max_ij |m_i - m_j|) per ray; the density gradient, weighted per ray by a known grad_loss and a scale,
    within rtol 5e-4 + 5e-6 max |g64| on EVERY node, added onto a pre-filled buffer (a pattern 2^-10 of the gradient's size: adding it
    costs the sum a rounding 1000 times below the bar, overwriting it would miss the bar 200-fold); NaN in the padding of bricked
    parameters is never read, the padding of the gradient never written; the feature tensors keep their bits."""
    ref, t_rand = dm.case_reference(dims, F, mode, S, option, count)
    dens, feat = dm.case_grid(dims, F, mode)
    o, d, near, far = dm.case_rays(count, S)
    grid = make_grid(hip_device, dens, feat, dims, storage, mode, dm.rho_of(mode, S))
    if option == "occupancy":
        grid.build_occupancy()
    poison_padding(grid)
    first, second = grid.kernel_tensors()
    second_before = None if second is None else second.clone()
    first_before = first.clone()
    batch, flags = batch_of(hip_device, o, d, S, near, far, option, t_rand)
    scale = 0.75
    g64 = scale * ref["grad"]
    gmax = float(np.abs(g64).max())
    unit = 2.0 ** (np.floor(np.log2(gmax)) - 10) if gmax > 0 else 1.0
    pattern = T(hash_uniform(tuple(first.shape), 300, 0.5, 1.5)).to(hip_device) * float(unit)
    if storage == "bricked":
        pattern[padding_mask(grid, pattern)] = float("nan")
    out = pattern.clone()
    loss = torch.full((count,), float("nan"), device=hip_device)
    gl = T(dm.case_grad_loss(count)).to(hip_device)
    ops.distortion_raw(grid, batch, flags, scale, gl, loss, out)
    got = loss.cpu().numpy().astype(np.float64)
    err_l = np.abs(got - ref["loss"]) / dm.loss_bar(ref["spread"])
    g = density_gradient(grid, out) - density_gradient(grid, pattern)
    bar_g = dm.GRAD_ATOL * gmax + dm.GRAD_RTOL * np.abs(g64)
    err_g = float((np.abs(g - g64) / np.where(bar_g > 0, bar_g, 1.0)).max()) if gmax > 0 else 0.0
    WORST["loss"], WORST["grad"] = max(WORST["loss"], float(err_l.max())), max(WORST["grad"], err_g)
    print(f"distortion {dm.case_id(dims)} {storage} S={S} F={F} {mode} {option} {count} rays: max |l - l64| = {np.abs(got - ref['loss']).max():.3e} "
          f"({err_l.max():.3f} of the bar), gradient {err_g:.3f} of its bar (max |g64| {gmax:.3e}); worst so far {WORST['loss']:.3f} / {WORST['grad']:.3f}")
    assert np.isfinite(got).all() and (err_l <= 1.0).all(), err_l.max()
    if gmax > 0:
        assert dm.grad_within_bar(g, g64), err_g
    else:  # nothing to add: the pattern keeps its bits
        assert torch.equal(out.nan_to_num(7.0), pattern.nan_to_num(7.0))
    # everything but the density element of the gradient keeps the pattern's bits; the parameters are untouched
    if storage != "reference":
        assert torch.equal(out[..., 1:].nan_to_num(7.0), pattern[..., 1:].nan_to_num(7.0))
    if storage == "bricked":
        pad = padding_mask(grid, out)
        assert bool(torch.isnan(out[pad]).all()) and bool(torch.isfinite(out[~pad]).all())
    assert torch.equal(first.nan_to_num(7.0), first_before.nan_to_num(7.0))
    assert second is None or torch.equal(second.nan_to_num(7.0), second_before.nan_to_num(7.0))


@pytest.mark.parametrize("storage", dm.STORAGES)
def test_exact_properties(hip_device, storage):
    """loss-only leaves the gradient buffer's bits; a grad_loss of zeros (or scale 0) adds nothing; l is bit-identical on relaunch,
    with and without the gradient pass, and under a split into two calls with first_ray (keyed jitter)."""
    dims, F, mode, S, count = (9, 8, 17), 27, "relu", 130, 67
    dens, feat = dm.case_grid(dims, F, mode)
    o, d, near, far = dm.case_rays(count, S)
    grid = make_grid(hip_device, dens, feat, dims, storage, mode, dm.rho_of(mode, S))
    poison_padding(grid)
    first, second = grid.kernel_tensors()
    pattern = T(hash_uniform(tuple(first.shape), 301, 0.5, 1.5)).to(hip_device)

    def run(lo=0, hi=count, grad=None, gl=None, scale=1.0, want_loss=True):
        batch, flags = batch_of(hip_device, o[lo:hi], d[lo:hi], S, near, far, "keyed", None, first_ray=lo)
        loss = torch.full((hi - lo,), float("nan"), device=hip_device) if want_loss else None
        ops.distortion_raw(grid, batch, flags, scale, gl, loss, grad)
        return loss

    whole = run()
    assert bool(torch.isfinite(whole).all()) and float(whole.max()) > 1e-3
    assert torch.equal(run(), whole)
    assert torch.equal(torch.cat([run(0, 30), run(30, count)]), whole)
    buf = pattern.clone()
    assert torch.equal(run(grad=buf, scale=0.0), whole) and torch.equal(buf, pattern)  # scale 0: the loss-only launch
    assert torch.equal(run(grad=buf, gl=torch.zeros(count, device=hip_device)), whole) and torch.equal(buf, pattern)
    assert torch.equal(run(grad=buf, gl=torch.ones(count, device=hip_device), scale=1e-3), whole) and not torch.equal(buf, pattern)
    second_before = None if second is None else second.clone()
    run(grad=pattern.clone(), want_loss=False)
    assert second is None or torch.equal(second.nan_to_num(7.0), second_before.nan_to_num(7.0))


@functools.lru_cache(maxsize=None)
def autograd_reference():
    dims, F, mode, S, count = (9, 8, 17), 27, "relu", 65, 67
    dens, feat = dm.case_grid(dims, F, mode)
    o, d, near, far = dm.case_rays(count, S)
    t_rand = T(hash_uniform((count, S), 78, 0.0, 1.0))
    ref = dm.model(dens, orc.make_aabb(dims, dm.voxel_of(dims)), dm.rho_of(mode, S), mode, o, d, near, far, S, t_rand=t_rand)
    assert ref["band"] == 0
    return dims, F, mode, S, count, t_rand, ref


@pytest.mark.parametrize("bucket", [False, True])
@pytest.mark.parametrize("storage", dm.STORAGES)
def test_distortion_loss_through_autograd(hip_device, storage, bucket):
    dims, F, mode, S, count, t_rand, ref = autograd_reference()
    dens, feat = dm.case_grid(dims, F, mode)
    o, d, near, far = dm.case_rays(count, S)
    grid = make_grid(hip_device, dens, feat, dims, storage, mode, dm.rho_of(mode, S), tunable=True)
    flat = FlatGrid(grid) if bucket else None
    rays = rf.Rays(o.to(hip_device), d.to(hip_device))
    L = rf.distortion_loss(grid, rays, S, rf.CameraBounds(near, far), t_rand=t_rand.to(hip_device))
    assert L.dim() == 0 and abs(float(L) - ref["loss"].mean()) <= float(dm.loss_bar(ref["spread"]).max())
    (3.0 * L).backward()
    first, second = grid.kernel_tensors()
    if bucket:
        g_first, _ = flat.views_for_accumulation()
        assert first.grad is g_first  # nothing was returned to autograd: the kernel added into the bucket
    else:
        g_first = first.grad
        assert second is None or second.grad is None  # the features do not enter
    assert dm.grad_within_bar(density_gradient(grid, g_first), 3.0 * ref["grad"] / count)
    if storage != "reference":
        assert float(g_first[..., 1:].abs().max()) == 0.0
    if flat is not None:
        flat.detach()


def test_distortion_loss_on_a_foreign_grid_and_a_model(hip_device):
    dims, F, mode, S, count, t_rand, ref = autograd_reference()
    dens, feat = dm.case_grid(dims, F, mode)
    o, d, near, far = dm.case_rays(count, S)
    src = make_grid(hip_device, dens, feat, dims, "reference", mode, dm.rho_of(mode, S), tunable=True)

    class Foreign(torch.nn.Module):  # the reference VoxelGrid's attribute names, nothing else
        def __init__(self):
            super().__init__()
            self.densities, self.features = torch.nn.Parameter(src.densities.detach().clone()), torch.nn.Parameter(src.features.detach().clone())
            self.aabb, self._expected_density_scale = src.aabb, src.expected_density_scale
            self._density_preactivation, self._density_postactivation = torch.nn.Identity(), torch.nn.ReLU()

    foreign = Foreign()
    rays = rf.Rays(o.to(hip_device), d.to(hip_device))
    bounds = rf.CameraBounds(near, far)
    L = rf.distortion_loss(foreign, rays, S, bounds, t_rand=t_rand.to(hip_device))
    L.backward()
    assert dm.grad_within_bar(foreign.densities.grad.cpu().numpy().astype(np.float64)[..., 0], ref["grad"] / count)
    cfg = rf.SHVoxGridRenderConfig(S, bounds, perturb_sampled_points=False)
    model = rf.VolumetricModel(src, rf.render_sh_voxel_grid, cfg, device=hip_device)
    assert float(rf.distortion_loss(model, rays, S, (near, far), t_rand=t_rand.to(hip_device))) == float(L)


# --------------------------------------------------------------------------------------------
# the trainer
# --------------------------------------------------------------------------------------------
STEPPERS = {
    "fused-binned-merged": dict(fused=True, backward="binned"),
    "fused-binned-per-render": dict(fused=True, backward="binned", merge_bricks=False),
    "fused-binned-pieces": dict(fused=True, backward="binned"),  # with a kernel timer: the launches issued one by one
    "fused-atomic": dict(fused=True, backward="atomic"),
    "autograd": dict(fused=False),
}
ADAM_CASE = dict(dims=(9, 8, 17), F=3, S=16, count=67, lr=0.01, weight=0.5, steps=3)


@functools.lru_cache(maxsize=None)
def adam_reference():
    """float64 torch.optim.Adam on the model's gradient of weight * mean_r l_r: (start densities, features, densities after the
    steps, sum l of step 0, per-node bar, mask of the nodes whose gradient is exactly 0 in every step).
    The bar: Adam's update lr m^ / (sqrt(v^) + eps) is homogeneous of degree 0 in the gradients of the steps so far and bounded by
    lr, so a relative error rho_t of the step's gradient moves it by at most 2 lr rho_t; the kernel's bar allows
    rho_t = GRAD_RTOL + GRAD_ATOL max|g_t| / |g_t| on a node, and the parameter error of the earlier steps feeds back into the later
    gradients (a factor 2 on top).  Per node: sum_t min(2 lr, 4 lr rho_t) -- vacuous (a full step either way) exactly where the gradient
    is within the kernel's absolute bar of zero, and no node is left out."""
    c = ADAM_CASE
    dens, feat = procedural_grid(c["dims"], c["F"], 51)
    # the outermost layer of nodes is negative: between a face of the box and the first plane of nodes the interpolation pads with
    # zeros, so a sample there has a colour below 1 -- with sigma = 0 (closed ReLU gate, weight 0) it cannot carry a render gradient
    edge = np.zeros(c["dims"], dtype=bool)
    for axis, size in enumerate(c["dims"]):
        index = [slice(None)] * 3
        for at in (0, size - 1):
            index[axis] = at
            edge[tuple(index)] = True
    dens = torch.where(torch.from_numpy(edge)[..., None], -dens.abs() - 0.01, dens)
    o, d, near, far = dm.case_rays(c["count"], c["S"])
    aabb = orc.make_aabb(c["dims"], dm.voxel_of(c["dims"]))
    D = dens.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([D], lr=c["lr"], betas=(0.9, 0.999))
    bar, zero, first_sum = np.zeros(c["dims"]), np.ones(c["dims"], dtype=bool), None
    for it in range(c["steps"]):
        ref = dm.model(D.detach(), aabb, 100.0 / 3.0, "relu", o, d, near, far, c["S"])
        assert ref["band"] == 0
        g = c["weight"] * ref["grad"] / c["count"]
        first_sum = ref["loss"].sum() if it == 0 else first_sum
        with np.errstate(divide="ignore"):
            rho = dm.GRAD_RTOL + dm.GRAD_ATOL * np.abs(g).max() / np.abs(g)
        bar += np.minimum(2 * c["lr"], 4 * c["lr"] * rho)
        zero &= g == 0
        D.grad = torch.from_numpy(g)[..., None].clone()
        opt.step()
    return dens, feat, D.detach()[..., 0].numpy(), first_sum, bar + 1e-7, zero


def missing_pixels(dev, n):
    return T(hash_uniform((n, 3), 43, 0.0, 1.0)).to(dev)


@pytest.mark.parametrize("storage", dm.STORAGES)
@pytest.mark.parametrize("config", list(STEPPERS))
def test_trainer_with_distortion_alone_equals_float64_adam(hip_device, monkeypatch, config, storage):
    """Three steps whose only density gradient is the distortion term, against torch.optim.Adam in float64 on the model's gradient,
    on EVERY node at the per-node bar adam_reference() derives from the kernel's gradient bar; a node whose float64 gradient is exactly
    0 in every step (no sample with an open ReLU gate weights it) keeps its bits.  The render gradients are removed by construction: every
    feature is 100, so a sample whose 8 corners are nodes has the colour sigmoid(28.2) = 1.0f, and on a white background
    e_i = gC . (c_i - 1) and c (1 - c) vanish for any target; the samples of the zero-padded outer shell have sigma = 0 (adam_reference)."""
    c = ADAM_CASE
    dens, feat, ref_d, first_sum, bar, zero = adam_reference()
    if config == "fused-binned-pieces":
        monkeypatch.setattr(ops, "KERNEL_TIMER", ops.KernelTimer())
    grid = make_grid(hip_device, dens, torch.full_like(feat, 100.0), c["dims"], storage, "relu", 100.0 / 3.0, tunable=True)
    o, d, near, far = dm.case_rays(c["count"], c["S"])
    cfg = rf.SHVoxGridRenderConfig(c["S"], rf.CameraBounds(near, far), perturb_sampled_points=False, white_bkgd=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, c["count"], learning_rate=c["lr"], data_parallel=False, distortion_weight=c["weight"], **STEPPERS[config])
    assert stepper.fuse_optimizer is False and stepper.flat.deferred is False and stepper.exchange == "dense"
    assert stepper.merged_bricks == (config in ("fused-binned-merged", "fused-binned-pieces"))
    rays = rf.Rays(o.to(hip_device), d.to(hip_device))
    target = missing_pixels(hip_device, c["count"])
    for it in range(c["steps"]):
        stats = stepper.step_on(rays, target)
        if it == 0:
            np.testing.assert_allclose(float(stats.distortion), first_sum, rtol=1e-4)
    # (the features are not the subject: whatever reaches them, Adam moves an element by at most lr per step, which leaves every
    # interior colour saturated)
    assert float((grid.features.detach() - 100.0).abs().max()) <= c["steps"] * c["lr"] * 1.001
    got = grid.densities.detach().cpu().numpy()[..., 0]
    err = np.abs(got.astype(np.float64) - ref_d)
    tight = bar <= 0.1 * c["lr"]  # the nodes on which the bar says something
    print(f"{config} {storage}: max |D - float64 Adam| / bar = {(err / bar).max():.3f}; {tight.mean():.1%} of the nodes have a bar below lr / 10, "
          f"largest error there {err[tight].max():.3e}; {zero.mean():.1%} exact zeros")
    assert (err <= bar).all(), float((err / bar).max())
    assert np.array_equal(got[zero].view(np.uint32), dens.numpy()[..., 0][zero].view(np.uint32))
    assert (tight & ~zero).sum() >= 50  # (a property of the case: the comparison is not vacuous)
    assert np.abs(ref_d - dens.numpy()[..., 0]).max() > 1e-3  # the steps moved the densities
    stepper.flat.detach()


@pytest.mark.parametrize("config,storage", [("fused-binned-merged", "split"), ("fused-atomic", "reference"), ("autograd", "reference"), ("fused-binned-per-render", "bricked")])
def test_stepper_gradient_equals_the_autograd_sum_of_renders_and_distortion_loss(hip_device, config, storage):
    """dims (9, 8, 17), 130 rays, keyed jitter: the bucket of one TrainStepper(distortion_weight > 0) iteration against autograd of
    L1(specular) + L1(diffuse) + weight * distortion_loss with the SAME jitter keys (an equally seeded generator), on a second grid."""
    dims, F, S, n, weight = (9, 8, 17), 27, 24, 130, 0.3
    dens, feat = procedural_grid(dims, F, 61)
    cam_o, cam_d, near, far = dm.case_rays(67, S)
    o = torch.cat([cam_o, cam_o[:63]]).contiguous()
    d = torch.cat([cam_d, cam_d[:63] * 1.01]).contiguous()
    cfg = rf.SHVoxGridRenderConfig(S, rf.CameraBounds(near, far), perturb_sampled_points=True, white_bkgd=True)
    rays = rf.Rays(o.to(hip_device), d.to(hip_device))
    pixels = missing_pixels(hip_device, n)
    # the stepper: lr 0 would still move nothing but Adam divides by sqrt(v): read the bucket BEFORE the optimizer by hooking it
    grid = make_grid(hip_device, dens, feat, dims, storage, "relu", 100.0 / 3.0, tunable=True)
    model = rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=hip_device)
    stepper = TrainStepper(model, n, learning_rate=0.01, data_parallel=False, distortion_weight=weight, **STEPPERS[config])
    seen = {}
    real_step = stepper.optimizer.step

    def spy(*args, **kwargs):
        seen["grad"] = [None if g is None else g.clone() for g in stepper.flat.views_for_accumulation()]
        return real_step(*args, **kwargs)

    stepper.optimizer.step = spy
    torch.manual_seed(77)
    stats = stepper.step_on(rays, pixels)
    gd, gf = unpack_storage(seen["grad"][0], seen["grad"][1], storage, dims)
    # autograd on a reference-storage twin, the same two key draws
    twin = make_grid(hip_device, dens, feat, dims, "reference", "relu", 100.0 / 3.0, tunable=True)
    torch.manual_seed(77)
    k0 = ops.KeyedJitter(ops.draw_jitter_key(), 0)
    k1 = ops.KeyedJitter(ops.draw_jitter_key(), 0)
    spec = rf.render_sh_voxel_grid(twin, rays, cfg, t_rand=k0).colour
    diff = rf.render_sh_voxel_grid(twin, rays, dataclasses.replace(cfg, render_diffuse=True), t_rand=k1).colour
    L = rf.distortion_loss(twin, rays, S, rf.CameraBounds(near, far), t_rand=k0)
    total = torch.nn.functional.l1_loss(spec, pixels) + torch.nn.functional.l1_loss(diff, pixels) + weight * L
    total.backward()
    np.testing.assert_allclose(float(stats.distortion) / n, float(L), rtol=1e-5)
    for got, want in ((gd, twin.densities.grad), (gf, twin.features.grad)):
        err = (got - want).abs()
        assert float(err.max()) <= 1e-6 + 1e-3 * float(want.abs().max()), float(err.max())
    # ... and the term took part: the render gradients alone are somewhere else
    twin.densities.grad = None
    (weight * rf.distortion_loss(twin, rays, S, rf.CameraBounds(near, far), t_rand=k0)).backward()
    assert float(twin.densities.grad.abs().max()) > 1e-2 * float(gd.abs().max())
    stepper.flat.detach()


def _model(dev, storage="split", F=27, G=16):
    dens, feat = procedural_grid((G, G, G), F, 3)
    grid = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(3.0 / G, 3.0 / G, 3.0 / G), density_preactivation=torch.nn.Identity(),
                        density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, tunable=True, storage=storage)
    cfg = rf.SHVoxGridRenderConfig(16, rf.CameraBounds(1.8, 6.6), perturb_sampled_points=False, white_bkgd=True)
    return rf.VolumetricModel(grid, rf.render_sh_voxel_grid, cfg, device=dev)


def test_options_that_cannot_hold_a_gradient_bucket_raise(hip_device):
    with pytest.raises(ValueError, match="fuse_optimizer"):
        TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, distortion_weight=0.1, fuse_optimizer=True)
    with pytest.raises(ValueError, match="owner"):
        TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, distortion_weight=0.1, exchange="owner")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TrainStepper(_model(hip_device), 64, 0.03, data_parallel=False, distortion_weight=bad)


@pytest.mark.parametrize("storage,fused", [("split", True), ("bricked", True), ("reference", True), ("reference", False), ("split", False)])
def test_zero_weight_resolves_every_option_as_before(hip_device, monkeypatch, storage, fused):
    plain = TrainStepper(_model(hip_device, storage), 64, 0.03, data_parallel=False, fused=fused)
    plain.flat.detach()
    zero = TrainStepper(_model(hip_device, storage), 64, 0.03, data_parallel=False, fused=fused, distortion_weight=0.0)
    for name in ("fuse_optimizer", "brick_size", "exchange", "merged_bricks", "backward"):
        assert getattr(zero, name) == getattr(plain, name), name
    assert zero.flat.deferred == plain.flat.deferred and zero.flat.brick_size == plain.flat.brick_size
    if fused:
        assert zero.fuse_optimizer == (storage != "reference") and zero.exchange == "dense"
    else:
        assert zero.flat.deferred == (storage == "reference")

    def forbidden(*args, **kwargs):
        raise AssertionError("a distortion launch in a step with distortion_weight=0")

    monkeypatch.setattr(ops, "distortion_raw", forbidden)
    o = T(hash_uniform((64, 3), 41, 9.0, 10.0)).to(hip_device)
    d = T(hash_uniform((64, 3), 42, 0.5, 1.0)).to(hip_device)
    stats = zero.step_on(rf.Rays(o, d), missing_pixels(hip_device, 64))
    assert stats.distortion is None and zero._distortion_ring is None
    monkeypatch.undo()
    on = TrainStepper(_model(hip_device, storage), 64, 0.03, data_parallel=False, fused=fused, distortion_weight=1e-2)
    assert on.fuse_optimizer is False and on.flat.deferred is False and on.exchange == "dense"
    zero.flat.detach()
    on.flat.detach()


def test_cli_flag_round_trip(hip_device, tmp_path):
    """scripts/train_sh_based_voxel_grid.py --distortion_weight: the summary lines carry the term."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "scripts/train_sh_based_voxel_grid.py", "-o", str(tmp_path / "run"), "--grid_dims", "16", "16", "16", "--sh_degree", "0",
                        "--ray_batch_size", "512", "--render_num_samples_per_ray", "32", "--num_stages", "1", "--num_iterations_per_stage", "6",
                        "--save_frequency", "1000", "--test_frequency", "1000", "--summary_frequency", "3", "--distortion_weight", "0.01", "--synthetic", "True",
                        "--synthetic_size", "24", "--train_num_samples_per_ray", "32"], cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    values = [float(line.split("distortion: ")[1].split()[0]) for line in r.stdout.splitlines() if "distortion: " in line]
    assert len(values) >= 2 and all(np.isfinite(v) and v >= 0.0 for v in values)


def _gloo_worker(rank, world, port, result_dir):
    import os

    import torch.distributed as dist

    from tests.test_hip_data_parallel import R, _setup, _train

    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        data, model = _setup(dev, jitter=True)
        stepper = TrainStepper(model, R, learning_rate=0.03, global_batch=True, distortion_weight=0.5)
        assert stepper.exchange == "dense" and not stepper.fuse_optimizer
        dp = _train(stepper, data)
        data, model = _setup(dev, jitter=True)
        single = _train(TrainStepper(model, R, learning_rate=0.03, data_parallel=False, distortion_weight=0.5), data)
        data, model = _setup(dev, jitter=True)
        without = _train(TrainStepper(model, R, learning_rate=0.03, data_parallel=False, fuse_optimizer=False), data)
        err, took_part = float((dp - single).abs().max()), float((single - without).abs().max())
        open(os.path.join(result_dir, f"ok{rank}"), "w").write(f"{err} {took_part}")
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_equal_the_single_process_step(hip_device, tmp_path):
    """Strong scaling (global_batch, keyed jitter with first_ray): two ranks with the term equal the single-process run at the bar
    of tests/test_hip_data_parallel.py (2e-4), and the term took part."""
    import os

    import torch.multiprocessing as mp

    from tests.test_hip_data_parallel import _free_port

    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        err, took_part = (float(v) for v in open(tmp_path / f"ok{rank}").read().split())
        assert err <= 2e-4 and took_part > 10 * 2e-4, (err, took_part)
