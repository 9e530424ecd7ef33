"""Float64 model of the whole regularised training iteration, composed from the models the suite already has (no new arithmetic):

    L(D, F) = mean|C_spec - P| + mean|C_diff - P| + lambda_dist (1/n) sum_r l_r(D) + lambda_D TV_density(D) + lambda_F TV_features(F)

C_spec / C_diff: oracle.relu_field_oracle.render in float64 (white background; render_diffuse for the second) with the jitter tables
of the two renders; l_r and its density gradient: tests.distortion_model.model on the SPECULAR render's jitter table; the TV terms:
tests.tv_model.tv_loss_and_grad.  Keyed jitter is restated as a table (orc.keyed_jitter) from the keys ops.draw_jitter_key() draws
after torch.manual_seed, in the order of the step path under test.

Per element the bar is assembled only from bars the project already states:

    bar = sum over {specular + diffuse render, distortion} of (GRAD_RTOL |g_term| + GRAD_ATOL max|g_term|) + tv_model.grad_bound(w)

(GRAD_RTOL = 5e-4, GRAD_ATOL = 5e-6: the grid-gradient bar of tests/test_hip_parity.py and tests/distortion_model.py; w: the TV weight
of the tensor's elements, tv_model.element_weights)."""
import functools

import numpy as np
import torch

from oracle import relu_field_oracle as orc
from tests import distortion_model as dm
from tests import tv_model
from tests.helpers import hash_uniform, procedural_grid

GRAD_RTOL, GRAD_ATOL = dm.GRAD_RTOL, dm.GRAD_ATOL
RHO = 100.0 / 3.0
NUM_RAYS = 130
LR = 0.01
TV_EPSILON = 1e-8
WEIGHTS = {"distortion_weight": 1.0, "tv_density_weight": 0.1, "tv_feature_weight": 0.1}
SEED = 7700  # torch.manual_seed(SEED + iteration) precedes every iteration of the GPU tests
STEPS = 3
PARAM_ROUNDING = 1e-7  # the float32 parameters' own roundings over the steps (as adam_reference() of tests/test_hip_distortion.py)

CASES = {
    "A": {"dims": (9, 8, 17), "voxel": dm.voxel_of((9, 8, 17)), "location": (0.0, 0.0, 0.0), "F": 27, "S": 24},
    # as tightening leaves a grid: non-cubic dims, anisotropic voxels, off-centre
    "B": {"dims": (10, 13, 7), "voxel": (0.21, 0.17, 0.26), "location": (0.15, -0.1, 0.2), "F": 3, "S": 65},
}


def case_aabb(name):
    c = CASES[name]
    return orc.make_aabb(c["dims"], c["voxel"], c["location"])


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(densities, features, origins, directions, near, far, pixels) of a case: float32 tensors, never modified.  The rays are those
    of test_stepper_gradient_equals_the_autograd_sum_of_renders_and_distortion_loss: 67 camera rays plus 63 of them with longer
    directions."""
    c = CASES[name]
    dens, feat = procedural_grid(c["dims"], c["F"], 61)
    cam_o, cam_d, near, far = dm.case_rays(67, c["S"])
    o = torch.cat([cam_o, cam_o[:63]]).contiguous()
    d = torch.cat([cam_d, cam_d[:63] * 1.01]).contiguous()
    pixels = torch.from_numpy(hash_uniform((NUM_RAYS, 3), 43, 0.0, 1.0))
    return dens, feat, o, d, float(np.float32(near)), float(np.float32(far)), pixels


def draw_keys(seed, count=2, selection=False):
    """The 64-bit keys a step draws from torch's CPU generator after torch.manual_seed(seed): (selection key or None, jitter keys).
    Every step path draws the specular render's key, then the diffuse render's; TrainStepper.step() draws the batch's key first."""
    from thr3ed_atom_amd import ops

    torch.manual_seed(seed)
    sel = int(torch.randint(-(2**63), 2**63 - 1, (1,), dtype=torch.int64).item()) if selection else None
    return sel, [ops.draw_jitter_key() for _ in range(count)]


def jitter_tables(keys, n, S, first_ray=0):
    return [torch.from_numpy(orc.keyed_jitter(k, first_ray, n, S).astype(np.float32)) for k in keys]


def objective(dens, feat, aabb, o, d, near, far, S, pixels, t_spec, t_diff, weights=None, tv_epsilon=TV_EPSILON, rho=RHO):
    """One evaluation of L at (dens, feat) (reference layout; float32 or float64 tensors).  Returns a dict:
    ``terms``: name -> (value, gd [X,Y,Z,1], gf [X,Y,Z,F]) float64, names "render", "distortion", "tv";
    ``specular_loss`` / ``diffuse_loss`` / ``distortion_sum`` (sum_r l_r) / ``distortion_bar`` (sum_r loss_bar) / ``tv_density`` /
    ``tv_features``: what StepStats reports; ``gd`` / ``gf``: the gradient of L; ``bar_d`` / ``bar_f``: the per-element bar;
    ``band``: ReLU band count of distortion_model on the samples of the specular and of the diffuse render."""
    w = WEIGHTS if weights is None else weights
    n = o.shape[0]
    D = dens.detach().double().clone().requires_grad_(True)
    F = feat.detach().double().clone().requires_grad_(True)
    P = pixels.double()
    losses = []
    for diffuse, t in ((False, t_spec), (True, t_diff)):
        r = orc.render(D, F, o.double(), d.double(), aabb, near, far, S, rho, "relu", white_bkgd=True, render_diffuse=diffuse,
                       t_rand=None if t is None else t.double())
        losses.append((r["colour"] - P).abs().mean())
    rd, rf_ = torch.autograd.grad(losses[0] + losses[1], (D, F))
    dist = dm.model(D.detach(), aabb, rho, "relu", o, d, near, far, S, t_rand=t_spec)
    band_diffuse = dm.model(D.detach(), aabb, rho, "relu", o, d, near, far, S, t_rand=t_diff, want_grad=False)["band"]
    dist_gd = torch.from_numpy(w["distortion_weight"] / n * dist["grad"])[..., None]
    tv_value, tvd, tvf = tv_model.tv_loss_and_grad(D, F, w["tv_density_weight"], w["tv_feature_weight"], tv_epsilon)
    tv_d, tv_f = tv_model.tv_values(D, F, tv_epsilon)
    terms = {
        "render": (float((losses[0] + losses[1]).detach()), rd, rf_),
        "distortion": (w["distortion_weight"] * float(dist["loss"].mean()), dist_gd, torch.zeros_like(rf_)),
        "tv": (tv_value, tvd, tvf),
    }
    wd, wf = tv_model.element_weights(tuple(D.shape[:3]), F.shape[-1], w["tv_density_weight"], w["tv_feature_weight"])
    bar_d = torch.full_like(rd, tv_model.grad_bound(wd))
    bar_f = torch.full_like(rf_, tv_model.grad_bound(wf))
    for name in ("render", "distortion"):
        _, gd, gf = terms[name]
        bar_d = bar_d + GRAD_RTOL * gd.abs() + GRAD_ATOL * gd.abs().max()
        bar_f = bar_f + GRAD_RTOL * gf.abs() + GRAD_ATOL * gf.abs().max()
    return {
        "terms": terms, "specular_loss": float(losses[0].detach()), "diffuse_loss": float(losses[1].detach()), "distortion_sum": float(dist["loss"].sum()),
        "distortion_bar": float(dm.loss_bar(dist["spread"]).sum()), "tv_density": tv_d, "tv_features": tv_f,
        "gd": sum(t[1] for t in terms.values()), "gf": sum(t[2] for t in terms.values()), "bar_d": bar_d, "bar_f": bar_f,
        "band": (dist["band"], band_diffuse), "value": sum(t[0] for t in terms.values()),
    }


def case_objective(name, dens, feat, keys, o=None, d=None, pixels=None, first_ray=0):
    """objective() of a case at the given parameters with the keyed jitter of ``keys`` = (specular key, diffuse key)"""
    c = CASES[name]
    _, _, o0, d0, near, far, p0 = case_inputs(name)
    o, d, pixels = (o0 if o is None else o), (d0 if d is None else d), (p0 if pixels is None else pixels)
    t_spec, t_diff = jitter_tables(keys, o.shape[0], c["S"], first_ray)
    return objective(dens, feat, case_aabb(name), o, d, near, far, c["S"], pixels, t_spec, t_diff)


def adam_steps(dens, feat, evaluate, steps, lr=LR):
    """``steps`` iterations of torch.optim.Adam(betas=(0.9, 0.999)) in float64 on L; ``evaluate(D, F, t)`` is the objective() of step t
    (a fresh pair of jitter tables per step).  Returns a dict: ``dens`` / ``feat`` the final parameters; ``bar_d`` / ``bar_f`` the
    per-element Adam bar sum_t min(2 lr, 4 lr bar_t / |g_t|) (+ the float32 parameters' own rounding) -- the rule adam_reference() of
    tests/test_hip_distortion.py derives: the update is homogeneous of degree 0 in the gradients and bounded by lr, so a relative
    gradient error rho moves it by at most 2 lr rho, and the earlier steps' parameter error feeds back (a factor 2); ``zero_d`` /
    ``zero_f`` the elements whose float64 gradient is exactly 0 in every step; ``evals`` the per-step objective() dicts."""
    D = dens.detach().double().clone().requires_grad_(True)
    F = feat.detach().double().clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [D, F], "lr": lr}], betas=(0.9, 0.999))
    bars = [torch.zeros_like(D), torch.zeros_like(F)]
    zeros = [torch.ones_like(D, dtype=torch.bool), torch.ones_like(F, dtype=torch.bool)]
    evals = []
    for t in range(steps):
        ev = evaluate(D.detach(), F.detach(), t)
        evals.append(ev)
        for i, (g, bar) in enumerate(((ev["gd"], ev["bar_d"]), (ev["gf"], ev["bar_f"]))):
            rho = torch.where(g == 0, torch.full_like(g, float("inf")), bar / g.abs())
            bars[i] += torch.minimum(torch.full_like(g, 2 * lr), 4 * lr * rho)
            zeros[i] &= g == 0
        D.grad, F.grad = ev["gd"].clone(), ev["gf"].clone()
        opt.step()
    return {"dens": D.detach(), "feat": F.detach(), "bar_d": bars[0] + PARAM_ROUNDING, "bar_f": bars[1] + PARAM_ROUNDING, "zero_d": zeros[0],
            "zero_f": zeros[1], "evals": evals}


def step_keys(step):
    """(specular key, diffuse key) of iteration ``step`` of the GPU tests (torch.manual_seed(SEED + step) precedes it)"""
    return draw_keys(SEED + step)[1]


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """adam_steps() of a case over STEPS iterations with the keys of the GPU tests -- computed once, never modified"""
    dens, feat = case_inputs(name)[:2]
    return adam_steps(dens, feat, lambda D, F, t: case_objective(name, D, F, step_keys(t)), STEPS)


# --------------------------------------------------------------------------------------------
# the trainer's own path: TrainStepper.step(dataset, image_ids) draws the batch with a key of its own
# --------------------------------------------------------------------------------------------
BATCH_SEED = 7800
BATCH_HW = 12
BATCH_FOCAL = 10.75
BATCH_VIEWS = [(40.0, -35.0), (160.0, -20.0), (280.0, -50.0)]  # (yaw, pitch) of pose_spherical
BATCH_IMAGE_IDS = (2, 0, 1)


@functools.lru_cache(maxsize=None)
def trainer_dataset():
    """(images [3, 3, 12, 12] in [0, 1), poses [3, 3, 4]) of the three views, float32, never modified"""
    from tests.helpers import hotdog_like_camera
    from thr3ed_atom_amd.camera import pose_spherical

    radius = hotdog_like_camera()["radius"]
    poses = [pose_spherical(yaw, pitch, radius) for yaw, pitch in BATCH_VIEWS]
    pose_mat = torch.stack([torch.cat([torch.as_tensor(p.rotation), torch.as_tensor(p.translation)], dim=1) for p in poses]).to(torch.float32)
    images = torch.from_numpy(hash_uniform((len(poses), 3, BATCH_HW, BATCH_HW), 47, 0.0, 1.0))
    return images, pose_mat


@functools.lru_cache(maxsize=None)
def trainer_batch():
    """The batch TrainStepper.step(dataset, BATCH_IMAGE_IDS) draws after torch.manual_seed(BATCH_SEED), rebuilt independently: the
    selection key replayed from the seed, orc.keyed_permutation over the 3 x 144 pixels, orc.cast_rays per image, the pixel table.
    Returns (origins, directions, pixels, (specular key, diffuse key))."""
    images, pose_mat = trainer_dataset()
    key, jitter_keys = draw_keys(BATCH_SEED, selection=True)
    hw = BATCH_HW * BATCH_HW
    index = orc.keyed_permutation(np.arange(NUM_RAYS), len(BATCH_IMAGE_IDS) * hw, key)
    image = np.asarray(BATCH_IMAGE_IDS)[index // hw]
    within = index % hw
    table = images.permute(0, 2, 3, 1).reshape(len(images), hw, 3)
    rays = [orc.cast_rays(BATCH_HW, BATCH_HW, BATCH_FOCAL, pose_mat[i, :, :3], pose_mat[i, :, 3]) for i in range(len(images))]
    o = torch.stack([rays[i][0].reshape(-1, 3)[j] for i, j in zip(image, within)]).contiguous()
    d = torch.stack([rays[i][1].reshape(-1, 3)[j] for i, j in zip(image, within)]).contiguous()
    pixels = torch.stack([table[i, j] for i, j in zip(image, within)]).contiguous()
    return o, d, pixels, tuple(jitter_keys)


@functools.lru_cache(maxsize=None)
def trainer_batch_objective(name):
    """objective() of a case's start parameters on the trainer's own batch -- computed once, never modified"""
    dens, feat = case_inputs(name)[:2]
    o, d, pixels, keys = trainer_batch()
    return case_objective(name, dens, feat, keys, o, d, pixels)


def exceeds(a, b):
    """share of the elements of ``a`` whose magnitude is above ``b``"""
    return float((a.abs() > b).double().mean())


def worst_ratio(got, want, bar):
    """largest |got - want| / bar over EVERY element (got: a float32 tensor on any device)"""
    return float(((got.detach().double().cpu() - want).abs() / bar).max())
