"""A fixed replay of the randomised parity sweep (tests/parity_fuzz.py; `python -m tests.parity_fuzz` runs it open-ended): configurations
the parametrised tests do not enumerate -- grid dims 2..22 per axis, anisotropic voxels, off-centre grids, every SH degree / density
mode / storage, 1..150 samples, rays that start inside the volume, odd frame sizes, either frame kernel, the occupancy mask, either
adjoint -- against the oracle at the bars of tests/test_hip_parity.py.

The sweep found (round 6) what no enumerated case had: with a ray's LAST sample inside the volume -- its interval is 1e10 |d|
(reference accumulate.py:49-52) -- the adjoint's `1 - exp(-softplus)` slope and its `T (1 - alpha)` own term cancel to relative errors
of per cents on that sample's density gradient (softplus grids; the reference's autograd keeps exp(-x) and z / (z + 1)).  The cases that
showed it are replayed by name."""
import pytest
import torch

from tests import parity_fuzz

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run_seed,first", [(1, 0), (1, 40), (3, 0), (5, 0)])
def test_randomised_parity_sweep(hip_device, run_seed, first):
    for i in range(first, first + 40):
        parity_fuzz.run_case(run_seed, i, "all", hip_device)


def test_randomised_training_iterations(hip_device):
    """Two iterations of TrainStepper in randomly drawn set-ups (fused / autograd-driven, atomic / binned adjoint, cubic and 4 x 8 x 8
    bricks, Adam in the brick flush or from the bucket, every SH degree / density mode / storage, ragged batches, partial bricks) against
    the oracle's autograd + torch.optim.Adam."""
    for i in range(40):
        parity_fuzz.run_case(11, i, "train", hip_device)
    for i in range(12):  # grids of up to 72 nodes per axis: many bricks, partial ones on every axis
        parity_fuzz.run_case(301, i, "bigtrain", hip_device)


def test_randomised_small_entry_points(hip_device):
    """Point queries with their adjoint (bit-identical interpolation, points on the faces of the box), the stage transition at random
    size ratios (bit-identical to the restated ATen kernel), the keyed batch selection against its numpy restatement, frames with the
    in-kernel jitter cut into pixel ranges (bit-identical to the whole frame, either kernel) and against the oracle fed with the
    restated jitter table."""
    for i in range(60):
        parity_fuzz.run_case(21, i, "misc", hip_device)


def test_randomised_composed_renders(hip_device):
    """render_sh_voxel_grid with callables the fused kernels do not recognise (the default occupancy law / tone map re-stated under other
    names): the COMPOSED path -- rf_grid_query between torch ops, through autograd -- against the oracle, forward and gradients."""
    for i in range(40):
        parity_fuzz.run_case(71, i, "composed", hip_device)


def test_randomised_renders_through_the_reference_side_binding(hip_device):
    """integration/renderers_hip.py -- the file a maintainer adds to the reference -- on a module that has exactly the reference VoxelGrid's
    attributes: the render procedure, the pair procedure and the frame entry in random set-ups (both adjoint policies), against the oracle."""
    for i in range(60):
        parity_fuzz.run_case(101, i, "binding", hip_device)


@pytest.mark.parametrize("cases", [list(range(0, 24)), [28, 33, 49, 73, 222, 229, 257, 316, 364, 376]], ids=["first-24", "found"])
def test_rays_of_255_to_5000_samples(hip_device, cases):
    """Sample counts around the kernels' internal group sizes (64-sample chunks, 64 chunk masks = 4096 samples per mask group) and at
    the reference's default render count (render_num_samples_per_ray = 1024) and beyond, held to the float64-anchored bar: the HIP result
    may be as far from the float64 oracle as 3 x the float32 reference's own worst error of the batch + the bar.  The "found" cases are
    the ones the sweep failed on before the transmittance scan carried 1 - prod E beside prod E (slowly varying density: the doubling
    steps of a product scan round all lanes alike, 1e-5 of transmittance lost per 1000 samples) and before exp(-x) near 1 came from
    the series instead of v_exp_f32."""
    for i in cases:
        parity_fuzz.run_case(42, i, "long", hip_device)


def test_frames_of_256_to_5000_samples(hip_device):
    """Frames at high sample counts through either frame kernel (float64-anchored bar).  A packet lane adds its ray's weighted samples
    one after the other; at 4096+ samples that sequential float32 sum drifts 3..8e-5 on depth where torch.sum's pairwise order keeps
    the reference within 2e-6, so frames of more than 1024 samples per ray are dispatched to the per-ray kernel (the cases that showed
    it are among these)."""
    for i in [154, 320, 349, 397, 445, 469, 619] + list(range(0, 16)):
        parity_fuzz.run_case(201, i, "longframes", hip_device)


@pytest.mark.parametrize("run_seed,i,kind,mode", [(1, 138, "all", ""), (1, 268, "all", ""), (1, 284, "all", ""), (1, 292, "all", ""), (2, 251, "rays", "softplus")])
def test_last_sample_inside_the_volume_softplus_density_gradient(hip_device, run_seed, i, kind, mode):
    desc = parity_fuzz.run_case(run_seed, i, kind, hip_device, mode)
    assert "mode=softplus" in desc


@pytest.mark.parametrize("kind,run_seed,count", [("rays", 501, 40), ("frames", 502, 20), ("train", 503, 20), ("binding", 504, 20), ("long", 505, 8)])
def test_identity_densities(hip_device, kind, run_seed, count):
    """Identity/Identity densities (signed: negative occupancies where sigma delta < 0, transmittances above 1) in random set-ups of
    every kind that forms an occupancy: both adjoints, either frame kernel, rf_train_step with its forward / emit pair kernels and the
    brick pass (with and without Adam in the flush), the reference-side binding's Identity/Identity mapping, and 255..5000 samples per
    ray, where |sigma delta| is small on both sides and the transmittance scan runs on 1 - a with a < 0.  Rays whose last sample
    (interval 1e10 |d|) sits at a negative density, or whose transmittance exceeds 8, are left out (tests/parity_fuzz.py
    IDENTITY_STATS); most cases must keep rays, and many must reach sigma delta <= -0.5."""
    parity_fuzz.IDENTITY_STATS.clear()
    for i in range(count):
        desc = parity_fuzz.run_case(run_seed, i, kind, hip_device, "identity")
        assert "mode=identity" in desc
    stats = parity_fuzz.IDENTITY_STATS
    used = [s for s in stats if s[0] > 0]
    assert len(used) >= 0.75 * len(stats), stats
    if kind != "long":  # (hundreds of samples per ray: |sigma delta| stays small by construction)
        assert sum(s[2] <= -0.5 for s in used) >= 0.2 * len(used), stats
