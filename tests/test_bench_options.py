"""bench.py's command line on the CPU: a plain run (`--gpus 1 --steps K --warmup W`) skips every reporting leg behind the headline,
`--full` runs them all at their usual sizes, and a leg given a count of its own runs at that count either way.  What a plain run
prints on a GPU is tests/test_hip_widening.py::test_bench_plain_run_skips_the_reporting_legs."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("render_frames", "highres_frames", "dropin_steps", "windows", "second_point_rays", "train256_steps", "cpu_rays")


def _parse(*argv):
    """bench.parse_args in a child process (importing bench sets OMP_NUM_THREADS for the process that imports it)"""
    code = f"import json, bench; a = bench.parse_args({list(argv)!r}); print(json.dumps({{'args': vars(a), 'full': bench.FULL_LEGS}}))"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for name in ("WORLD_SIZE", "RANK", "RF_BENCH_WORKER"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    return out["args"], out["full"]


def test_plain_run_skips_the_reporting_legs():
    args, full = _parse("--gpus", "1", "--steps", "20", "--warmup", "5")
    assert sorted(full) == sorted(LEGS)
    assert args["full"] is False and args["steps"] == 20 and args["warmup"] == 5
    for name in LEGS:
        assert args[name] == 0, name
    assert args["timed_steps"] == 5  # (recorded inside the timed steps: the same in both modes)


def test_full_runs_every_leg_and_an_explicit_count_wins():
    args, full = _parse("--gpus", "1", "--steps", "20", "--warmup", "5", "--full")
    assert args["full"] is True
    for name in LEGS:
        assert args[name] == full[name] > 0, name
    assert full["windows"] == 9 and full["train256_steps"] == 10 and full["cpu_rays"] == 2048
    args, _ = _parse("--steps", "3", "--full", "--windows", "1", "--cpu-rays", "0")
    assert args["windows"] == 1 and args["cpu_rays"] == 0 and args["render_frames"] == full["render_frames"]
    args, _ = _parse("--steps", "3", "--render-frames", "2")
    assert args["render_frames"] == 2 and all(args[name] == 0 for name in LEGS if name != "render_frames")
