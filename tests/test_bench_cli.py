"""bench.py's multi-rank launch (CPU, gloo): ``--gpus N`` without a torchrun environment must
start N ranks itself (one process each, as VSLURM:47's ``torchrun --nproc_per_node`` does) and
the gradient average they compute must be the rank mean -- the path the driver's N = 2/4/8
scaling runs take, here in ``--dry`` mode (stand-in gradient buffer, no GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=240):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, lines


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_flag_launches_that_many_ranks(n):
    p, lines = _run("--gpus", str(n), "--dry", "--steps", "2", "--warmup", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout  # rank 0 alone prints
    out = json.loads(lines[0])
    assert out["n_gpus"] == n
    assert out["grad_avg_ok"] is True and out["ranks_ok"] == [True] * n


def test_plain_run_is_the_default_and_full_is_opt_in():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--no-cpu", "--no-c3", "--dump-outputs", "d"])
    assert a.full is True and a.no_cpu and a.no_c3 and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_arrays_with_a_fixed_parameter_sample(tmp_path):
    """dump_outputs on a stand-in model (CPU): one float32 .npy per array, the parameter sample
    drawn at the same indices on every call, and far below the 64 MB a dump may take."""
    import numpy as np
    import torch
    import bench
    m = torch.nn.Linear(300, 70)
    logits = torch.arange(6.0).reshape(2, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(1.5), logits, m)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["logits", "loss", "params_sample"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].tolist() == [1.5] and np.array_equal(got["logits"], logits.numpy())
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    assert got["params_sample"].shape == (bench.PARAM_SAMPLE,) and np.isin(got["params_sample"], flat).all()
    assert np.array_equal(got["params_sample"], np.load(tmp_path / "b" / "params_sample.npy"))
    assert sum(v.nbytes for v in got.values()) <= 64 << 20


def test_single_rank_dry_run():
    p, lines = _run("--dry", "--steps", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(lines[-1])["n_gpus"] == 1
