"""bench.py's multi-rank plumbing on the CPU (QVIT_BENCH_DRYRUN=1: gloo, stand-in per-image model).

`python bench.py --gpus N` without a launcher must start N ranks itself and rank 0 must print one
JSON line with n_gpus == N and the global batch N * batch; a launcher whose WORLD_SIZE disagrees
with --gpus is an error (VERDICT r01 Missing #1)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=240):
    env = dict(os.environ, QVIT_BENCH_DRYRUN="1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          env=env, timeout=timeout, cwd=ROOT)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_bench_gpus_flag_launches_n_ranks(n):
    r = _run(["--gpus", str(n), "--steps", "3", "--warmup", "1", "--batch", "4"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    j = json.loads(lines[0])
    assert j["n_gpus"] == n
    assert j["config"]["global_batch"] == 4 * n
    assert j["config"]["parallelism"] == f"dp{n}"
    assert j["steps"] == 3 and j["value"] > 0 and j["scaling"] == "weak"


def test_dump_outputs_is_repeatable_and_plain_line_is_lean(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float32 .npy, identical from run to run; a plain
    run's line carries the headline fields and nothing that --full alone measures."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        assert os.listdir(tmp_path / d) == ["logits.npy"]
        got.append(np.load(tmp_path / d / "logits.npy"))
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert got[0].dtype == np.float32 and got[0].shape == (4, 10)
    assert np.array_equal(got[0], got[1])
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["unit"] == "img/s" and j["higher_is_better"] is True
    assert abs(j["value"] - 4 / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
    assert not {"cpu_baseline", "parity", "gather_check"} & set(j)


def test_dump_outputs_samples_a_large_output(tmp_path, monkeypatch):
    """An output over the size limit is stored as the same seeded sample of its elements every time."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    t = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"big": t, "small": t[:2].double()})
    bench.dump_outputs(str(tmp_path / "b"), {"big": t.clone(), "small": t[:2].double()})
    big, small = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "small.npy")
    assert big.dtype == np.float32 and big.shape == (500,) and (np.diff(big) > 0).all()   # 2000 B share, no repeats
    assert small.dtype == np.float64 and np.array_equal(small, t[:2].numpy())
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))
    assert big.nbytes + small.nbytes <= 4000


def test_bench_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"],
             extra_env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in (r.stderr + r.stdout)


def test_metric_names_the_workload_run():
    """The headline workload carries BASELINE.json's metric verbatim; any other workload names itself."""
    import json
    import os
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "BASELINE.json")) as f:
        base = json.load(f)
    assert bench.metric_for("vit_base_patch16_224", 224, 256) == bench.METRIC == base["metric"]
    m = bench.metric_for("vit_large_patch16_384", 384, 128)
    assert "vit_large_patch16_384" in m and "batch 128" in m and m != bench.METRIC
