"""CPU: bench.py's launch logic (the advisor's round-1 finding: `bench.py --gpus N` silently measured one GPU).

`python bench.py --gpus N` without a launcher must either start N ranks itself or refuse loudly; a WORLD_SIZE that disagrees with
--gpus must be an error, not a warning.  (The sharded path itself runs in tests/test_dist_cpu.py on gloo and, on the GPU box, in
tests/test_dist_gpu.py with two ranks on the leased GPU.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)


def test_more_gpus_than_visible_is_refused_before_any_gpu_call():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two GPUs visible")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 2 and "GPU(s) visible" in r.stderr and r.stdout.strip() == ""


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


def test_steps_below_one_is_refused():
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout.strip() == ""


def test_dump_outputs_writes_float64_and_samples_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    J, u0 = np.arange(1000, dtype=np.float64), np.arange(2000, dtype=np.float64).reshape(2, 1000)
    st = np.zeros(1000, dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "all"), {"J_T": J, "u0": u0, "status": st})
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in ("J_T", "u0", "status")}
    assert all(a.dtype == np.float64 for a in got.values()) and not (tmp_path / "all" / "sample_index.npy").exists()
    assert np.array_equal(got["J_T"], J) and np.array_equal(got["u0"], u0) and np.array_equal(got["status"], st)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"J_T": J, "u0": u0, "status": st})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["J_T.npy", "sample_index.npy", "status.npy", "u0.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 8000 + 4 * 128          # (+ the .npy headers)
    idx = np.load(tmp_path / "a" / "sample_index.npy").astype(np.int64)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy").astype(np.int64))   # the same sample every run
    assert len(idx) > 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "J_T.npy"), J[idx]) and np.array_equal(np.load(tmp_path / "a" / "u0.npy"), u0[:, idx])
