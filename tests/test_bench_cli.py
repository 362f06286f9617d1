"""bench.py's command line: a plain run times exactly --steps steps, and --dump-outputs writes what the timed path returned
(float32 .npy files, < 64 MB in all, the same sample of rows for the same shape)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _bench(args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=_env(), capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    return r, [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def test_plain_run_times_exactly_k_steps():
    """no pilot block and no 50 ms rule by default: K steps of 1 ms give a timed region of exactly K steps"""
    r, lines = _bench(["--gpus", "1", "--steps", "7", "--warmup", "2", "--stub-step-ms", "1"])
    assert r.returncode == 0, r.stderr
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 7 and line["timed_steps"] == 7 and line["warmup"] == 2
    assert 0.9 <= line["ms_per_step"] <= 50.0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert "roofline" not in line and "cpu_baseline" not in line and "backward" not in line


def test_full_is_an_option():
    r, lines = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--stub-step-ms", "1", "--full"])
    assert r.returncode == 0, r.stderr
    assert len(lines) == 1 and lines[0]["timed_steps"] == 3


def test_dump_outputs_small_tensor_is_written_whole(tmp_path):
    import bench
    o = torch.randn(2, 2, 128, 32, dtype=torch.bfloat16)
    shapes = bench.dump_outputs({"out": o}, str(tmp_path))
    a = np.load(tmp_path / "out.npy")
    assert shapes == {"out": [2, 2, 128, 32]} and a.dtype == np.float32
    assert np.array_equal(a, o.float().numpy())


def test_dump_outputs_large_tensors_are_a_fixed_sample_below_64_mb(tmp_path):
    """four outputs of the (8,16,4096,64) shape (268 MB as float32) - the sample is the same rows every time"""
    import bench
    shape, nrows = (8, 16, 4096, 64), 8 * 16 * 4096
    outs = {}
    for i, nm in enumerate(("out", "dq", "dk", "dv")):
        t = torch.arange(64, dtype=torch.float32).repeat(nrows, 1) + 100 * i   # columns 1..63: j + 100 i
        t[:, 0] = torch.arange(nrows, dtype=torch.float32)                     # column 0: the row index
        outs[nm] = t.reshape(shape)
    bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    total = 0
    for i, nm in enumerate(outs):
        pa, pb = tmp_path / "a" / f"{nm}.npy", tmp_path / "b" / f"{nm}.npy"
        total += os.path.getsize(pa)
        a, b = np.load(pa), np.load(pb)
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 64 and a.shape[0] > 10000
        assert np.array_equal(a, b)
        assert np.all(np.diff(a[:, 0]) > 0) and a[-1, 0] < nrows   # distinct rows, in order
        assert np.array_equal(a[:, 1:], np.broadcast_to(np.arange(1, 64, dtype=np.float32) + 100 * i, (a.shape[0], 63)))   # whole rows
    assert total < 64_000_000


@pytest.mark.gpu
def test_dump_outputs_of_a_gpu_run_match_the_front_end(tmp_path, pkg, dev):
    """a plain run of C2 (8,16,1024,64) bf16 forward: out.npy is the sampled output of flash_attention_n on the same seeded inputs"""
    import bench
    from flash_attention_softmax_n_amd import synth
    r, lines = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c2", "--dump-outputs", str(tmp_path / "d")])
    assert r.returncode == 0, r.stderr
    assert len(lines) == 1 and lines[0]["timed_steps"] == 3 and lines[0]["ms_per_step"] > 0
    B, H, S, D, _, n, causal = bench.WORKLOADS["c2"]
    q, k, v = (synth.counter_normal((B, H, S, D), seed, dtype=torch.bfloat16, device=dev) for seed in (101, 102, 103))
    with torch.no_grad():
        o = pkg.flash_attention_n(q, k, v, softmax_n_param=n, is_causal=causal)
    bench.dump_outputs({"out": o}, str(tmp_path / "e"))
    got, want = np.load(tmp_path / "d" / "out.npy"), np.load(tmp_path / "e" / "out.npy")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-2   # the same kernel on the same inputs (a different launch order may round differently)
