"""bench.py --dump-outputs: the fused image of the last timed step, written as float32 .npy files (a fixed, seeded sample
when it would not fit in 64 MB), identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-1500:] + r.stderr[-3000:]
    return json.loads(lines[-1])


def test_dry_run_dump_is_the_result_and_repeats(tmp_path, oracle):
    outs = []
    for k in range(2):
        d = _bench(["--dry-run", "--steps", "3", "--warmup", "1", "--frames", "6", "--dump-outputs", str(tmp_path / f"run{k}")], 280)
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["verified"] is True
        assert d["dump_outputs"]["files"] == {"fused": {"shape": [96, 128, 3], "dtype": "uint8"}}
        outs.append(np.load(tmp_path / f"run{k}" / "fused.npy"))
    assert outs[0].dtype == np.float32 and np.array_equal(outs[0], outs[1])
    so = oracle.StreamingOracle(96, 128, np.uint8, min_size=16, arith="separable")
    for f in range(6):
        so.push_frame(oracle.synth_frame_numpy(96, 128, f, 6))
    assert np.array_equal(outs[0], so.finish().astype(np.float32))


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "0"], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_of_a_large_output_is_a_fixed_sample(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 500)
    a = np.random.default_rng(3).integers(0, 65536, (40, 30, 3), dtype=np.uint16)
    info = [bench.dump_outputs(str(tmp_path / f"d{k}"), {"fused": a}) for k in range(2)]
    assert info[0]["bytes"] == 2000 <= 4000 and "sample" in info[0]["files"]["fused_sample"]
    s0, s1 = (np.load(tmp_path / f"d{k}" / "fused_sample.npy") for k in range(2))
    assert s0.dtype == np.float32 and s0.shape == (500,) and np.array_equal(s0, s1)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(a.size, 500, replace=False))
    assert np.array_equal(s0, a.ravel()[idx].astype(np.float32))


SIDE_PARTS = ("no_verify", "no_other_mode", "no_other_dtypes", "no_projection", "no_cpu_baseline")


def test_plain_run_leaves_the_side_parts_to_full(monkeypatch):
    """a plain run does only what the headline needs; --full switches every side part on, and --no-* still picks parts off"""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and all(getattr(a, k) for k in SIDE_PARTS)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert a.full and not any(getattr(a, k) for k in SIDE_PARTS)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.no_cpu_baseline and not any(getattr(a, k) for k in SIDE_PARTS if k != "no_cpu_baseline")


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline(tmp_path, oracle):
    """without --full the line carries the headline and what the timed steps recorded, no side measurement; the dumped
    image is the same one --full verifies"""
    H, W, N = 600, 900, 8
    d = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", str(N), "--height", str(H), "--width", str(W),
                "--dump-outputs", str(tmp_path)], 600)
    assert d["metric"] == "Mpixels/s fused (pyramid build+select+collapse)" and d["unit"] == "Mpixels/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and abs(d["value"] - N * H * W / d["ms_per_step"] / 1e3) <= 1e-6 * d["value"]
    assert d["roofline"]["launches"] > 0 and d["breakdown_ms_per_step"]
    for k in ("verified", "verify", "other_mode", "other_dtypes", "projected_scaling", "shard_step", "cpu_baseline", "cv2"):
        assert k not in d, k
    got = np.load(tmp_path / "fused.npy")
    so = oracle.StreamingOracle(H, W, np.uint8, arith="separable")
    for f in range(N):
        so.push_frame(oracle.synth_frame_numpy(H, W, f, N))
    assert np.array_equal(got, so.finish().astype(np.float32))


@pytest.mark.gpu
def test_bench_dump_on_gpu_equals_the_oracle(tmp_path, oracle):
    """the timed path's own result (separable arithmetic, float-32 frames resident in HBM) == its CPU oracle"""
    H, W, N = 600, 900, 8
    d = _bench(["--full", "--steps", "2", "--warmup", "1", "--frames", str(N), "--height", str(H), "--width", str(W),
                "--no-other-mode", "--no-cpu-baseline", "--no-projection", "--no-other-dtypes", "--dump-outputs", str(tmp_path)], 600)
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["verified"] is True
    got = np.load(tmp_path / "fused.npy")
    so = oracle.StreamingOracle(H, W, np.uint8, arith="separable")
    for f in range(N):
        so.push_frame(oracle.synth_frame_numpy(H, W, f, N))
    assert got.dtype == np.float32 and np.array_equal(got, so.finish().astype(np.float32))
