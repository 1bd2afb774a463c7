"""bench.py --dump-outputs: float32 .npy files, and above the size budget the same seeded rows in every run."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_float32(tmp_path):
    bench = _bench()
    x = np.arange(12, dtype=np.uint8).reshape(3, 4)
    bench.dump_outputs(SimpleNamespace(dump_outputs=str(tmp_path / "d")), 0, {"x": x, "flags": np.array([0, 1, 0])})
    assert sorted(os.listdir(tmp_path / "d")) == ["flags.npy", "x.npy"]
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x)
    assert np.load(tmp_path / "d" / "flags.npy").shape == (3, 1)


def test_dump_outputs_samples_the_same_rows_within_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    x = np.random.default_rng(3).integers(0, 256, (200, 64), dtype=np.uint8)  # 51200 B as float32
    for name in ("a", "b"):
        bench.dump_outputs(SimpleNamespace(dump_outputs=str(tmp_path / name)), 0, {"x": x})
    rows = np.load(tmp_path / "a" / "x_rows.npy")
    got = np.load(tmp_path / "a" / "x.npy")
    assert got.nbytes <= 4096 and len(rows) == len(got) == 16
    assert np.array_equal(got, x[rows.astype(int)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "x_rows.npy"))
    assert np.array_equal(got, np.load(tmp_path / "b" / "x.npy"))


def test_dump_outputs_only_on_rank_0_and_when_asked(tmp_path):
    bench = _bench()
    bench.dump_outputs(SimpleNamespace(dump_outputs=None), 0, {"x": np.zeros((2, 2))})
    bench.dump_outputs(SimpleNamespace(dump_outputs=str(tmp_path / "r1")), 1, {"x": np.zeros((2, 2))})
    assert not (tmp_path / "r1").exists()


def test_full_and_dump_outputs_are_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--full", "--dump-outputs", "unused", "--dry-run"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
