"""bench.py --dump-outputs without a GPU: what dump_outputs writes (float32 /
float64 files, at most 64 MB in all, the same seeded row sample every time)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float_arrays_unchanged(tmp_path):
    import bench
    nodes = np.random.default_rng(0).normal(size=(1000, 4))
    active = (np.arange(1000) % 3 == 0).astype(np.uint8)
    stats = np.array([[3, 40, 1234, 17, 0]], dtype=np.float64)
    bench.dump_outputs(str(tmp_path), dict(nodes=nodes, active=active, loop_stats=stats))
    assert sorted(os.listdir(str(tmp_path))) == ["active.npy", "loop_stats.npy", "nodes.npy"]
    got = np.load(str(tmp_path / "nodes.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, nodes)
    got = np.load(str(tmp_path / "active.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, active)
    assert np.array_equal(np.load(str(tmp_path / "loop_stats.npy")), stats)


def test_dump_outputs_samples_the_same_rows_above_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 1024)
    big = np.arange(40000, dtype=np.float64).reshape(10000, 4)    # 320 KB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), dict(big=big))
    a = np.load(str(tmp_path / "a" / "big.npy"))
    b = np.load(str(tmp_path / "b" / "big.npy"))
    assert a.nbytes <= 64 * 1024 and a.shape[1] == 4 and a.shape[0] > 0
    assert np.array_equal(a, b)
    rows = a[:, 0].astype(np.int64) // 4
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, big[rows])
