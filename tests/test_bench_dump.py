"""bench.py --dump-outputs on the host side: what is written, in which type, and the seeded row sample that keeps a large output
under the size limit (the GPU run itself is tests/test_gpu_parity.py::test_plain_bench_run_times_its_steps_and_dumps_the_last_step)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    x = np.arange(12.0).reshape(4, 3)
    st = np.array([0, 2, 0, 0], dtype=np.int32)
    bench.dump_outputs({"x": x, "status": st}, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["status.npy", "x.npy"]
    a, s = np.load(tmp_path / "x.npy"), np.load(tmp_path / "status.npy")
    assert a.dtype == np.float64 and np.array_equal(a, x)
    assert s.dtype == np.float64 and np.array_equal(s, st)


def test_large_outputs_keep_the_same_seeded_rows_under_the_limit(tmp_path):
    rng = np.random.default_rng(7)
    arrays = {"x": rng.standard_normal((1000, 50)), "kkt": rng.standard_normal(1000)}
    limit = 100_000                      # the arrays hold 408 000 bytes
    for d in ("a", "b"):
        bench.dump_outputs(arrays, str(tmp_path / d), limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["kkt.npy", "kkt_rows.npy", "x.npy", "x_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    for name in ("x", "kkt"):
        rows = np.load(tmp_path / "a" / (name + "_rows.npy"))
        assert np.array_equal(rows, np.load(tmp_path / "b" / (name + "_rows.npy")))
        assert len(rows) > 0 and np.all(np.diff(rows) > 0)
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), arrays[name][rows.astype(np.int64)])
