"""bench.py without a GPU: what --dump-outputs writes for a step's result, and what a plain run (no --full) leaves out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import polars_amd as pl  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_a_group_by_result_in_canonical_order(tmp_path):
    """A Q1-shaped result (to_dict: lists, keys as strings, a null) comes out as float64 arrays, rows sorted by the columns left to right, whatever
    order the groups came in."""
    res = {"l_returnflag": ["R", "A", "N", "N"], "l_linestatus": ["F", "F", "O", "F"], "sum_qty": [3, 1, 2, 5], "avg_disc": [0.25, 0.5, None, 0.75]}
    bench.dump_outputs(pl, res, str(tmp_path / "a"))
    shuffled = {k: [v[i] for i in (2, 0, 3, 1)] for k, v in res.items()}
    bench.dump_outputs(pl, shuffled, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(res) and all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["l_returnflag"], [0, 1, 1, 2]) and np.array_equal(a["l_linestatus"], [0, 0, 1, 0])
    assert np.array_equal(a["sum_qty"], [1, 5, 2, 3]) and np.array_equal(a["avg_disc"], [0.5, 0.75, np.nan, 0.25], equal_nan=True)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_dump_outputs_samples_a_large_result_the_same_way_every_time(tmp_path):
    n, cap = 1_000_000, 800_000
    res = {"x": np.arange(n, dtype=np.int64), "y": np.arange(n, dtype=np.float64) * 0.5}
    bench.dump_outputs(pl, res, str(tmp_path / "a"), max_bytes=cap)
    bench.dump_outputs(pl, res, str(tmp_path / "b"), max_bytes=cap)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= cap and 0 < len(a["x"]) < n
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], a["x"] * 0.5)
    assert np.all(np.diff(a["x"]) > 0)          # a sample keeps the returned row order


def test_plain_run_leaves_the_extras_and_checks_to_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert not args.full and args.steps == 7 and args.warmup == 2 and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "out"
    monkeypatch.setattr(bench, "FULL", False)
    assert not bench.verify_on()
    monkeypatch.setattr(bench, "FULL", True)
    monkeypatch.setenv("PLX_BENCH_VERIFY", "1")
    assert bench.verify_on()
