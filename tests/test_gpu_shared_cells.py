"""Shared cells of the LDS-table scans on the device (csrc/fused_cells.hpp, csrc/fused_sinks.hpp LdsCellSink; DESIGN.md 4.11 "Shared cells") -- against numpy and,
for TPC-H Q1, the oracle.

The switch behind PLX_SHARED_CELLS belongs to the process, so every case runs in a fresh child (tests/shared_cells_worker.py): the query with shared cells, then
switched off.  Integer outputs and the integer mean are equal bit for bit between the two and equal to numpy; f64 sums within RTOL = 1e-6
(tests/test_gpu_encoded_inputs.py); the cell count of each run is asserted from pl._ffi.last_lds_cells().  Row counts 511, 512, 513 and 1025: below one wide tile,
exactly one, one and a one-row tail tile, two and a one-row tail tile."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["one_group", "row_mod_6", "group_fails_predicate", "group_of_zeros", "hundred_groups", "eight_copies"]
SOURCES = ["u8_all_255", "u16_all_65535", "affine_base_5_stride_3"]
DECLINED = ["negative_base", "nullable_source", "base_2_45"]
Q1 = ["q1_shape_15", "q1_shape_16"]


def worker(case, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shared_cells_worker.py"), case], capture_output=True, text=True, timeout=240, cwd=ROOT,
                       env=dict(os.environ, **(env or {})))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-1500:], r.stderr[-2500:])
    return r.stdout


@pytest.mark.parametrize("case", LAYOUTS + SOURCES)
def test_shared_then_switched_off(case):
    """run-time compiled kernels (no ahead-of-time shape has these programs): count, sum and mean of the integer column in one cell"""
    assert "count, sum and mean in one cell" in worker(case)


@pytest.mark.parametrize("case", DECLINED)
def test_declined(case):
    """a base below zero and a nullable source keep one cell per aggregate; at base 2^45 the count still shares the sum's cell and the mean keeps its own"""
    out = worker(case)
    assert ("the mean in its own" if case == "base_2_45" else "one cell per aggregate") in out


@pytest.mark.parametrize("case", Q1)
def test_q1_ahead_of_time_shapes_against_the_oracle(case):
    assert "5 cells, off: 7" in worker(case)


def test_environment_switch_is_read_once():
    """PLX_SHARED_CELLS=0 in the environment: the first run holds one cell per aggregate"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport polars_amd as pl\nimport shared_cells_worker as W\nimport test_gpu_encoded_inputs as T\n"
            "pl.init(0)\npl._ffi.jit_set_min_rows(0)\ndata = W.case_table('row_mod_6', 1025)\ndf = T.frame_of(pl, data)\n"
            "out = df.lazy().filter(pl.col('p') > 3).group_by('g').agg(*T.aggs_of(pl, W.COLS)).collect()\n"
            "T.check(out, T.reference(data, W.COLS, data['p'][0] > 3, data['g'][0]), True, 'env')\n"
            "assert pl._ffi.last_lds_cells() == 4, pl._ffi.last_lds_cells()\nprint('one cell per aggregate')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLX_SHARED_CELLS="0"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "one cell per aggregate" in r.stdout, r.stdout + r.stderr
