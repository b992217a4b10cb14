"""The compiled aggregate scans over narrow rows -- dictionaries staged in LDS, no bitmap test on non-nullable loads (csrc/fused_sinks.hpp fused_scan_body, DESIGN.md
"Encoded shadows") -- against numpy.

As in tests/test_gpu_encoded_inputs.py every query runs three times -- the plain scan, the scan that builds the shadows, the scan that reads them -- and all three
results are compared with numpy: integers, counts and min / max exactly, f64 sums within RTOL = 1e-6.  The third run must name the encodings the data admits, and
with them a row is at most 16 bytes (asserted from the data), so the run-time compiled kernel reads its dictionaries from LDS and leaves the bitmap test out of its
non-nullable loads.  The small sizes lower the run-time compilation threshold to 0 rows: below it the generic interpreter would run, which has neither."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_encoded_inputs as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY_US = T.DAY_US
# launch geometry of the scans (csrc/kernels_fused.hip fused_lds_agg / fused_regagg): a wave takes 128-row tiles grid-stride; at most 8 workgroups per CU are ever
# launched by default or through the PLX_BPC_* knobs' measured range (the default is 5), so the sizes below hold for any of them
CUS, MAX_WG_PER_CU, WAVES_PER_WG, TILE_ROWS = 256, 8, 4, 128
# nothing, one row, around one 128-row tile, around 512 and 1024 rows (several tiles, the last one full, one row short, one row over)
SMALL = [0, 1, 127, 128, 129, 511, 512, 513, 1023, 1025]
# every wave runs several full iterations (five at 8 workgroups per CU, eight at 5), the last tile holds one row, and the default threshold of the run-time
# compiler (2^22 rows) is passed
LARGE = 5 * CUS * MAX_WG_PER_CU * WAVES_PER_WG * TILE_ROWS + 385 + 256
assert LARGE > 2 * CUS * MAX_WG_PER_CU * WAVES_PER_WG * TILE_ROWS + 385 and LARGE % TILE_ROWS == 1 and LARGE >= 1 << 22

WIDTH = {"affine8": 1, "affine16": 2, "dict8": 1}
COLS = [("q", ("sum", "min", "max")), ("d", ("sum", "mean")), ("t", ("sum",)), ("x", ("sum", "min", "max"))]


@functools.lru_cache(maxsize=None)
def table(n, nulls=False):
    """g: u8 key with 6 values; day: date-like i64 with a stride; q: small-range i64; d, t: f64 with 11 / 9 distinct values; x: f64 that does not encode"""
    rng = np.random.default_rng(4000 + n)
    data = {
        "g": (rng.integers(0, 6, n).astype(np.uint8), None),
        "day": (8035 * DAY_US + DAY_US * rng.integers(0, 2500, n).astype(np.int64), None),
        "q": (1 + rng.integers(0, 50, n).astype(np.int64), None),
        "d": (np.round(rng.integers(0, 11, n) / 100.0, 2), None),
        "t": (np.round(rng.integers(0, 9, n) / 100.0, 2), None),
        "x": (900.0 + 100000.0 * rng.random(n), None),
    }
    if nulls:
        data["q"] = (data["q"][0], rng.random(n) < 0.9)
    for v, valid in data.values():
        v.setflags(write=False)
        if valid is not None:
            valid.setflags(write=False)
    return data


CUTOFF = 8035 * DAY_US + 2450 * DAY_US      # keeps 98 % of the rows


def expected(data):
    e = {"day": T.expected_affine(data["day"][0]), "q": T.expected_affine(*data["q"]), "d": T.expected_dict(data["d"][0]), "t": T.expected_dict(data["t"][0]),
         "x": T.expected_dict(data["x"][0])}
    n = len(data["g"][0])
    if n:
        row = 1 + sum(WIDTH[v] if v else 8 for v in e.values())      # g + the five inputs as the third run reads them
        assert row <= 16, (row, e)
        assert n < 1000 or (e["x"] is None and e["day"] == "affine16" and e["q"] == "affine8" and e["d"] == "dict8" and e["t"] == "dict8"), e
    return e


def run_three(pl, n, keyed, nulls=False, cols=COLS, compiled=True):
    data = table(n, nulls)
    df = T.frame_of(pl, data)
    keep = data["day"][0] <= CUTOFF
    if n >= 1000:
        assert 0.97 < keep.mean() < 0.99
    if n == 0:      # no rows: no scan is launched and nothing can be encoded; the result is no group / one row of empty aggregates, three times
        ref = T.reference(data, cols, keep, data["g"][0] if keyed else None)
        for run in range(3):
            lf = df.lazy().filter(pl.col("day") <= CUTOFF)
            out = (lf.group_by("g").agg(*T.aggs_of(pl, cols)) if keyed else lf.select(*T.aggs_of(pl, cols))).collect()
            assert pl.last_plan_encodings() == "", pl.last_plan_encodings()
            T.check(out, ref, keyed, ("narrow rows", 0, keyed, run))
        return data, df
    used = {"day"} | {name for name, _ in cols}
    T.three_runs(pl, df, data, cols, pl.col("day") <= CUTOFF, keep, keyed, {k: v for k, v in expected(data).items() if k in used}, ("narrow rows", n, keyed, nulls))
    if compiled and n:
        assert "fused_scan[jit]" in pl.last_plan(), pl.last_plan()
    return data, df


def configured_min_rows():
    """the threshold the library starts with (csrc/jit.cpp enabled()): it has a setter but no getter, so this mirrors its reading of the environment"""
    if os.environ.get("PLX_JIT", "1").startswith("0"):
        return -1
    return int(os.environ.get("PLX_JIT_MIN_ROWS", 1 << 22))


@pytest.fixture
def compile_every_size(pl):
    pl._ffi.jit_set_min_rows(0)
    yield
    pl._ffi.jit_set_min_rows(configured_min_rows())


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", SMALL)
def test_row_counts_around_the_tile_boundaries(pl, compile_every_size, n, keyed):
    run_three(pl, n, keyed)


@pytest.mark.parametrize("keyed", [True, False])
def test_every_wave_runs_full_iterations_and_the_last_tile_is_partial(pl, keyed):
    run_three(pl, LARGE, keyed)


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", [1025, LARGE])
def test_null_bitmap_on_one_input(pl, compile_every_size, n, keyed):
    """q carries a validity bitmap: that input keeps its bitmap test, the others do not look for one"""
    cols = [("q", ("sum", "min", "max", "count")), ("d", ("sum",)), ("x", ("sum",))]
    run_three(pl, n, keyed, nulls=True, cols=cols)


@pytest.mark.parametrize("keyed", [True, False])
def test_a_shape_of_its_own_is_compiled_at_run_time(pl, keyed):
    """one aggregate more than any other query here, at the default threshold: compiled (not interpreted), with the LDS dictionaries"""
    before = pl._ffi.jit_stats()[0]
    run_three(pl, LARGE, keyed, cols=COLS + [("t", ("min", "max", "mean"))])
    assert "fused_scan[jit]" in pl.last_plan() and "fused_scan[generic]" not in pl.last_plan(), pl.last_plan()
    assert pl._ffi.jit_stats()[0] > before, pl._ffi.jit_stats()


def test_first_row_of_a_group_deep_in_the_input(pl):
    """maintain_order=True numbers the groups by their first selected row (AGG_FIRST_ROW), which the scan forms from each tile's row0.  Keys 3, 4 and 5 appear for the
    first time deep in the input, in three consecutive tiles, at lane offsets that would order them 5, 4, 3 if the tile's share of the row number were lost."""
    data = dict(table(LARGE))
    g = data["g"][0].copy()
    t0 = (LARGE // TILE_ROWS) // 2
    first = {4: (t0 + 1) * TILE_ROWS + 5, 3: (t0 + 2) * TILE_ROWS + 77, 5: (t0 + 3) * TILE_ROWS + 2}
    for key, row in first.items():
        g[:row][g[:row] == key] = key - 3      # 3 -> 0, 4 -> 1, 5 -> 2 in front of its first row
        g[row] = key
    g[:3] = [2, 0, 1]
    day = data["day"][0].copy()
    day[[0, 1, 2] + list(first.values())] = 8035 * DAY_US      # these rows pass the filter
    data["g"], data["day"] = (g, None), (day, None)
    keep = day <= CUTOFF
    want = [int(k) for k in g[keep][np.sort(np.unique(g[keep], return_index=True)[1])]]
    assert want == [2, 0, 1, 4, 3, 5], want
    df = T.frame_of(pl, data)
    ref = T.reference(data, COLS, keep, g)
    for run in range(3):
        out = df.lazy().filter(pl.col("day") <= CUTOFF).group_by("g", maintain_order=True).agg(*T.aggs_of(pl, COLS)).collect()
        assert "lds_table" in pl.last_plan() and "fused_scan[jit]" in pl.last_plan(), pl.last_plan()
        assert [int(k) for k in out.to_dict()["g"]] == want, (run, out.to_dict()["g"])
        T.check(out, ref, True, ("first row", run))
    assert T.encodings_in(pl.last_plan_encodings()) == {k: v for k, v in expected(data).items() if v}, pl.last_plan_encodings()


def test_switched_off_the_same_results_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport numpy as np\nimport polars_amd as pl\nimport test_gpu_encoded_inputs as T\nimport test_gpu_scan_tiles as S\n"
            "pl.init(0)\ndata = S.table(S.LARGE)\ndf = T.frame_of(pl, data)\nkeep = data['day'][0] <= S.CUTOFF\n"
            "for keyed in (True, False):\n    ref = T.reference(data, S.COLS, keep, data['g'][0] if keyed else None)\n    for run in range(3):\n"
            "        lf = df.lazy().filter(pl.col('day') <= S.CUTOFF)\n        lf = lf.group_by('g').agg(*T.aggs_of(pl, S.COLS)) if keyed else lf.select(*T.aggs_of(pl, S.COLS))\n"
            "        out = lf.collect()\n        assert pl.last_plan_encodings() == '', pl.last_plan_encodings()\n        T.check(out, ref, keyed, ('off', keyed, run))\nprint('plain every time')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLX_ENCODED_INPUTS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plain every time" in r.stdout, r.stdout + r.stderr
