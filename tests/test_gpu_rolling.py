"""rolling_sum / rolling_mean / rolling_min / rolling_max on the device, plain and under `.over(keys)`, against tests/rolling_ref.py: every row in row order,
validity bit for bit, on BOTH routes (the tile-halo kernel and the two scans, forced with PLX_ROLLING_ROUTE) -- the two agreeing with one reference at every shape
is the check that neither hides a fault behind the other.

Sizes around the wave (64), the workgroup (256) and the tile (2048); windows 1, 2, 3, 7, 64, 65, 2047, 2048 (the tile route's bound) and 2049 (the two scans by
the default rule), larger than a partition and larger than the column, both center values, min_samples 1, w and one between; the segment patterns that can break a
segmented scan and partitions shorter than the window whose head lies inside a halo; validity patterns with payloads under the nulls that would show (an all-null
window, a window with exactly min_samples and exactly min_samples - 1 valid values); values at the bounds of their types, NaN and infinities, an infinity that
leaves the window; every operand dtype with its result dtype; the places an expression may stand; sharing one sorted order; the C entry and the plugin symbol.

Exact where the function is exact (integer results, rolling_min / rolling_max as numbers); a float rolling_sum within RTOL * sum over the window of |x_j| of the
float64 reference, rolling_mean within that divided by the count (tests/rolling_ref.py check_rolling)."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from polars_amd import _ffi as F
from tests import cumulative_ref as CR
from tests import plugin_abi as P
from tests import rolling_ref as R
from tests.test_gpu_cumulative import cells, contiguous_keys, frame_of

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5)
N = 2 * 2048 + 5
BOUND = 2048                          # rolling::kMaxWindow: the tile route's largest window
WINDOWS = (1, 2, 3, 7, 64, 65, 2047, 2048, 2049)
ROUTES = ("tile", "scans")
TILE, SCANS, EMPTY = "rolling[tile halo:", "rolling[two scans:", "rolling[empty]"
PATTERNS = ("one", "each", "three_tiles", "tile_first", "tile_last", "wave_edges", "random", "short")


def route_word(route, w, n=1):
    return EMPTY if n == 0 else TILE if route == "tile" and w <= BOUND else SCANS


def fn(e, op, w, m=None, center=False):
    return getattr(e, op)(w, min_samples=m, center=center)


def between(w):
    return max(1, (w + 1) // 2)


@pytest.fixture(params=ROUTES)
def route(request, monkeypatch):
    monkeypatch.setenv("PLX_ROLLING_ROUTE", request.param)
    return request.param


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_whole_column_and_over(pl, n, route):
    rng = np.random.default_rng(4190 + n)
    i = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    x, xm = rng.normal(5.0, 2.0, n), rng.random(n) > 0.2
    k, km = rng.integers(-2, max(n // 5, 1) - 2, n).astype(np.int32), rng.random(n) > 0.1
    df = frame_of(pl, {"k": (k, km), "i": (i, None), "x": (x, xm)})
    c = pl.col
    for w, center, m in ((3, False, 1), (65, True, 2), (BOUND + 1, False, 1)):
        for keys, wrap in ((None, lambda e: e), ([(k, km)], lambda e: e.over("k"))):
            out = df.select(*[wrap(fn(c("x"), op, w, m, center)).alias(op) for op in R.OPS], wrap(c("i").rolling_sum(w, min_samples=m, center=center)).alias("isum"))
            plan = pl.last_plan()
            assert plan.count("Rolling{") == 1 and "fns=5" in plan and route_word(route, w, n) in plan and f"w={w}" in plan and f"rows={n}" in plan, plan
            assert ("keys=[k]" if keys else "keys=[]") in plan and (("sorted rows:" in plan) == (keys is not None and n > 0)), plan
            for op in R.OPS:
                R.check_rolling(*cells(out[op]), op, x, xm, w, m, center, keys, what=(n, w, op, keys is not None))
            R.check_rolling(*cells(out["isum"]), "rolling_sum", i, None, w, m, center, keys, what=(n, w, "isum"))


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_table():
    rng = np.random.default_rng(4191)
    x, xm = rng.normal(0.0, 100.0, N), rng.random(N) > 0.25
    i = rng.integers(-1000, 1000, N).astype(np.int32)
    k = contiguous_keys("random", N, rng)                    # partitions of 1..300 rows: most windows are larger than their partition
    k = k[rng.permutation(N)]                                # ... interleaved, so the sorted order is a real permutation
    return {"k": (k, None), "x": (x, xm), "i": (i, xm)}


@pytest.mark.parametrize("w", WINDOWS + (N + 7,))
def test_windows_center_and_min_samples(pl, window_table, w, route):
    df = frame_of(pl, window_table)
    (k, _), (x, xm), (i, _) = (window_table[nm] for nm in ("k", "x", "i"))
    c = pl.col
    for center in (False, True):
        for m in sorted({1, between(w), w}):
            out = df.select(*[fn(c("x"), op, w, m, center).alias(op) for op in R.OPS], *[fn(c("x"), op, w, m, center).over("k").alias("o_" + op) for op in R.OPS],
                            c("i").rolling_min(w, min_samples=m, center=center).alias("imin"), c("i").rolling_sum(w, min_samples=m, center=center).over("k").alias("o_isum"))
            plan = pl.last_plan()
            assert plan.count("Rolling{") == 2 and plan.count(route_word(route, w)) == 2 and (TILE in plan) != (SCANS in plan), plan
            for op in R.OPS:
                R.check_rolling(*cells(out[op]), op, x, xm, w, m, center, None, what=(w, m, center, op))
                R.check_rolling(*cells(out["o_" + op]), op, x, xm, w, m, center, [(k, None)], what=(w, m, center, "over", op))
            R.check_rolling(*cells(out["imin"]), "rolling_min", i, xm, w, m, center, None, what=(w, m, center, "imin"))
            R.check_rolling(*cells(out["o_isum"]), "rolling_sum", i, xm, w, m, center, [(k, None)], what=(w, m, center, "o_isum"))


def test_the_default_rule_and_the_environment_variable(pl, monkeypatch):
    s = pl.Series("x", np.arange(100, dtype=np.float64))
    monkeypatch.delenv("PLX_ROLLING_ROUTE", raising=False)
    for w, word in ((1, TILE), (BOUND, TILE), (BOUND + 1, SCANS), (10 ** 6, SCANS)):
        s.rolling_sum(w, min_samples=1)
        assert word in pl.last_plan() and f"w={w}" in pl.last_plan(), pl.last_plan()
    monkeypatch.setenv("PLX_ROLLING_ROUTE", "scans")          # read per call
    s.rolling_sum(7)
    assert SCANS in pl.last_plan(), pl.last_plan()
    monkeypatch.setenv("PLX_ROLLING_ROUTE", "tile")
    s.rolling_sum(7)
    assert TILE in pl.last_plan() and "lds=" in pl.last_plan(), pl.last_plan()
    s.rolling_sum(BOUND + 1)                                  # "tile" names the default rule: above the bound the two scans run
    assert SCANS in pl.last_plan(), pl.last_plan()


# ---- segment patterns, through .over -------------------------------------------------------------------------------------------------------------------
def pattern_keys(pattern, n, rng):
    if pattern == "short":                                   # partitions of 1..40 rows: shorter than the window, heads inside every halo
        lens, used = [], 0
        while used < n:
            ln = min(n - used, int(rng.integers(1, 41)))
            lens.append(ln); used += ln
        return np.repeat(np.arange(len(lens), dtype=np.int32), lens)
    return contiguous_keys(pattern, n, rng)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_segment_patterns(pl, pattern, route):
    rng = np.random.default_rng(4192)
    k = pattern_keys(pattern, N, rng)
    x = rng.integers(-(1 << 31), 1 << 31, N, dtype=np.int64).astype(np.int32)
    xm = rng.random(N) > 0.15
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    c = pl.col
    for w, center in ((7, False), (64, True), (700, False), (BOUND, True)):
        m = between(w) if pattern in ("one", "three_tiles") else 1
        out = df.select(*[fn(c("x"), op, w, m, center).over("k").alias(op) for op in ("rolling_sum", "rolling_min", "rolling_max")])
        assert route_word(route, w) in pl.last_plan() and pl.last_plan().count("Rolling{") == 1, pl.last_plan()
        for op in ("rolling_sum", "rolling_min", "rolling_max"):
            R.check_rolling(*cells(out[op]), op, x, xm, w, m, center, [(k, None)], what=(pattern, w, op))


# ---- validity -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("validity", ("all_null_window", "exactly_min_samples", "one_short_of_min_samples", "none"))
def test_validity_patterns_with_payloads_under_the_nulls(pl, validity, route):
    rng = np.random.default_rng(4193)
    n, w = N, 8
    pos = np.arange(n)
    if validity == "all_null_window":
        ok = (pos // 40) % 2 == 0                            # stretches of 40 nulls: five whole windows without a value
        m = 1
    elif validity == "none":
        ok, m = None, w
    else:
        ok = pos % 8 < 3                                     # every full window holds exactly three valid values
        m = 3 if validity == "exactly_min_samples" else 4
    mask = np.ones(n, bool) if ok is None else ok
    f = rng.normal(0.0, 100.0, n)
    i = rng.integers(-1000, 1000, n).astype(np.int16)
    f[~mask] = np.nan                                        # what a null row carries would show: NaN in a float sum, the type's extremes in min / max
    i[~mask] = np.where(rng.random(int((~mask).sum())) < 0.5, np.iinfo(np.int16).min, np.iinfo(np.int16).max)
    k = np.repeat(np.arange(n // 500 + 1, dtype=np.int32), 500)[:n]
    df = frame_of(pl, {"k": (k, None), "f": (f, ok), "i": (i, ok)})
    c = pl.col
    for center in (False, True):
        out = df.select(*[fn(c(col), op, w, m, center).over("k").alias(f"{col}_{op}") for col in ("f", "i") for op in R.OPS],
                        *[fn(c(col), op, w, m, center).alias(f"w_{col}_{op}") for col in ("f", "i") for op in R.OPS])
        for col, v in (("f", f), ("i", i)):
            for op in R.OPS:
                R.check_rolling(*cells(out[f"{col}_{op}"]), op, v, ok, w, m, center, [(k, None)], what=(validity, col, op, center))
                R.check_rolling(*cells(out[f"w_{col}_{op}"]), op, v, ok, w, m, center, None, what=(validity, "whole", col, op, center))
        if validity == "one_short_of_min_samples":
            assert cells(out["w_f_rolling_sum"])[1].sum() == 0 and cells(out["i_rolling_min"])[1].sum() == 0          # no window reaches min_samples
        if validity == "exactly_min_samples" and not center:
            assert cells(out["w_f_rolling_sum"])[1][w - 1:].all()


# ---- values and dtypes --------------------------------------------------------------------------------------------------------------------------------------
DTYPES = (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype_with_its_result_dtype_and_values_at_the_bounds(pl, dtype, route):
    rng = np.random.default_rng(4194)
    n = 2049
    dt = np.dtype(dtype)
    if dt.kind == "b":
        x = rng.random(n) < 0.5
    elif dt.kind == "f":
        x = rng.normal(0.0, 1000.0, n).astype(dt)
        x[rng.random(n) < 0.05] = 0.0
        x[rng.random(n) < 0.05] = -0.0                  # signed zeros
    else:
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        x[rng.random(n) < 0.2] = info.max               # the bounds of the type: sums wrap
        x[rng.random(n) < 0.2] = info.min
    xm = rng.random(n) > 0.1
    k = rng.integers(0, 9, n).astype(np.int32)
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    c = pl.col
    for keys, wrap in ((None, lambda e: e), ([(k, None)], lambda e: e.over("k"))):
        for w, center in ((5, False), (66, True)):
            out = df.select(*[wrap(fn(c("x"), op, w, 2, center)).alias(op) for op in R.OPS])
            for op in R.OPS:
                v, ok = cells(out[op])
                assert v.dtype == R.result_dtype(op, dt), (dt, op, v.dtype)
                assert out[op].dtype == pl.datatypes.NP_TO_DTYPE[R.result_dtype(op, dt)], (dt, op, out[op].dtype)
                R.check_rolling(v, ok, op, x, xm, w, 2, center, keys, what=(dt.name, op, keys is not None, w))


def test_nan_and_infinities_and_an_infinity_that_leaves_the_window(pl, route):
    nan, inf = np.nan, np.inf
    c = pl.col
    cases = {"nan_first": [nan, 1.0, 2.0, -1.0, 3.0], "nan_last": [1.0, 2.0, -1.0, nan], "nan_alone": [nan], "nan_mid": [3.0, nan, 1.0, nan, 2.0, 5.0, 6.0],
             "inf_leaves": [1.0, inf, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], "minus_inf_leaves": [-inf, 5.0, 1.0, 2.0, 3.0], "inf_and_minus_inf": [1.0, inf, 2.0, -inf, 3.0, 4.0, 5.0, 6.0],
             "all_nan": [nan, nan, nan, nan], "zeros": [-0.0, 0.0, -0.0, 1.0, -1.0, 0.0]}
    for dt in (np.float64, np.float32):
        for name, vals in cases.items():
            x = np.array(vals, dt)
            s = pl.Series("x", x)
            for w in (2, 3):
                for op in R.OPS:
                    R.check_rolling(*cells(getattr(s, op)(w, min_samples=1)), op, x, None, w, 1, False, None, what=(name, dt.__name__, op, w))
        # after the infinity has left the window the results are finite again: what a difference of prefixes gets wrong
        x = np.array(cases["inf_leaves"], dt)
        v, ok = cells(pl.Series("x", x).rolling_sum(3))
        assert ok.tolist() == [False, False] + [True] * 6 and np.isinf(v[2:4]).all() and v[4:].tolist() == [9.0, 12.0, 15.0, 18.0], v
        v, ok = cells(pl.Series("x", x).rolling_mean(2))
        assert np.isinf(v[1:3]).all() and v[3:].tolist() == [2.5, 3.5, 4.5, 5.5, 6.5], v
        # the same vectors side by side as partitions of one column, in a long column: a NaN or an infinity stays inside its own partition and its own windows
        reps = 40
        x = np.concatenate([np.array(v, dt) for v in cases.values()] * reps)
        k = np.concatenate([np.full(len(v), j + r * len(cases), np.int32) for r in range(reps) for j, v in enumerate(cases.values())])
        perm = np.random.default_rng(4195).permutation(len(x))
        x, k = x[perm], k[perm]
        out = frame_of(pl, {"k": (k, None), "x": (x, None)}).select(*[fn(c("x"), op, 3, 1).over("k").alias(op) for op in R.OPS], *[fn(c("x"), op, 4, 2, True).alias("w_" + op) for op in R.OPS])
        for op in R.OPS:
            R.check_rolling(*cells(out[op]), op, x, None, 3, 1, False, [(k, None)], what=("partitions", dt.__name__, op))
            R.check_rolling(*cells(out["w_" + op]), op, x, None, 4, 2, True, None, what=("whole", dt.__name__, op))


def test_integer_valued_floats_are_bit_exact_on_both_routes(pl, monkeypatch):
    rng = np.random.default_rng(4196)
    n = 3 * 2048 + 77
    x = rng.integers(-1000, 1000, n).astype(np.float64)           # every partial sum is an integer below 2^53: any association gives the same bits
    k = rng.integers(0, 50, n).astype(np.int32)
    df = frame_of(pl, {"k": (k, None), "x": (x, None)})
    c = pl.col
    got = {}
    for r in ROUTES:
        monkeypatch.setenv("PLX_ROLLING_ROUTE", r)
        out = df.select(c("x").rolling_sum(100, min_samples=1).alias("w"), c("x").rolling_sum(100, min_samples=1, center=True).over("k").alias("o"))
        got[r] = (out["w"].to_numpy(), out["o"].to_numpy())
    want, _, _, _ = R.rolling("rolling_sum", x, None, 100, 1, False)
    assert got["tile"][0].view(np.uint64).tolist() == want.view(np.uint64).tolist() == got["scans"][0].view(np.uint64).tolist()
    want, _, _, _ = R.rolling("rolling_sum", x, None, 100, 1, True, [(k, None)])
    assert got["tile"][1].view(np.uint64).tolist() == want.view(np.uint64).tolist() == got["scans"][1].view(np.uint64).tolist()


def test_temporal_and_categorical_operands(pl, route):
    rng = np.random.default_rng(4197)
    n = 700
    d, t = rng.integers(8000, 11000, n).astype(np.int32), rng.integers(0, 10 ** 15, n).astype(np.int64)
    ok = rng.random(n) > 0.2
    k = rng.integers(0, 5, n).astype(np.int32)
    df = pl.DataFrame([pl.Series("k", k), pl.Series("d", d, pl.Date, validity=ok), pl.Series("t", t, pl.Datetime, validity=ok),
                       pl.Series("s", rng.integers(0, 3, n).astype(np.uint8), pl.Categorical(["A", "N", "R"], pl.UInt8))])
    c = pl.col
    out = df.select(c("d").rolling_min(5, min_samples=1).alias("dmin"), c("t").rolling_max(9, min_samples=2, center=True).over("k").alias("tmax"))
    assert out["dmin"].dtype == pl.Date and out["tmax"].dtype == pl.Datetime
    R.check_rolling(*cells(out["dmin"]), "rolling_min", d, ok, 5, 1, False, None, what="date")
    R.check_rolling(*cells(out["tmax"]), "rolling_max", t, ok, 9, 2, True, [(k, None)], what="datetime")
    for e in (c("d").rolling_sum(3), c("t").rolling_mean(3), c("s").rolling_min(3), c("s").rolling_sum(3), c("s").rolling_max(3).over("k")):
        with pytest.raises(TypeError, match=r"rolling_\w+\(\) needs"):
            df.select(e)
    with pytest.raises(TypeError, match="rolling_sum"):
        df["s"].rolling_sum(3)
    assert df["d"].rolling_max(3).dtype == pl.Date


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(4198)
    n = 1000
    return {"k": (rng.integers(0, 40, n).astype(np.int32), rng.random(n) > 0.05), "g": (rng.integers(0, 5, n).astype(np.int64), None),
            "x": (rng.integers(-50, 50, n).astype(np.float64), rng.random(n) > 0.1), "i": (rng.integers(-500, 500, n).astype(np.int64), None)}


def test_in_select_with_columns_filter_and_inside_expressions(pl, table, route):
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (g, _), (x, xm), (i, _) = (table[nm] for nm in ("k", "g", "x", "i"))
    n = len(k)
    out = df.with_columns((c("i") * c("g")).rolling_sum(5).over("k").alias("run"), c("i").rolling_max(4, min_samples=1).alias("hi"), c("i").rolling_mean(3, center=True).over("g", "k").alias("gk"))
    plan = pl.last_plan()
    assert out.columns == ["k", "g", "x", "i", "run", "hi", "gk"] and out.height == n and plan.count("Rolling{") == 3, plan
    assert "keys=[k]" in plan and "keys=[g, k]" in plan and "keys=[]" in plan, plan
    R.check_rolling(*cells(out["run"]), "rolling_sum", i * g, None, 5, 5, False, [(k, km)], what="operand expression")
    R.check_rolling(*cells(out["hi"]), "rolling_max", i, None, 4, 1, False, None, what="hi")
    R.check_rolling(*cells(out["gk"]), "rolling_mean", i, None, 3, 3, True, [(g, None), (k, km)], what="gk")
    # inside arithmetic, comparisons and when / then / otherwise; twins are computed once
    out = df.select(c("i").rolling_sum(3, min_samples=1).over("k").alias("a"), (c("i") - c("i").rolling_sum(3, min_samples=1).over("k")).alias("rest"),
                    pl.when(c("i").rolling_min(3, min_samples=1).over("k") > 0).then(c("i")).otherwise(c("i").rolling_max(3, min_samples=1).over("k")).alias("w"))
    plan = pl.last_plan()
    assert plan.count("Rolling{") == 1 and "fns=4" in plan, plan
    s3, _, _, _ = R.rolling("rolling_sum", i, None, 3, 1, False, [(k, km)])
    lo, _, _, _ = R.rolling("rolling_min", i, None, 3, 1, False, [(k, km)])
    hi, _, _, _ = R.rolling("rolling_max", i, None, 3, 1, False, [(k, km)])
    assert np.array_equal(out["rest"].to_numpy(), i - s3) and np.array_equal(out["w"].to_numpy(), np.where(lo > 0, i, hi))
    # as a filter predicate (a null predicate row is dropped)
    kept = df.filter(c("i").rolling_sum(3).over("k") > 100)
    assert "Rolling{" in pl.last_plan() and "shift / diff / rolling expression: per-node route" in pl.last_plan(), pl.last_plan()
    s3f, ok3, _, _ = R.rolling("rolling_sum", i, None, 3, 3, False, [(k, km)])
    assert np.array_equal(kept["i"].to_numpy(), i[ok3 & (s3f > 100)])
    # lazily, after a filter, with and without fusion; an empty frame
    keep = i > 0
    q = df.lazy().filter(c("i") > 0).with_columns(c("i").rolling_sum(4, min_samples=2).over("k").alias("s"))
    for res in (q.collect(), q.collect(no_fusion=True)):
        R.check_rolling(*cells(res["s"]), "rolling_sum", i[keep], None, 4, 2, False, [(k[keep], km[keep])], what="after filter")
    out = df.filter(c("i") > 10_000).select(c("i").rolling_sum(3).over("k").alias("s"), c("x").rolling_mean(2).alias("m"), c("g").cast(pl.Int8).rolling_sum(2).alias("w"))
    assert out.height == 0 and (out["s"].dtype, out["m"].dtype, out["w"].dtype) == (pl.Int64, pl.Float64, pl.Int64) and EMPTY in pl.last_plan(), pl.last_plan()


def test_functions_over_one_key_list_share_one_sorted_order(pl, table):
    """cum_sum, shift and rolling over [k] in one node: one bucket, one stable sort and one head mask (one segment_heads launch, the sort's launches of a single
    function), and the three plan lines name the same sorted order"""
    def kernel_records():
        recs = (F.ProfileRecord * 4096)()
        count = C.c_int32()
        F.check(F.lib().plx_profile_fetch(recs, 4096, C.byref(count)))
        F.check(F.lib().plx_profile_clear())
        return [recs[j].name.decode() for j in range(count.value)]
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (i, _) = table["k"], table["i"]

    def launches(exprs):
        F.check(F.lib().plx_synchronize()); F.check(F.lib().plx_profile_enable(1))
        kernel_records()
        out = df.select(*exprs)
        F.check(F.lib().plx_synchronize())
        recs = kernel_records()
        F.check(F.lib().plx_profile_enable(0))
        return out, recs, pl.last_plan()
    _, one, _ = launches([c("i").shift(1).over("k").alias("s")])
    out, three, plan = launches([c("i").cum_sum().over("k").alias("c"), c("i").shift(1).over("k").alias("s"), c("i").rolling_sum(3).over("k").alias("r"),
                                 c("i").rolling_min(3).over("k").alias("m")])
    sort_of = lambda recs: sorted(r for r in recs if r.startswith("sort_"))
    assert three.count("segment_heads") == 1 == one.count("segment_heads") and sort_of(three) == sort_of(one) and sort_of(one), (one, three)
    assert plan.count("Cumulative{") == 1 and plan.count("Shift{") == 1 and plan.count("Rolling{") == 1 and "fns=2" in plan, plan
    orders = {seg.split("}")[0].split("]")[0] for seg in plan.split("sorted rows: ")[1:]}
    assert len(orders) == 1, plan                                        # one sorted order, named by each line of the bucket
    CR.check_cum(*cells(out["c"]), "cum_sum", i, None, [(k, km)], False, what="shared cum")
    R.check_shift(*cells(out["s"]), i, None, 1, None, [(k, km)], what="shared shift")
    R.check_rolling(*cells(out["r"]), "rolling_sum", i, None, 3, 3, False, [(k, km)], what="shared rolling")
    R.check_rolling(*cells(out["m"]), "rolling_min", i, None, 3, 3, False, [(k, km)], what="shared rolling min")


def test_refusals(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    with pytest.raises(TypeError, match="group_by"):
        df.lazy().group_by("g").agg(c("x").rolling_sum(3)).collect()
    with pytest.raises(TypeError, match="an aggregate"):
        df.select(c("x").sum().rolling_sum(2))
    with pytest.raises(TypeError, match="a window expression"):
        df.select(c("x").sum().over("k").rolling_max(2))
    with pytest.raises(TypeError, match="inside the operand of another one"):
        df.select(c("x").rolling_sum(2).cum_max())
    with pytest.raises(TypeError, match="inside the operand of another one"):
        df.select(c("x").cum_sum().rolling_mean(2))
    with pytest.raises(TypeError, match="mixes a cumulative / ranking expression"):
        df.select((c("x").rolling_sum(2) / c("x").sum()).over("k"))
    with pytest.raises(ValueError, match="weights"):
        df.select(c("x").rolling_sum(2, [0.5, 0.5]))
    with pytest.raises(ValueError, match="temporal window"):
        df.select(c("x").rolling_mean("7d"))
    with pytest.raises(pl.UnsupportedError, match="1..8"):
        df.select(c("x").rolling_sum(2).over(*["k"] * 9))
    out = df.select((c("x").rolling_sum(2, min_samples=1).over("k") / c("x").sum().over("k")).alias("share"))          # the arithmetic outside the two .over()s
    assert out.height == df.height and "Rolling{" in pl.last_plan() and "Window{" in pl.last_plan()


def test_example_query(pl, route):
    from polars_amd import queries as QQ
    rng = np.random.default_rng(4199)
    n = 3000
    flag = rng.integers(0, 3, n).astype(np.uint8)
    price, disc = rng.uniform(900.0, 100000.0, n), rng.integers(0, 11, n) / 100.0
    df = frame_of(pl, {"l_returnflag": (flag, None), "l_extendedprice": (price, None), "l_discount": (disc, None)})
    out = QQ.moving_average_revenue_by_flag(df.lazy()).collect()
    assert pl.last_plan().count("Rolling{") == 1 and route_word(route, 7) in pl.last_plan() and "w=7" in pl.last_plan(), pl.last_plan()
    R.check_rolling(*cells(out["revenue_ma7"]), "rolling_mean", price * (1.0 - disc), None, 7, 1, False, [(flag, None)], what="moving average")


# ---- the C entry and the plugin symbol ----------------------------------------------------------------------------------------------------------------------
def test_c_entry_and_plugin_symbol(pl, route):
    rng = np.random.default_rng(4200)
    n = 2100
    k, km = rng.integers(0, 9, n).astype(np.int32), rng.random(n) > 0.1
    x, xm = rng.normal(2.0, 1.0, n), rng.random(n) > 0.2
    i = rng.integers(-50, 50, n).astype(np.int8)
    ks, xs, isr = pl.Series("k", k, validity=km), pl.Series("x", x, validity=xm), pl.Series("i", i)
    out = C.c_uint64()
    F.check(F.lib().plx_rolling((C.c_uint64 * 1)(ks._h), 1, isr._h, F.ROLLING_SUM, 5, 2, 1, C.byref(out)))
    plan = F.lib().plx_last_plan_description().decode()
    assert "Rolling{keys=[1 columns], fns=1" in plan and route_word(route, 5) in plan and "sorted rows:" in plan and "w=5" in plan, plan
    R.check_rolling(*cells(pl.Series._from_handle("s", out.value, pl.Int64)), "rolling_sum", i, None, 5, 2, True, [(k, km)], what="C over")
    F.check(F.lib().plx_rolling(None, 0, xs._h, F.ROLLING_MIN, 3000, 1, 0, C.byref(out)))
    assert SCANS in F.lib().plx_last_plan_description().decode()
    R.check_rolling(*cells(pl.Series._from_handle("m", out.value, pl.Float64)), "rolling_min", x, xm, 3000, 1, False, None, what="C whole, a window above the column")
    # parameters are refused by name before anything runs, an empty input included
    empty = pl.Series("e", np.zeros(0, np.int64))
    err = lambda: F.lib().plx_last_error().decode()
    for col in (xs, empty):
        assert F.lib().plx_rolling(None, 0, col._h, 4, 3, 3, 0, C.byref(out)) == 1 and "no plx_rolling_op" in err()
        assert F.lib().plx_rolling(None, 0, col._h, F.ROLLING_SUM, 0, 1, 0, C.byref(out)) == 1 and "window_size" in err()
        assert F.lib().plx_rolling(None, 0, col._h, F.ROLLING_SUM, 1 << 31, 1, 0, C.byref(out)) == 1 and "window_size" in err()
        assert F.lib().plx_rolling(None, 0, col._h, F.ROLLING_SUM, 3, 4, 0, C.byref(out)) == 1 and "min_samples" in err()
        assert F.lib().plx_rolling(None, 0, col._h, F.ROLLING_SUM, 3, 0, 0, C.byref(out)) == 1 and "min_samples" in err()
        assert F.lib().plx_rolling(None, 0, col._h, F.ROLLING_SUM, 3, 3, 2, C.byref(out)) == 1 and "center must be 0 or 1" in err()
    F.check(F.lib().plx_rolling(None, 0, empty._h, F.ROLLING_MEAN, 3, 3, 0, C.byref(out)))
    e = pl.Series._from_handle("n", out.value, pl.Float64)
    assert len(e) == 0 and EMPTY in F.lib().plx_last_plan_description().decode()
    nine = (C.c_uint64 * 9)(*([ks._h] * 9))
    assert F.lib().plx_rolling(nine, 9, xs._h, F.ROLLING_SUM, 3, 3, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in err()
    # the plugin symbol: the value series, then the key series
    arr_x, arr_k = pa.array(x, mask=~xm), pa.array(k, mask=~km)
    res, inp = P.call("plx_rolling", [arr_x, arr_k], {"op": "mean", "window_size": 7, "min_samples": 2, "center": True}, names=["x", "k"])
    assert res is not None and inp.released == 2 and inp.out_name == b"x" and res.type == pa.float64() and len(res) == n, P.last_error()
    R.check_rolling(np.asarray(res.fill_null(0.0)), ~np.asarray(res.is_null()), "rolling_mean", x, xm, 7, 2, True, [(k, km)], what="plugin over")
    res, _ = P.call("plx_rolling", [pa.array(i)], {"op": "max", "window_size": 4})
    assert res is not None and res.type == pa.int8(), P.last_error()
    R.check_rolling(np.asarray(res.fill_null(0)), ~np.asarray(res.is_null()), "rolling_max", i, None, 4, 4, False, None, what="plugin whole")
    for arrs in ([arr_x, arr_k], [arr_x.slice(0, 0), arr_k.slice(0, 0)]):
        res, inp = P.call("plx_rolling", arrs, {"op": "var", "window_size": 3})
        assert res is None and inp.released == 2 and "kwargs must carry op in {sum, mean, min, max}" in P.last_error(), P.last_error()
        res, inp = P.call("plx_rolling", arrs, {"op": "sum"})
        assert res is None and "window_size must be an integer of at least 1" in P.last_error(), P.last_error()
        res, inp = P.call("plx_rolling", arrs, {"op": "sum", "window_size": 3, "min_samples": 5})
        assert res is None and "min_samples must be an integer in 1..window_size" in P.last_error(), P.last_error()
        res, inp = P.call("plx_rolling", arrs, {"op": "sum", "window_size": 3, "center": "yes"})
        assert res is None and "center must be a bool" in P.last_error(), P.last_error()
