"""cum_sum / cum_min / cum_max / cum_count on the device, plain and under `.over(keys)`, against tests/cumulative_ref.py: every row in row order, validity bit
for bit.

Sizes around the wave (64), the workgroup (256) and the scan's tile (2048), plus one size whose tile aggregates need the recursive level (2048 * 2048 + 3 rows, an
Int32 column, once per op); the segment patterns that can break a segmented scan (no head in a tile, heads on tile and wave edges); validity patterns with payloads
under the nulls that would show; values at the bounds of their types, NaN and infinities; every operand dtype with its result dtype; the places an expression may
stand; the plan text of each route; the C entry and the plugin symbol.

Exact where the function is exact (integer results, cum_count, cum_min / cum_max as numbers); a float cum_sum at row i within RTOL * sum_{j<=i} |x_j| of the float64
reference (tests/cumulative_ref.py check_cum: the bound tests/agg_edges.py compare() gives the sum aggregate -- the scan adds in another association than a loop,
nothing more)."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from polars_amd import _ffi as F
from tests import cumulative_ref as R
from tests import plugin_abi as P

pytestmark = pytest.mark.gpu

TILE = 2048
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5)
BIG = 2048 * 2048 + 3
WHOLE, SORTED, EMPTY = "cumulative[whole column]", "cumulative[sorted rows:", "cumulative[empty]"
PATTERNS = ("one", "each", "three_tiles", "tile_first", "tile_last", "wave_edges", "random")


def frame_of(pl, cols, dtypes=None):
    return pl.DataFrame([pl.Series(name, v, (dtypes or {}).get(name), validity=m) for name, (v, m) in cols.items()])


def cells(series):
    """(values, valid as a bool array or None)"""
    return series._download()


def fns(c, name, reverse=False):
    return {"cum_sum": c.cum_sum, "cum_min": c.cum_min, "cum_max": c.cum_max, "cum_count": c.cum_count}[name](reverse=reverse)


def lengths(pattern, n, rng):
    """partition lengths that sum to n"""
    def fill(first):
        out, used = [], 0
        for ln in first:
            ln = min(ln, n - used)
            if ln > 0:
                out.append(ln); used += ln
        return out + ([n - used] if used < n else [])
    if pattern == "one":
        return fill([n])
    if pattern == "each":
        return [1] * n
    if pattern == "three_tiles":                       # a partition over three whole tiles and more: the carry through a tile without a head
        return fill([5, 3 * TILE + 700])
    if pattern == "tile_first":                        # a head exactly on a tile's first row
        return fill([TILE])
    if pattern == "tile_last":                         # a head on a tile's last row
        return fill([TILE - 1, 1])
    if pattern == "wave_edges":                        # heads on a wave's lane 0 (position 512 k) and lane 63 (position 512 k + 504)
        out, used = [], 0
        while used < n:
            ln = min(n - used, 8 if len(out) & 1 else 504)
            out.append(ln); used += ln
        return out
    out, used = [], 0
    while used < n:
        ln = min(n - used, int(rng.integers(1, 301)))
        out.append(ln); used += ln
    return out


def contiguous_keys(pattern, n, rng):
    """an Int32 key column whose partitions are the runs of `lengths` in row order: the key-sorted order is the row order, so the heads fall where the pattern says"""
    lens = lengths(pattern, n, rng)
    return np.repeat(np.arange(len(lens), dtype=np.int32), lens)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_whole_column_and_over(pl, n):
    rng = np.random.default_rng(4180 + n)
    i = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    x, xm = rng.normal(5.0, 2.0, n), rng.random(n) > 0.2
    k, km = rng.integers(-2, max(n // 5, 1) - 2, n).astype(np.int32), rng.random(n) > 0.1
    df = frame_of(pl, {"k": (k, km), "i": (i, None), "x": (x, xm)})
    c = pl.col
    names = [(op, rev) for op in R.OPS for rev in (False, True)]
    out = df.select(*[fns(c("x"), op, rev).alias(f"{op}_{int(rev)}") for op, rev in names], c("i").cum_sum().alias("isum"))
    plan = pl.last_plan()
    assert plan.count("Cumulative{") == 1 and "fns=9" in plan and (EMPTY if n == 0 else WHOLE) in plan and "keys=[]" in plan and f"rows={n}" in plan, plan
    for op, rev in names:
        R.check_cum(*cells(out[f"{op}_{int(rev)}"]), op, x, xm, None, rev, what=(n, op, rev))
    R.check_cum(*cells(out["isum"]), "cum_sum", i, None, None, False, what=(n, "isum"))
    out = df.select(*[fns(c("x"), op, rev).over("k").alias(f"{op}_{int(rev)}") for op, rev in names], c("i").cum_sum().over("k").alias("isum"))
    plan = pl.last_plan()
    assert plan.count("Cumulative{") == 1 and "fns=9" in plan and (EMPTY if n == 0 else SORTED) in plan and "keys=[k]" in plan, plan
    for op, rev in names:
        R.check_cum(*cells(out[f"{op}_{int(rev)}"]), op, x, xm, [(k, km)], rev, what=(n, "over", op, rev))
    R.check_cum(*cells(out["isum"]), "cum_sum", i, None, [(k, km)], False, what=(n, "over", "isum"))


@pytest.mark.parametrize("op", R.OPS)
def test_the_recursive_level_of_the_tile_aggregates(pl, op):
    """2048 * 2048 + 3 rows: 2049 tile aggregates, one more than one workgroup scans, so the aggregates are reduced and scanned a level up"""
    rng = np.random.default_rng(4181)
    x = rng.integers(-(1 << 31), 1 << 31, BIG, dtype=np.int64).astype(np.int32)
    xm = rng.random(BIG) > 0.1
    s = pl.Series("x", x, validity=xm)
    out = {"cum_sum": s.cum_sum, "cum_min": s.cum_min, "cum_max": s.cum_max, "cum_count": s.cum_count}[op]()
    assert WHOLE in pl.last_plan(), pl.last_plan()
    R.check_cum(*cells(out), op, x, xm, None, False, what=("big", op))


# ---- segment patterns, through .over -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", (2 * 2048 + 5, BIG))
def test_segment_patterns(pl, pattern, n):
    rng = np.random.default_rng(4182)
    k = contiguous_keys(pattern, n, rng)
    x = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    xm = rng.random(n) > 0.15
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    c = pl.col
    big = n == BIG
    names = [(op, rev) for op in R.OPS for rev in ((False,) if big and op != "cum_sum" else (False, True))]      # the large size: every op once, one of them mirrored
    out = df.select(*[fns(c("x"), op, rev).over("k").alias(f"{op}_{int(rev)}") for op, rev in names])
    assert SORTED in pl.last_plan() and pl.last_plan().count("Cumulative{") == 1, pl.last_plan()
    for op, rev in names:
        R.check_cum(*cells(out[f"{op}_{int(rev)}"]), op, x, xm, [(k, None)], rev, what=(pattern, n, op, rev))


# ---- validity -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("validity", ("none", "random", "heads", "all_null_partition"))
def test_validity_patterns_with_payloads_under_the_nulls(pl, validity):
    rng = np.random.default_rng(4183)
    n = 2 * 2048 + 5
    k = contiguous_keys("random", n, rng)
    heads = np.r_[True, k[1:] != k[:-1]]
    ok = {"none": None, "random": rng.random(n) > 0.3, "heads": ~heads, "all_null_partition": k != k[n // 2]}[validity]
    mask = np.ones(n, bool) if ok is None else ok
    f = rng.normal(0.0, 100.0, n)
    i = rng.integers(-1000, 1000, n).astype(np.int16)
    f[~mask] = np.nan                                   # what a null row carries would show: NaN in a float sum, the type's extremes in min / max
    i[~mask] = np.where(rng.random(int((~mask).sum())) < 0.5, np.iinfo(np.int16).min, np.iinfo(np.int16).max)
    df = frame_of(pl, {"k": (k, None), "f": (f, ok), "i": (i, ok)})
    c = pl.col
    for rev in (False, True):
        out = df.select(*[fns(c(col), op, rev).over("k").alias(f"{col}_{op}") for col in ("f", "i") for op in R.OPS],
                        *[fns(c(col), op, rev).alias(f"w_{col}_{op}") for col in ("f", "i") for op in R.OPS])
        for col, v in (("f", f), ("i", i)):
            for op in R.OPS:
                R.check_cum(*cells(out[f"{col}_{op}"]), op, v, ok, [(k, None)], rev, what=(validity, col, op, rev))
                R.check_cum(*cells(out[f"w_{col}_{op}"]), op, v, ok, None, rev, what=(validity, "whole", col, op, rev))


# ---- values and dtypes --------------------------------------------------------------------------------------------------------------------------------------
DTYPES = (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype_with_its_result_dtype_and_values_at_the_bounds(pl, dtype):
    rng = np.random.default_rng(4184)
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
    for keys, over in ((None, False), ([(k, None)], True)):
        wrap = (lambda e: e.over("k")) if over else (lambda e: e)
        for rev in (False, True):
            out = df.select(*[wrap(fns(c("x"), op, rev)).alias(op) for op in R.OPS])
            for op in R.OPS:
                v, ok = cells(out[op])
                assert v.dtype == R.result_dtype(op, dt), (dt, op, v.dtype)
                assert out[op].dtype == pl.datatypes.NP_TO_DTYPE[R.result_dtype(op, dt)], (dt, op, out[op].dtype)
                R.check_cum(v, ok, op, x, xm, keys, rev, what=(dt.name, op, over, rev))


def test_nan_and_infinities(pl):
    nan, inf = np.nan, np.inf
    c = pl.col
    cases = {"nan_first": [nan, 1.0, 2.0, -1.0], "nan_last": [1.0, 2.0, -1.0, nan], "nan_alone": [nan], "nan_mid": [3.0, nan, 1.0, nan, 2.0],
             "inf_then_minus_inf": [1.0, inf, 2.0, -inf, 3.0, 4.0], "minus_inf_first": [-inf, 5.0, inf, 1.0], "all_nan": [nan, nan, nan],
             "zeros": [-0.0, 0.0, -0.0, 1.0, -1.0, 0.0]}
    for dt in (np.float64, np.float32):
        for name, vals in cases.items():
            x = np.array(vals, dt)
            s = pl.Series("x", x)
            for op, fn in (("cum_sum", s.cum_sum), ("cum_min", s.cum_min), ("cum_max", s.cum_max)):
                for rev in (False, True):
                    R.check_cum(*cells(fn(reverse=rev)), op, x, None, None, rev, what=(name, dt.__name__, op, rev))
        # the same vectors side by side as partitions of one column: a NaN or an infinity stays inside its own partition
        x = np.concatenate([np.array(v, dt) for v in cases.values()])
        k = np.concatenate([np.full(len(v), j, np.int32) for j, v in enumerate(cases.values())])
        perm = np.random.default_rng(4185).permutation(len(x))
        x, k = x[perm], k[perm]
        out = frame_of(pl, {"k": (k, None), "x": (x, None)}).select(*[fns(c("x"), op).over("k").alias(op) for op in ("cum_sum", "cum_min", "cum_max")])
        for op in ("cum_sum", "cum_min", "cum_max"):
            R.check_cum(*cells(out[op]), op, x, None, [(k, None)], False, what=("partitions", dt.__name__, op))


def test_integer_valued_floats_are_bit_exact_and_runs_are_bit_identical(pl):
    rng = np.random.default_rng(4186)
    n = 3 * 2048 + 77
    x = rng.integers(-1000, 1000, n).astype(np.float64)           # every partial sum is an integer below 2^53: any association gives the same bits
    k = rng.integers(0, 50, n).astype(np.int32)
    df = frame_of(pl, {"k": (k, None), "x": (x, None), "y": (rng.normal(size=n), None)})
    c = pl.col
    q = df.lazy().select(c("x").cum_sum().alias("w"), c("x").cum_sum().over("k").alias("o"), c("y").cum_sum().alias("yw"), c("y").cum_sum(reverse=True).over("k").alias("yo"))
    a, b = q.collect(), q.collect()
    want, _, _ = R.cum("cum_sum", x)
    assert a["w"].to_numpy().view(np.uint64).tolist() == want.view(np.uint64).tolist()
    want, _, _ = R.cum("cum_sum", x, None, [(k, None)])
    assert a["o"].to_numpy().view(np.uint64).tolist() == want.view(np.uint64).tolist()
    for name in ("w", "o", "yw", "yo"):                                  # two runs of the same input: the same bits
        assert np.array_equal(a[name].to_numpy().view(np.uint64), b[name].to_numpy().view(np.uint64)), name


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_key_dtypes_and_key_edges(pl):
    rng = np.random.default_rng(4187)
    n = 700
    x, xm = rng.integers(-99, 99, n).astype(np.int64), rng.random(n) > 0.1
    f = rng.integers(0, 4, n).astype(np.float64)
    f[rng.random(n) < 0.2] = np.nan                                      # NaN == NaN: one partition
    f[rng.random(n) < 0.1] = -0.0                                        # -0 == +0
    keys = {"i8": (rng.integers(-3, 3, n).astype(np.int8), rng.random(n) > 0.2), "u64": (rng.integers(0, 1 << 64, 5, dtype=np.uint64)[rng.integers(0, 5, n)], None),
            "i64": (np.array([-(1 << 63), (1 << 63) - 1, 0, -1], np.int64)[rng.integers(0, 4, n)], None),          # full-range Int64
            "f64": (f, rng.random(n) > 0.1), "f32": (rng.integers(0, 3, n).astype(np.float32), None), "b": (rng.random(n) < 0.5, rng.random(n) > 0.2)}
    df = frame_of(pl, dict(keys, x=(x, xm)))
    c = pl.col
    for name, (kv, km) in keys.items():
        out = df.select(c("x").cum_sum().over(name).alias("s"), c("x").cum_max(reverse=True).over(name).alias("m"))
        assert SORTED in pl.last_plan() and f"keys=[{name}]" in pl.last_plan(), pl.last_plan()
        R.check_cum(*cells(out["s"]), "cum_sum", x, xm, [(kv, km)], False, what=name)
        R.check_cum(*cells(out["m"]), "cum_max", x, xm, [(kv, km)], True, what=name)
    out = df.select(c("x").cum_count().over("i8", "f64", "b").alias("n"), c("x").cum_sum().over(*["i8"] * 8).alias("s8"))
    assert pl.last_plan().count("Cumulative{") == 2 and "keys=[i8, f64, b]" in pl.last_plan(), pl.last_plan()
    R.check_cum(*cells(out["n"]), "cum_count", x, xm, [keys["i8"], keys["f64"], keys["b"]], False, what="three keys")
    R.check_cum(*cells(out["s8"]), "cum_sum", x, xm, [keys["i8"]], False, what="eight keys")
    with pytest.raises(pl.UnsupportedError, match="1..8"):
        df.select(c("x").cum_sum().over(*["i8"] * 9))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(4188)
    n = 1000
    return {"k": (rng.integers(0, 40, n).astype(np.int32), rng.random(n) > 0.05), "g": (rng.integers(0, 5, n).astype(np.int64), None),
            "x": (rng.integers(-50, 50, n).astype(np.float64), rng.random(n) > 0.1), "i": (rng.integers(-500, 500, n).astype(np.int64), None)}


def test_in_select_with_columns_filter_and_inside_expressions(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (g, _), (x, xm), (i, _) = (table[nm] for nm in ("k", "g", "x", "i"))
    n = len(k)
    out = df.with_columns((c("i") * c("g")).cum_sum().over("k").alias("run"), c("i").cum_max().alias("hi"), c("i").cum_sum().over("g", "k").alias("gk"))
    plan = pl.last_plan()
    assert out.columns == ["k", "g", "x", "i", "run", "hi", "gk"] and out.height == n and plan.count("Cumulative{") == 3, plan
    assert "keys=[k]" in plan and "keys=[g, k]" in plan and "keys=[]" in plan and WHOLE in plan and SORTED in plan, plan
    R.check_cum(*cells(out["run"]), "cum_sum", i * g, None, [(k, km)], what="operand expression")
    R.check_cum(*cells(out["hi"]), "cum_max", i, None, None, what="hi")
    R.check_cum(*cells(out["gk"]), "cum_sum", i, None, [(g, None), (k, km)], what="gk")
    assert np.array_equal(out["i"].to_numpy(), i)
    # two functions over [k] and the same operand: one bucket, one sort
    out = df.select(c("i").cum_sum().over("k").alias("a"), c("i").cum_min().over("k").alias("b"), (c("i").cum_sum().over("k") - c("i")).alias("before"),
                    pl.when(c("i").cum_sum().over("k") > 0).then(c("i")).otherwise(c("i").cum_count().over("k").cast(pl.Int64)).alias("w"))
    plan = pl.last_plan()
    assert plan.count("Cumulative{") == 1 and "fns=5" in plan, plan
    run, _, _ = R.cum("cum_sum", i, None, [(k, km)])
    cnt, _, _ = R.cum("cum_count", i, None, [(k, km)])
    assert np.array_equal(out["before"].to_numpy(), run - i) and np.array_equal(out["w"].to_numpy(), np.where(run > 0, i, cnt.astype(np.int64)))
    # as a filter predicate
    kept = df.filter(c("i").cum_sum().over("k") > 100)
    assert "Cumulative{" in pl.last_plan() and "cumulative / ranking expression: per-node route" in pl.last_plan(), pl.last_plan()
    assert kept.height == int((run > 100).sum()) and np.array_equal(kept["i"].to_numpy(), i[run > 100])
    kept = df.filter((c("x").cum_count() <= 10) & (c("i") > -1000))
    cnt, _, _ = R.cum("cum_count", x, xm)
    assert np.array_equal(kept["i"].to_numpy(), i[cnt <= 10])


def test_after_a_filter_after_a_join_lazy_and_no_fusion(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (g, _), (i, _) = (table[nm] for nm in ("k", "g", "i"))
    keep = i > 0
    q = df.lazy().filter(c("i") > 0).with_columns(c("i").cum_sum().over("k").alias("s"), c("i").cum_count(reverse=True).alias("left"))
    a, b = q.collect(), q.collect(no_fusion=True)
    for out in (a, b):
        assert out.height == int(keep.sum())
        R.check_cum(*cells(out["s"]), "cum_sum", i[keep], None, [(k[keep], km[keep])], what="after filter")
        R.check_cum(*cells(out["left"]), "cum_count", i[keep], None, None, True, what="after filter")
    eager = df.filter(c("i") > 0).with_columns(c("i").cum_sum().over("k").alias("s"), c("i").cum_count(reverse=True).alias("left"))
    assert eager.to_dict() == a.to_dict() == b.to_dict()
    right = frame_of(pl, {"g": (np.arange(5, dtype=np.int64), None), "w": (np.array([3, 1, 3, 2, 1], np.int32), None)})
    out = df.lazy().join(right.lazy(), on="g", how="inner", maintain_order="left").with_columns(c("i").cum_sum().over("w").alias("s")).collect()
    w = np.array([3, 1, 3, 2, 1], np.int32)[g]
    assert out.height == len(g) and np.array_equal(out["i"].to_numpy(), i)
    R.check_cum(*cells(out["s"]), "cum_sum", i, None, [(w, None)], what="after join")
    # an empty frame: empty columns of the right dtype
    out = df.filter(c("i") > 10_000).select(c("i").cum_sum().over("k").alias("s"), c("x").cum_count().alias("n"), c("g").cast(pl.Int8).cum_sum().alias("w"))
    assert out.height == 0 and (out["s"].dtype, out["n"].dtype, out["w"].dtype) == (pl.Int64, pl.UInt32, pl.Int64) and EMPTY in pl.last_plan(), pl.last_plan()


def test_refusals(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    with pytest.raises(TypeError, match="group_by"):
        df.lazy().group_by("g").agg(c("x").cum_sum()).collect()
    with pytest.raises(TypeError, match="group_by"):
        df.lazy().group_by(c("i").cum_sum().over("k")).agg(c("x").sum()).collect()
    with pytest.raises(TypeError, match="an aggregate"):
        df.select(c("x").sum().cum_sum())
    with pytest.raises(TypeError, match="a window expression"):
        df.select(c("x").sum().over("k").cum_sum())
    with pytest.raises(TypeError, match="inside the operand of another one"):
        df.select(c("x").cum_sum().cum_max())
    with pytest.raises(TypeError, match="mixes a cumulative / ranking expression"):
        df.select((c("x").cum_sum() / c("x").sum()).over("k"))
    out = df.select((c("x").cum_sum().over("k") / c("x").sum().over("k")).alias("share"))          # the arithmetic outside the two .over()s
    assert out.height == df.height and "Cumulative{" in pl.last_plan() and "Window{" in pl.last_plan()
    # what stays refused exactly as before
    with pytest.raises(pl.UnsupportedError, match="window functions that do not aggregate"):
        df.select(c("x").over("k"))
    with pytest.raises(pl.UnsupportedError, match="window functions that do not aggregate"):
        df.select((c("x") - c("x").mean()).over("k"))
    with pytest.raises(ValueError, match="order_by"):
        c("x").cum_sum().over("k", order_by="i")
    with pytest.raises(ValueError, match="mapping_strategy"):
        c("x").cum_sum().over("k", mapping_strategy="explode")
    d = pl.DataFrame([pl.Series("d", np.arange(5, dtype=np.int32), pl.Date), pl.Series("s", np.array([0, 1, 0, 1, 0], np.uint8), pl.Categorical(["a", "b"], pl.UInt8))])
    with pytest.raises(TypeError, match="cum_sum"):
        d.select(c("d").cum_sum())
    for e in (c("s").cum_sum(), c("s").cum_min(), c("s").cum_max()):
        with pytest.raises(TypeError, match="Categorical|cum_"):
            d.select(e)
    out = d.select(c("d").cum_max().alias("m"), c("s").cum_count().alias("n"), c("d").cum_min(reverse=True).alias("r"))          # temporal min / max and any count are served
    days = lambda s: np.asarray(cells(s)[0]).astype(np.int64).tolist()
    assert out["m"].dtype == pl.Date and days(out["m"]) == [0, 1, 2, 3, 4] and days(out["n"]) == [1, 2, 3, 4, 5] and days(out["r"]) == [0, 1, 2, 3, 4]


def test_example_query(pl):
    from polars_amd import queries as QQ
    rng = np.random.default_rng(4189)
    n = 3000
    flag, status = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
    price, disc = rng.uniform(900.0, 100000.0, n), rng.integers(0, 11, n) / 100.0
    df = frame_of(pl, {"l_returnflag": (flag, None), "l_linestatus": (status, None), "l_extendedprice": (price, None), "l_discount": (disc, None)})
    out = QQ.running_revenue_by_flag(df.lazy()).collect()
    assert pl.last_plan().count("Cumulative{") == 1 and SORTED in pl.last_plan(), pl.last_plan()
    assert out.height == n
    R.check_cum(*cells(out["running_revenue"]), "cum_sum", price * (1.0 - disc), None, [(flag, None), (status, None)], what="running revenue")


# ---- the C entry and the plugin symbol ----------------------------------------------------------------------------------------------------------------------
def test_c_entry_and_plugin_symbol(pl):
    rng = np.random.default_rng(4190)
    n = 2100
    k, km = rng.integers(0, 9, n).astype(np.int32), rng.random(n) > 0.1
    x, xm = rng.normal(2.0, 1.0, n), rng.random(n) > 0.2
    i = rng.integers(-50, 50, n).astype(np.int8)
    ks, xs, isr = pl.Series("k", k, validity=km), pl.Series("x", x, validity=xm), pl.Series("i", i)
    out = C.c_uint64()
    F.check(F.lib().plx_cumulative((C.c_uint64 * 1)(ks._h), 1, isr._h, F.CUM_SUM, 1, C.byref(out)))
    plan = F.lib().plx_last_plan_description().decode()
    assert "Cumulative{keys=[1 columns], fns=1" in plan and SORTED in plan, plan
    R.check_cum(*cells(pl.Series._from_handle("s", out.value, pl.Int64)), "cum_sum", i, None, [(k, km)], True, what="C over")
    F.check(F.lib().plx_cumulative(None, 0, xs._h, F.CUM_MIN, 0, C.byref(out)))
    assert WHOLE in F.lib().plx_last_plan_description().decode()
    R.check_cum(*cells(pl.Series._from_handle("m", out.value, pl.Float64)), "cum_min", x, xm, None, False, what="C whole")
    # parameters are refused by name before anything runs, an empty input included
    empty = pl.Series("e", np.zeros(0, np.int64))
    for col in (xs, empty):
        assert F.lib().plx_cumulative(None, 0, col._h, 4, 0, C.byref(out)) == 1 and "no plx_cum_op" in F.lib().plx_last_error().decode()
        assert F.lib().plx_cumulative(None, 0, col._h, F.CUM_SUM, 2, C.byref(out)) == 1 and "reverse must be 0 or 1" in F.lib().plx_last_error().decode()
    F.check(F.lib().plx_cumulative(None, 0, empty._h, F.CUM_COUNT, 0, C.byref(out)))
    e = pl.Series._from_handle("n", out.value, pl.UInt32)
    assert len(e) == 0 and EMPTY in F.lib().plx_last_plan_description().decode()
    nine = (C.c_uint64 * 9)(*([ks._h] * 9))
    assert F.lib().plx_cumulative(nine, 9, xs._h, F.CUM_SUM, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in F.lib().plx_last_error().decode()
    # the plugin symbol: the value series, then the key series
    arr_x, arr_k = pa.array(x, mask=~xm), pa.array(k, mask=~km)
    res, inp = P.call("plx_cum", [arr_x, arr_k], {"op": "sum", "reverse": False}, names=["x", "k"])
    assert res is not None and inp.released == 2 and inp.out_name == b"x" and res.type == pa.float64() and len(res) == n, P.last_error()
    R.check_cum(np.asarray(res.fill_null(0.0)), ~np.asarray(res.is_null()), "cum_sum", x, xm, [(k, km)], False, what="plugin over")
    res, _ = P.call("plx_cum", [pa.array(i)], {"op": "max", "reverse": True})
    assert res is not None and res.type == pa.int8(), P.last_error()
    R.check_cum(np.asarray(res), None, "cum_max", i, None, None, True, what="plugin whole, reverse")
    res, _ = P.call("plx_cum", [arr_x], {"op": "count"})
    assert res is not None and res.type == pa.uint32() and res.null_count == 0, P.last_error()
    R.check_cum(np.asarray(res), None, "cum_count", x, xm, None, False, what="plugin count")
    for arrs in ([arr_x, arr_k], [arr_x.slice(0, 0), arr_k.slice(0, 0)]):
        res, inp = P.call("plx_cum", arrs, {"op": "prod"})
        assert res is None and inp.released == 2 and "kwargs must carry op in {sum, min, max, count}" in P.last_error(), P.last_error()
        res, inp = P.call("plx_cum", arrs, {"op": "sum", "reverse": "yes"})
        assert res is None and "reverse must be a bool" in P.last_error(), P.last_error()
    # what the window plugin keeps refusing
    res, inp = P.call("plx_window_agg", [arr_x, arr_k], {"agg": "cum_sum"})
    assert res is None and "kwargs must carry agg" in P.last_error()
