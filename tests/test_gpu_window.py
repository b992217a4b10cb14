"""Window expressions on the device: `f.over(keys)` in select / with_columns / filter against tests/window_ref.py, row by row in row order.

Sizes around the ballot word (64), the wave tile and the sort's one-workgroup and tile sizes, each on both routes of the row -> group map with the route asserted in
pl.last_plan(); the route rule just inside and just outside its bound; every aggregate kind over Int64 and Float64 sources (and Float32, Int8, UInt64, Boolean where
the aggregate takes them) with three validity patterns; the key dtypes and the key edges (null parts, NaN, signed zeros, full-range Int64); the shapes a window may
stand in; the refusals; the C entry and the plugin symbol.

Exact where the aggregate is exact (integer sum / min / max, count, len, n_unique, the picking quantiles); float sum / mean within tests/agg_edges.py compare()
(RTOL * sum |x|: the bound test_gpu_agg_edges.py applies to the same aggregates of a group-by), var / std within tests/program_eval_var.py within_contract (the bound
of test_gpu_var_std.py), interpolating quantiles within tests/quantile_ref.py accept (the bound of test_gpu_quantile.py).  Whatever the tolerance, all rows of one
partition hold bit-identical values."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from polars_amd import _ffi as F
from tests import agg_edges as AE
from tests import groupby_route_inputs as R
from tests import plugin_abi as P
from tests import program_eval_var as pv
from tests import quantile_ref as Q
from tests import window_ref as W

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 2048, 2049, 4097, 2 * 4096 + 5)
DIRECT, SORTED, EMPTY = "window[direct range=", "window[sorted rows:", "window[empty]"


def frame_of(pl, cols, dtypes=None):
    return pl.DataFrame([pl.Series(name, v, (dtypes or {}).get(name), validity=m) for name, (v, m) in cols.items()])


def cells(series):
    """(values, valid as a bool array)"""
    v, ok = series._download()
    return v, (np.ones(len(v), bool) if ok is None else ok)


class Host:
    """a pyarrow result where check() expects a Series"""

    def __init__(self, arr):
        self.ok = ~np.asarray(arr.is_null())
        self.v = np.asarray(arr.fill_null(0) if arr.null_count else arr)

    def _download(self):
        return self.v, self.ok


def check(series, keys, values, valid, op, what, ddof=1, q=0.5, interpolation="linear"):
    """one window column against the reference: validity bit for bit, the rows of a partition bit-identical, one comparison per partition"""
    params = {"ddof": ddof} if op in ("var", "std") else {"q": q, "interpolation": interpolation} if op == "quantile" else {}
    want, ids = W.over(keys, values, valid, op, **params)
    got, ok = cells(series)
    assert len(got) == len(want), (what, len(got), len(want))
    assert ok.tolist() == [w is not None for w in want], (what, "validity")
    bits = got if got.dtype == np.bool_ else got.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize])
    name = None if values is None else W.NP_NAME[np.asarray(values).dtype]
    vals = None if values is None else np.asarray(values)
    okv = None if values is None else (np.ones(len(vals), bool) if valid is None else np.asarray(valid, bool))
    D = 0.0
    if op in ("var", "std") and okv.any():
        xs = vals[okv].astype(np.float64)
        D = float(xs.max() - xs.min())                                   # the spread of the column, as in tests/test_gpu_var_std.py
    firsts = {}
    for r, g in enumerate(ids.tolist()):
        firsts.setdefault(g, r)
    for g, r in firsts.items():
        sel = ids == g
        if ok[r]:
            assert (bits[sel] == bits[r]).all(), (what, "rows of partition", g, "differ in their bits")
        if want[r] is None:
            continue
        gv = got[r].item()
        if op in ("count", "len", "n_unique"):
            assert gv == want[r], (what, op, g, gv, want[r])
        elif op in ("var", "std"):
            assert pv.within_contract(gv, vals[sel & okv].astype(np.float64), ddof, D, want_std=op == "std", f32=name == "Float32"), (what, op, g, gv, want[r])
        elif op == "quantile":
            assert Q.accept(gv, vals[sel & okv], q, interpolation, f32=name == "Float32"), (what, op, q, interpolation, g, gv, want[r])
        else:
            AE.compare(gv, want[r], name, op, list(zip(vals[sel].tolist(), okv[sel].tolist())), what=(what, g))
    return ids


def draw(rng, name, n):
    npdt = AE.NP[name]
    if name == "Boolean":
        return rng.random(n) < 0.5
    if name == "Int64":
        return rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    if name == "UInt64":
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)              # above 2^63: a signed conversion would show (tests/test_gpu_var_std.py draw)
    if name == "Int8":
        return rng.integers(-128, 128, n).astype(np.int8)
    return rng.normal(10.0, 3.0, n).astype(npdt)


# ---- sizes and routes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_on_both_routes(pl, monkeypatch, n):
    rng = np.random.default_rng(4170 + n)
    k = rng.integers(-2, max(n // 3, 1) - 2, n).astype(np.int32)
    km = rng.random(n) > 0.1
    x, xm = rng.normal(5.0, 2.0, n), rng.random(n) > 0.2
    i = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    flag = rng.random(n) < 0.5
    df = frame_of(pl, {"k": (k, km), "x": (x, xm), "i": (i, None), "flag": (flag, xm)})
    c = pl.col
    exprs = [c("i").sum().over("k").alias("isum"), c("x").mean().over("k").alias("xmean"), pl.len().over("k").alias("n"), c("flag").sum().over("k").alias("trues"),
             c("x").max().over("k").alias("xmax")]
    keys = [(k, km)]
    for route, word in (("direct", DIRECT), ("sort", SORTED)):
        monkeypatch.setenv("PLX_WINDOW_ROUTE", route)
        out = df.lazy().select(*exprs).collect()
        plan = pl.last_plan()
        assert (EMPTY if n == 0 else word) in plan and plan.count("Window{") == 1, (route, plan)
        assert "Window{keys=[k], aggs=5, groups=" + ("0, rows=0, " if n == 0 else "") in plan, plan          # one shape of text, the empty frame included
        assert out.height == n and out.schema == {"isum": pl.Int64, "xmean": pl.Float64, "n": pl.UInt32, "trues": pl.UInt32, "xmax": pl.Float64}, out.schema
        what = (n, route)
        check(out["isum"], keys, i, None, "sum", what)
        check(out["xmean"], keys, x, xm, "mean", what)
        check(out["n"], keys, None, None, "len", what)
        check(out["trues"], keys, flag, xm, "sum", what)
        check(out["xmax"], keys, x, xm, "max", what)


def test_route_bound_inside_and_outside(pl, monkeypatch):
    """2049 rows: the rule admits 4 R <= max(8 n, 4 MiB) = 4 MiB, i.e. R <= 1048576.  The key's range is exactly that, then one more."""
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    n = 2049
    rng = np.random.default_rng(5)
    base = rng.integers(1, 40, n).astype(np.int32)
    i = rng.integers(-1000, 1000, n).astype(np.int64)
    for top, word in ((1048575, "window[direct range=1048576]"), (1048576, SORTED)):
        k = base.copy()
        k[0], k[7] = 0, top
        df = frame_of(pl, {"k": (k, None), "i": (i, None)})
        out = df.with_columns(pl.col("i").sum().over("k").alias("s"))
        assert word in pl.last_plan(), (top, pl.last_plan())
        check(out["s"], [(k, None)], i, None, "sum", top)
    # with a validity bitmap the null takes one more code: the same values are one beyond the bound
    k = base.copy()
    k[0], k[7] = 0, 1048575
    km = np.ones(n, bool)
    km[3] = False
    out = frame_of(pl, {"k": (k, km), "i": (i, None)}).with_columns(pl.col("i").sum().over("k").alias("s"))
    assert SORTED in pl.last_plan(), pl.last_plan()
    check(out["s"], [(k, km)], i, None, "sum", "nullable at the bound")


# ---- every aggregate kind ---------------------------------------------------------------------------------------------------------------------
AGGS = {"sum": lambda e: e.sum(), "mean": lambda e: e.mean(), "min": lambda e: e.min(), "max": lambda e: e.max(), "count": lambda e: e.count(), "len": lambda e: e.len(),
        "n_unique": lambda e: e.n_unique()}
NUMERIC = tuple(AGGS) + ("var", "std", "quantile")                       # every kind a numeric source takes
SOURCES = {"Int64": NUMERIC, "Float64": NUMERIC, "Float32": NUMERIC, "Int8": NUMERIC, "UInt64": NUMERIC,
           "Boolean": ("sum", "mean", "count", "len", "n_unique")}      # tests/agg_edges.py ops_of: a Boolean has no min / max; var, std and quantiles refuse it
QUANTILES = ((0.5, "linear"), (0.25, "lower"), (0.75, "higher"), (0.5, "nearest"), (1.0 / 3.0, "midpoint"))
OUT_DTYPE = {"count": "UInt32", "len": "UInt32", "n_unique": "UInt32"}


def want_dtype(pl, dtype, op):
    """the dtype the aggregate has in group_by: Float32 stays Float32, counts are UInt32, integer sums follow the SumCast rule (tests/agg_edges.py out_dtype)"""
    if op in ("var", "std", "quantile"):
        return pl.Float32 if dtype == "Float32" else pl.Float64
    return getattr(pl, OUT_DTYPE.get(op) or AE.out_dtype(dtype, op))


@pytest.mark.parametrize("validity", ["none", "some", "all_null"])
@pytest.mark.parametrize("dtype", list(SOURCES))
def test_every_aggregate_kind(pl, monkeypatch, dtype, validity):
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    n = 389
    rng = np.random.default_rng(900 + list(SOURCES).index(dtype))
    k = rng.integers(0, n // 3, n).astype(np.int32)
    v = draw(rng, dtype, n)
    m = None if validity == "none" else (rng.random(n) > 0.3 if validity == "some" else np.zeros(n, bool))
    df = frame_of(pl, {"k": (k, None), "v": (v, m)}, {"v": getattr(pl, dtype)})
    c = pl.col
    # the full list in lists of at most 16 aggregate cells each (one group-by holds 16; a Float32 source is widened once per aggregate, so its cells are not
    # shared): the plain kinds (8 cells), var at both ddof (6), std at both ddof (6), the quantiles (no cells)
    chunks = [[(op, op, {}, AGGS[op](c("v"))) for op in SOURCES[dtype] if op in AGGS]]
    for op in ("var", "std"):
        if op in SOURCES[dtype]:
            chunks.append([(f"{op}{ddof}", op, {"ddof": ddof}, c("v").var(ddof) if op == "var" else c("v").std(ddof)) for ddof in (0, 1)])
    if "quantile" in SOURCES[dtype]:
        chunks.append([(f"q{j}", "quantile", {"q": q, "interpolation": ip}, c("v").quantile(q, ip)) for j, (q, ip) in enumerate(QUANTILES)])
    seen = set()
    for chunk in chunks:
        out = df.select(*[f.over("k").alias(name) for name, _, _, f in chunk])
        plan = pl.last_plan()
        assert plan.count("Window{") == 1 and DIRECT in plan, plan             # one key list: one group-by, one map
        gb = df.lazy().group_by("k").agg(*[f.alias(name) for name, _, _, f in chunk]).collect()
        for name, op, params, _ in chunk:
            check(out[name], [(k, None)], v, m, op, (dtype, validity, name), **params)
            assert out.schema[name] == gb.schema[name] == want_dtype(pl, dtype, op), (dtype, name, out.schema[name], gb.schema[name])
            seen.add(op)
    assert seen == set(SOURCES[dtype])


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------------
def key_case(pl, monkeypatch, cols, key_names, dtypes=None, keys_ref=None, word=None, routes=("direct", "sort")):
    """len and an exact integer sum over the keys, on the routes given; -> the partition ids"""
    n = len(next(iter(cols.values()))[0])
    rng = np.random.default_rng(n)
    i = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    df = frame_of(pl, dict(cols, i=(i, None)), dtypes)
    keys_ref = keys_ref or [cols[kn] for kn in key_names]
    ids = None
    for route in routes:
        monkeypatch.setenv("PLX_WINDOW_ROUTE", route)
        out = df.with_columns(pl.col("i").sum().over(*key_names).alias("s"), pl.len().over(key_names).alias("cnt"))
        plan = pl.last_plan()
        assert (word or (DIRECT if route == "direct" else SORTED)) in plan and plan.count("Window{") == 1, (route, plan)
        ids = check(out["s"], keys_ref, i, None, "sum", (key_names, route))
        check(out["cnt"], keys_ref, None, None, "len", (key_names, route))
    return ids


def test_null_keys_in_one_and_both_parts(pl, monkeypatch):
    n = 257
    rng = np.random.default_rng(31)
    a, am = rng.integers(0, 3, n).astype(np.int64), rng.random(n) > 0.3
    b, bm = rng.integers(1, 3, n).astype(np.int16), rng.random(n) > 0.3
    ids = key_case(pl, monkeypatch, {"a": (a, am)}, ["a"])
    assert len(set(ids.tolist())) == 4                                   # three values and the null partition
    ids = key_case(pl, monkeypatch, {"a": (a, am), "b": (b, bm)}, ["a", "b"])
    assert len(set(ids.tolist())) == 4 * 3                               # per part: (null, 1) != (null, 2) != (null, null)
    both_null = ~am & ~bm
    assert both_null.any() and len(set(ids[both_null].tolist())) == 1
    null_one, null_two = ~am & bm & (b == 1), ~am & bm & (b == 2)
    assert set(ids[null_one].tolist()).isdisjoint(ids[null_two].tolist())


def test_float_keys_nan_and_signed_zero(pl, monkeypatch):
    nan2 = np.array([0x7FF8000000000001, 0xFFF8000000000000], np.uint64).view(np.float64)
    f = np.tile(np.array([0.0, -0.0, nan2[0], nan2[1], 1.5, -1.5, np.inf]), 30)
    fm = np.arange(len(f)) % 11 != 0
    ids = key_case(pl, monkeypatch, {"f": (f, fm)}, ["f"], word=SORTED)      # floats have no direct route: both settings sort
    assert len(set(ids.tolist())) == 6                                   # 0, NaN, 1.5, -1.5, inf, null


def test_boolean_date_month_and_categorical_keys(pl, monkeypatch):
    n = 300
    rng = np.random.default_rng(32)
    b, bm = rng.random(n) < 0.5, rng.random(n) > 0.2
    ids = key_case(pl, monkeypatch, {"b": (b, bm)}, ["b"])
    assert len(set(ids.tolist())) == 3
    d = rng.integers(10_000, 10_400, n).astype(np.int32)
    key_case(pl, monkeypatch, {"d": (d, None)}, ["d"], {"d": pl.Date})
    # d.dt.month() as a key: an expression, evaluated as a column first
    month = (d.astype("datetime64[D]").astype("datetime64[M]").astype(np.int64) % 12 + 1).astype(np.int8)
    i = rng.integers(-1000, 1000, n).astype(np.int64)
    df = frame_of(pl, {"d": (d, None), "i": (i, None)}, {"d": pl.Date})
    for route, word in (("direct", DIRECT), ("sort", SORTED)):
        monkeypatch.setenv("PLX_WINDOW_ROUTE", route)
        out = df.with_columns(pl.col("i").sum().over(pl.col("d").dt.month()).alias("s"))
        assert word in pl.last_plan(), pl.last_plan()
        check(out["s"], [(month, None)], i, None, "sum", ("month", route))
    # a Categorical key partitions by its codes
    words = [["b", "a", None, "c"][j] for j in rng.integers(0, 4, n)]
    s = pl.Series("s", words)
    codes = np.array([{"a": 0, "b": 1, "c": 2}.get(w, 0) for w in words])
    sm = np.array([w is not None for w in words])
    df = pl.DataFrame([s, pl.Series("i", i)])
    for route, word in (("direct", DIRECT), ("sort", SORTED)):
        monkeypatch.setenv("PLX_WINDOW_ROUTE", route)
        out = df.with_columns(pl.col("i").sum().over("s").alias("t"))
        assert word in pl.last_plan(), pl.last_plan()
        check(out["t"], [(codes, sm)], i, None, "sum", ("categorical", route))


def test_full_range_int64_keys_take_the_sorted_route(pl, monkeypatch):
    n = 500
    rng = np.random.default_rng(33)
    ids = rng.integers(0, 60, n)
    k1, k2 = R.full64(ids), R.full64(ids % 7 + 100)
    key_case(pl, monkeypatch, {"k1": (k1, None), "k2": (k2, None)}, ["k1", "k2"], word=SORTED)
    u = rng.integers(0, 40, n).astype(np.uint64) + np.uint64((1 << 63) + 5)      # UInt64: never direct
    key_case(pl, monkeypatch, {"u": (u, None)}, ["u"], word=SORTED)


def test_one_partition_n_partitions_and_partitions_across_words(pl, monkeypatch):
    n = 200
    ids = key_case(pl, monkeypatch, {"k": (np.full(n, 7, np.int32), None)}, ["k"])
    assert len(set(ids.tolist())) == 1
    ids = key_case(pl, monkeypatch, {"k": (np.arange(n, dtype=np.int64)[::-1].copy() * 3, None)}, ["k"])
    assert len(set(ids.tolist())) == n
    k = (np.arange(n) // 50).astype(np.int16)                          # rows 50..99 and 100..149 straddle the words that end at 64 and 128
    ids = key_case(pl, monkeypatch, {"k": (k, None)}, ["k"])
    assert ids[63] == ids[64] and ids[127] == ids[128]


def test_nine_keys_are_refused_naming_the_limit(pl):
    df = frame_of(pl, {"k": (np.arange(5, dtype=np.int32), None), "x": (np.arange(5.0), None)})
    with pytest.raises(pl.UnsupportedError, match="window over 9 keys.*1..8"):
        df.select(pl.col("x").sum().over(*["k"] * 9))
    out = df.select(pl.col("x").sum().over(*["k"] * 8))
    assert out["x"].to_numpy().tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(34)
    n = 1000
    return {"k": (rng.integers(0, 40, n).astype(np.int32), rng.random(n) > 0.05), "g": (rng.integers(0, 5, n).astype(np.int64), None), "x": (rng.uniform(1.0, 9.0, n), rng.random(n) > 0.1),
            "y": (rng.normal(0.0, 1.0, n), None), "i": (rng.integers(-500, 500, n).astype(np.int64), None)}


def test_three_windows_one_group_by_and_two_key_lists(pl, monkeypatch, table):
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (g, _), (x, xm), (y, _), (i, _) = (table[nm] for nm in ("k", "g", "x", "y", "i"))
    out = df.select(c("x").sum().over("k").alias("xs"), c("x").mean().over("k").alias("xm"), c("y").max().over("k").alias("ym"))
    plan = pl.last_plan()
    assert plan.count("Window{") == 1 and "aggs=3" in plan and "keys=[k]" in plan and f"rows={len(k)}" in plan and DIRECT in plan, plan
    check(out["xs"], [(k, km)], x, xm, "sum", "xs")
    check(out["xm"], [(k, km)], x, xm, "mean", "xm")
    check(out["ym"], [(k, km)], y, None, "max", "ym")
    out = df.with_columns(c("i").sum().over("k").alias("by_k"), c("i").sum().over("g", "k").alias("by_gk"), c("i").min().over(["k"]).alias("min_k"))
    plan = pl.last_plan()
    assert plan.count("Window{") == 2 and "keys=[k]" in plan and "keys=[g, k]" in plan and "aggs=2" in plan and "aggs=1" in plan, plan
    assert out.columns == ["k", "g", "x", "y", "i", "by_k", "by_gk", "min_k"] and out.height == len(k)
    check(out["by_k"], [(k, km)], i, None, "sum", "by_k")
    check(out["by_gk"], [(g, None), (k, km)], i, None, "sum", "by_gk")
    check(out["min_k"], [(k, km)], i, None, "min", "min_k")
    assert np.array_equal(out["i"].to_numpy(), i)                       # the frame's own columns and row order are untouched


def test_windows_inside_expressions_and_filter(pl, monkeypatch, table):
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (x, xm), (i, _) = (table[nm] for nm in ("k", "x", "i"))
    n = len(k)
    xsum, ids = W.over([(k, km)], x, xm, "sum")
    xcnt, _ = W.over([(k, km)], x, xm, "count")
    nlen, _ = W.over([(k, km)], None, None, "len")
    xmed, _ = W.over([(k, km)], x, xm, "quantile", q=0.5, interpolation="linear")
    out = df.select((c("x") / c("x").sum().over("k")).alias("share"), (c("x").sum() / pl.len()).over("k").alias("per_row"),
                    pl.when(c("x") > c("x").median().over("k")).then(c("x")).otherwise(c("x").median().over("k")).alias("w"), (c("x").sum().over("k") - c("x")).alias("rest"))
    plan = pl.last_plan()
    assert plan.count("Window{") == 1, plan                              # four windows over [k]: one bucket
    share, sok = cells(out["share"])
    per, pok = cells(out["per_row"])
    w, wok = cells(out["w"])
    assert sok.tolist() == xm.tolist() and pok.all()
    n_then = n_else = n_band = 0
    for r in range(n):
        scale = float(np.abs(x[(ids == ids[r]) & xm]).sum())
        # every x is positive, so the partition's sum s is within AE.RTOL * s of the exact sum (tests/agg_edges.py compare): x / s is within RTOL / (1 - RTOL) of
        # x / s_exact, plus the division's own rounding -- 2 RTOL covers both; s / len likewise within RTOL * s / len plus one rounding of the quotient
        if xm[r]:
            assert abs(share[r] - x[r] / xsum[r]) <= 2 * AE.RTOL * abs(x[r] / xsum[r]), r
        assert abs(per[r] - xsum[r] / nlen[r]) <= AE.RTOL * scale / nlen[r] + 2.0 ** -52 * abs(xsum[r] / nlen[r]), r
        part = x[(ids == ids[r]) & xm]
        assert wok[r] == (xmed[r] is not None), r
        if xmed[r] is not None:
            # the branch is decided by the reference alone: x above the median -> the row's own x, bit for bit; else (x null included) the median.  Only an x that
            # the device's median may lie on either side of -- x itself accepted as the median by tests/quantile_ref.py accept -- may take either branch
            is_x, is_med = bool(xm[r]) and w[r] == x[r], Q.accept(float(w[r]), part, 0.5, "linear")
            if xm[r] and Q.accept(float(x[r]), part, 0.5, "linear"):
                assert is_x or is_med, (r, w[r], x[r], xmed[r])
                n_band += 1
            elif xm[r] and x[r] > xmed[r]:
                assert is_x, (r, "then branch", w[r], x[r], xmed[r])
                n_then += 1
            else:
                assert is_med and not (xm[r] and is_x), (r, "otherwise branch", w[r], x[r], xmed[r])
                n_else += 1
    assert n_then > 100 and n_else > 100 and n_band < 50, (n_then, n_else, n_band)      # both branches are exercised; the band is the medians' own rows at most
    # filter(x > x.median().over(k)) against the reference mask; i is exact, so the kept rows and their order show
    kept = df.filter(c("i") > c("i").quantile(0.5, "lower").over("k"))
    imed, _ = W.over([(k, km)], i, None, "quantile", q=0.5, interpolation="lower")
    mask = np.array([i[r] > imed[r] for r in range(n)])
    assert kept.height == int(mask.sum()) and np.array_equal(kept["i"].to_numpy(), i[mask]) and "Window{" in pl.last_plan()
    assert "window expression: per-node route" in pl.last_plan(), pl.last_plan()          # the fused filter declined by name
    kept = df.filter(c("x") > c("x").median().over("k"))
    mask = np.array([bool(xm[r]) and xmed[r] is not None and x[r] > xmed[r] for r in range(n)])
    assert kept.height == int(mask.sum()) and np.array_equal(kept["i"].to_numpy(), i[mask])


def test_after_a_filter_after_a_join_lazy_and_no_fusion(pl, monkeypatch, table):
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (g, _), (i, _) = (table[nm] for nm in ("k", "g", "i"))
    keep = i > 0
    q = df.lazy().filter(c("i") > 0).with_columns(c("i").sum().over("k").alias("s"), pl.len().over("k").alias("cnt"))
    a = q.collect()
    b = q.collect(no_fusion=True)
    for out in (a, b):
        assert out.height == int(keep.sum())
        check(out["s"], [(k[keep], km[keep])], i[keep], None, "sum", "after filter")
        check(out["cnt"], [(k[keep], km[keep])], None, None, "len", "after filter")
    eager = df.filter(c("i") > 0).with_columns(c("i").sum().over("k").alias("s"), pl.len().over("k").alias("cnt"))
    assert eager.to_dict() == a.to_dict() == b.to_dict()
    # after a join: the right side's column as the key
    right = frame_of(pl, {"g": (np.arange(5, dtype=np.int64), None), "w": (np.array([3, 1, 3, 2, 1], np.int32), None)})
    out = df.lazy().join(right.lazy(), on="g", how="inner", maintain_order="left").with_columns(c("i").sum().over("w").alias("s")).collect()
    w = np.array([3, 1, 3, 2, 1], np.int32)[g]
    assert out.height == len(g) and np.array_equal(out["i"].to_numpy(), i)
    check(out["s"], [(w, None)], i, None, "sum", "after join")
    out = df.lazy().join(right.lazy(), on="g", how="inner", maintain_order="left").select(c("i"), c("i").max().over("w", "g").alias("m")).collect()
    check(out["m"], [(w, None), (g, None)], i, None, "max", "select over join")


def test_refusals(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    with pytest.raises(pl.UnsupportedError, match="window functions that do not aggregate"):
        df.select(c("x").over("k"))
    with pytest.raises(pl.UnsupportedError, match="window functions that do not aggregate"):
        df.select((c("x") - c("x").mean()).over("k"))
    with pytest.raises(pl.PlxError, match=r"window expression \(\.over\).*group_by"):
        df.lazy().group_by("g").agg(c("x").sum().over("k")).collect()
    with pytest.raises(pl.PlxError, match=r"window expression \(\.over\).*group_by"):
        df.lazy().group_by(c("i").sum().over("k")).agg(c("x").sum()).collect()
    with pytest.raises(pl.PlxError, match="a key that holds an aggregate"):
        df.select(c("x").sum().over(c("i").max()))
    with pytest.raises(ValueError, match="order_by"):
        c("x").sum().over("k", order_by="i")
    with pytest.raises(ValueError, match="mapping_strategy"):
        c("x").sum().over("k", mapping_strategy="join")


def test_example_query(pl, monkeypatch):
    from polars_amd import queries as QQ
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    rng = np.random.default_rng(35)
    n = 3000
    flag, status = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
    qty, price = rng.integers(1, 51, n).astype(np.int64), rng.uniform(900.0, 100000.0, n)
    df = frame_of(pl, {"l_returnflag": (flag, None), "l_linestatus": (status, None), "l_quantity": (qty, None), "l_extendedprice": (price, None)})
    out = QQ.share_of_flag_total(df.lazy()).collect()
    assert pl.last_plan().count("Window{") == 2, pl.last_plan()
    med, _ = W.over([(flag, None)], qty, None, "quantile", q=0.5, interpolation="linear")
    tot, _ = W.over([(flag, None), (status, None)], price, None, "sum")
    mask = np.array([qty[r] > med[r] for r in range(n)])
    assert out.height == int(mask.sum()) and np.array_equal(out["l_quantity"].to_numpy(), qty[mask])
    assert np.allclose(out["share"].to_numpy(), (price / np.array(tot))[mask], rtol=2 * AE.RTOL, atol=0)


# ---- the C entry and the plugin symbol ------------------------------------------------------------------------------------------------------------
def test_c_entry_and_plugin_symbol(pl, monkeypatch):
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    rng = np.random.default_rng(36)
    n = 130
    k, km = rng.integers(0, 9, n).astype(np.int32), rng.random(n) > 0.1
    x, xm = rng.normal(2.0, 1.0, n), rng.random(n) > 0.2
    i = rng.integers(-50, 50, n).astype(np.int64)
    ks, xs, isr = pl.Series("k", k, validity=km), pl.Series("x", x, validity=xm), pl.Series("i", i)
    keys, vals = (C.c_uint64 * 1)(ks._h), (C.c_uint64 * 4)(isr._h, xs._h, 0, xs._h)
    aggs = (C.c_int32 * 4)(F.AGG_SUM, F.AGG_STD, F.AGG_LEN, F.AGG_QUANTILE)
    ddof, q, ip = (C.c_int32 * 4)(1, 0, 1, 1), (C.c_double * 4)(0.5, 0.5, 0.5, 0.25), (C.c_int32 * 4)(4, 4, 4, F.QUANTILE_LOWER)
    out = (C.c_uint64 * 4)()
    F.check(F.lib().plx_window_agg(keys, 1, vals, aggs, 4, ddof, q, ip, out))
    plan = F.lib().plx_last_plan_description().decode()
    assert "Window{" in plan and DIRECT in plan and "aggs=4" in plan, plan
    cols = [pl.Series._from_handle(nm, out[j], dt) for j, (nm, dt) in enumerate((("s", pl.Int64), ("sd", pl.Float64), ("n", pl.UInt32), ("q", pl.Float64)))]
    check(cols[0], [(k, km)], i, None, "sum", "C sum")
    check(cols[1], [(k, km)], x, xm, "std", "C std", ddof=0)
    check(cols[2], [(k, km)], None, None, "len", "C len")
    check(cols[3], [(k, km)], x, xm, "quantile", "C quantile", q=0.25, interpolation="lower")
    monkeypatch.setenv("PLX_WINDOW_ROUTE", "sort")
    F.check(F.lib().plx_window_agg(keys, 1, vals, aggs, 1, None, None, None, out))          # NULL parameters: the defaults
    assert SORTED in F.lib().plx_last_plan_description().decode()
    check(pl.Series._from_handle("s", out[0], pl.Int64), [(k, km)], i, None, "sum", "C sum, sorted")
    nine = (C.c_uint64 * 9)(*([ks._h] * 9))
    assert F.lib().plx_window_agg(nine, 9, vals, aggs, 1, None, None, None, out) == F.ERR_UNSUPPORTED and "1..8 keys" in F.lib().plx_last_error().decode()
    monkeypatch.delenv("PLX_WINDOW_ROUTE", raising=False)
    # the plugin symbol: the value series, then the key series; kwargs name the aggregate
    arr_x, arr_k = pa.array(x, mask=~xm), pa.array(k, mask=~km)
    res, inp = P.call("plx_window_agg", [arr_x, arr_k], {"agg": "mean"}, names=["x", "k"])
    assert res is not None and inp.released == 2 and inp.out_name == b"x" and res.type == pa.float64() and len(res) == n, P.last_error()
    check(Host(res), [(k, km)], x, xm, "mean", "plugin mean")
    res, _ = P.call("plx_window_agg", [pa.array(i), arr_k, pa.array(i % 2)], {"agg": "quantile", "q": 0.25, "interpolation": "higher"})
    assert res is not None and res.type == pa.float64(), P.last_error()
    check(Host(res), [(k, km), (i % 2, None)], i, None, "quantile", "plugin quantile", q=0.25, interpolation="higher")
    res, _ = P.call("plx_window_agg", [pa.array(i), arr_k], {"agg": "var", "ddof": 0})
    assert res is not None, P.last_error()
    check(Host(res), [(k, km)], i, None, "var", "plugin var", ddof=0)
    res, _ = P.call("plx_window_agg", [arr_x, arr_k], {"agg": "median"})
    assert res is not None, P.last_error()
    check(Host(res), [(k, km)], x, xm, "quantile", "plugin median", q=0.5, interpolation="linear")
    # q is checked by name in the plugin, also where no row would reach the group-by that checks it; the C entry likewise
    for arrs in ([arr_x, arr_k], [arr_x.slice(0, 0), arr_k.slice(0, 0)]):
        for q in (1.5, "high"):
            res, inp = P.call("plx_window_agg", arrs, {"agg": "quantile", "q": q})
            assert res is None and inp.released == 2 and "plx_window_agg: kwargs q must be a real number in [0, 1]" in P.last_error(), (q, P.last_error())
    res, _ = P.call("plx_window_agg", [arr_x.slice(0, 0), arr_k.slice(0, 0)], {"agg": "quantile", "q": 0.5, "interpolation": "lower"})
    assert res is not None and len(res) == 0 and res.type == pa.float64(), P.last_error()
    empty = pl.Series("e", np.zeros(0, np.int64))
    assert F.lib().plx_window_agg((C.c_uint64 * 1)(empty._h), 1, (C.c_uint64 * 1)(empty._h), (C.c_int32 * 1)(F.AGG_QUANTILE), 1, None, (C.c_double * 1)(-0.5), None, out) == 1
    assert "window: quantile q" in F.lib().plx_last_error().decode()
    F.check(F.lib().plx_window_agg((C.c_uint64 * 1)(empty._h), 1, (C.c_uint64 * 1)(empty._h), (C.c_int32 * 1)(F.AGG_SUM), 1, None, None, None, out))
    assert "Window{keys=[1 columns], aggs=1, groups=0, rows=0, route=window[empty]}" in F.lib().plx_last_plan_description().decode()
    res, inp = P.call("plx_window_agg", [arr_x, arr_k], {"agg": "rank"})
    assert res is None and inp.released == 2 and "kwargs must carry agg" in P.last_error()
    res, inp = P.call("plx_window_agg", [arr_x], {"agg": "sum"})
    assert res is None and inp.released == 1 and "key series" in P.last_error()
