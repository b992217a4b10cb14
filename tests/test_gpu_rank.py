"""rank on the device, plain and under `.over(keys)`, against tests/cumulative_ref.py: every row in row order, validity bit for bit, every rank exact.

The five methods, ascending and descending, with ties in every one of them; the sizes around the word (64), the workgroup (256) and the tile (2048); the segment
patterns of the partitioned form; nulls (a null row's rank is null and takes no part), NaN (greatest, all NaNs tie) and signed zeros (-0 == +0); the operand dtypes;
the key dtypes and their edges; the places an expression may stand (the top-3 filter among them); the plan text; the C entry and the plugin symbol."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from polars_amd import _ffi as F
from tests import cumulative_ref as R
from tests import plugin_abi as P
from tests.test_gpu_cumulative import BIG, PATTERNS, SIZES, cells, contiguous_keys, frame_of

pytestmark = pytest.mark.gpu

ROUTE, EMPTY = "rank[sorted segments:", "rank[empty]"


def all_ranks(c, over=None):
    """the ten (method, descending) forms of one operand"""
    out = []
    for m in R.METHODS:
        for desc in (False, True):
            e = c.rank(m, descending=desc)
            out.append((e.over(over) if over else e).alias(f"{m}_{int(desc)}"))
    return out


def check_all(out, x, xm, keys, what):
    for m in R.METHODS:
        for desc in (False, True):
            R.check_rank(*cells(out[f"{m}_{int(desc)}"]), x, xm, m, desc, keys, what=(what, m, desc))


@pytest.mark.parametrize("n", SIZES)
def test_sizes_whole_column_and_over(pl, n):
    rng = np.random.default_rng(4190 + n)
    x, xm = rng.integers(0, max(n // 3, 2), n).astype(np.int64), rng.random(n) > 0.2          # about three rows a value: ties in every method
    k, km = rng.integers(-2, max(n // 20, 1) - 2, n).astype(np.int32), rng.random(n) > 0.1
    df = frame_of(pl, {"k": (k, km), "x": (x, xm)})
    c = pl.col
    out = df.select(*all_ranks(c("x")))
    plan = pl.last_plan()
    # the ten forms share two sorts: one per direction
    assert plan.count("Rank{") == (1 if n == 0 else 2) and "keys=[]" in plan and (EMPTY if n == 0 else ROUTE) in plan, plan
    if n:
        assert "fns=5" in plan and "method=average+min+max+dense+ordinal" in plan and "descending" in plan and f"rows={n}" in plan, plan
    check_all(out, x, xm, None, (n, "whole"))
    out = df.select(*all_ranks(c("x"), "k"))
    plan = pl.last_plan()
    assert plan.count("Rank{") == (1 if n == 0 else 2) and "keys=[k]" in plan, plan
    check_all(out, x, xm, [(k, km)], (n, "over"))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_segment_patterns(pl, pattern):
    rng = np.random.default_rng(4191)
    n = 2 * 2048 + 5
    k = contiguous_keys(pattern, n, rng)
    x, xm = rng.integers(-5, 5, n).astype(np.int32), rng.random(n) > 0.15
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    out = df.select(*all_ranks(pl.col("x"), "k"))
    check_all(out, x, xm, [(k, None)], pattern)


def test_a_large_column(pl):
    """2048 * 2048 + 3 rows: positions, starts and ranks well past 2^16 and 2^22; random partitions of 1..300 rows and the whole column"""
    rng = np.random.default_rng(4192)
    k = contiguous_keys("random", BIG, rng)
    x, xm = rng.integers(0, 1000, BIG).astype(np.int32), rng.random(BIG) > 0.1
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    c = pl.col
    out = df.select(c("x").rank("ordinal", descending=True).over("k").alias("o"), c("x").rank("dense").over("k").alias("d"), c("x").rank("min").alias("w"))
    R.check_rank(*cells(out["o"]), x, xm, "ordinal", True, [(k, None)], what="big ordinal")
    R.check_rank(*cells(out["d"]), x, xm, "dense", False, [(k, None)], what="big dense")
    R.check_rank(*cells(out["w"]), x, xm, "min", False, None, what="big whole")


@pytest.mark.parametrize("dtype", (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_),
                         ids=lambda d: np.dtype(d).name)
def test_operand_dtypes_nan_zeros_and_nulls(pl, dtype):
    rng = np.random.default_rng(4193)
    n = 777
    dt = np.dtype(dtype)
    if dt.kind == "b":
        x = rng.random(n) < 0.5
    elif dt.kind == "f":
        x = rng.integers(-3, 4, n).astype(dt)
        x[rng.random(n) < 0.15] = np.nan                   # NaN is greatest, all NaNs tie
        x[rng.random(n) < 0.1] = -0.0                      # -0 == +0: one run of ties
        x[rng.random(n) < 0.05] = np.inf
        x[rng.random(n) < 0.05] = -np.inf
    else:
        info = np.iinfo(dt)
        x = np.array([info.min, info.max, 0, 1, info.max - 1], dt)[rng.integers(0, 5, n)]
    xm = rng.random(n) > 0.2
    k = rng.integers(0, 6, n).astype(np.int32)
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    c = pl.col
    out = df.select(*all_ranks(c("x")))
    for m in R.METHODS:
        assert out[f"{m}_0"].dtype == (pl.Float64 if m == "average" else pl.UInt32), m
    check_all(out, x, xm, None, (dt.name, "whole"))
    check_all(df.select(*all_ranks(c("x"), "k")), x, xm, [(k, None)], (dt.name, "over"))
    # every row null: every rank null; no nulls at all
    check_all(frame_of(pl, {"x": (x, np.zeros(n, bool))}).select(*all_ranks(c("x"))), x, np.zeros(n, bool), None, (dt.name, "all null"))
    check_all(frame_of(pl, {"x": (x, None)}).select(*all_ranks(c("x"))), x, None, None, (dt.name, "no nulls"))


def test_key_dtypes_and_key_edges(pl):
    rng = np.random.default_rng(4194)
    n = 700
    x, xm = rng.integers(-9, 9, n).astype(np.int64), rng.random(n) > 0.1
    f = rng.integers(0, 4, n).astype(np.float64)
    f[rng.random(n) < 0.2] = np.nan
    f[rng.random(n) < 0.1] = -0.0
    keys = {"i8": (rng.integers(-3, 3, n).astype(np.int8), rng.random(n) > 0.2), "u64": (rng.integers(0, 1 << 64, 5, dtype=np.uint64)[rng.integers(0, 5, n)], None),
            "i64": (np.array([-(1 << 63), (1 << 63) - 1, 0, -1], np.int64)[rng.integers(0, 4, n)], None),
            "f64": (f, rng.random(n) > 0.1), "b": (rng.random(n) < 0.5, rng.random(n) > 0.2)}
    df = frame_of(pl, dict(keys, x=(x, xm)))
    c = pl.col
    for name, (kv, km) in keys.items():
        out = df.select(c("x").rank("min").over(name).alias("a"), c("x").rank("ordinal", descending=True).over(name).alias("b"))
        assert ROUTE in pl.last_plan() and f"keys=[{name}]" in pl.last_plan() and pl.last_plan().count("Rank{") == 2, pl.last_plan()
        R.check_rank(*cells(out["a"]), x, xm, "min", False, [(kv, km)], what=name)
        R.check_rank(*cells(out["b"]), x, xm, "ordinal", True, [(kv, km)], what=name)
    out = df.select(c("x").rank("dense").over("i8", "f64", "b").alias("d"))
    R.check_rank(*cells(out["d"]), x, xm, "dense", False, [keys["i8"], keys["f64"], keys["b"]], what="three keys")
    with pytest.raises(pl.UnsupportedError, match="1..8"):
        df.select(c("x").rank().over(*["i8"] * 9))


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(4195)
    n = 1000
    return {"k": (rng.integers(0, 40, n).astype(np.int32), rng.random(n) > 0.05), "g": (rng.integers(0, 5, n).astype(np.int64), None),
            "x": (rng.integers(-50, 50, n).astype(np.float64), rng.random(n) > 0.1), "i": (rng.integers(-500, 500, n).astype(np.int64), None)}


def test_shapes_top3_filter_when_then_lazy_and_no_fusion(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    (k, km), (g, _), (x, xm), (i, _) = (table[nm] for nm in ("k", "g", "x", "i"))
    n = len(k)
    # top-3 per partition as a filter predicate: the ordinal ranks are distinct, so exactly min(3, valid rows) rows of every partition stay, in row order
    r, rok = R.rank(i, None, "ordinal", True, [(k, km)])
    q = df.lazy().filter(c("i").rank("ordinal", descending=True).over("k") <= 3)
    a, b = q.collect(), q.collect(no_fusion=True)
    assert "Rank{" in pl.last_plan() and ROUTE in pl.last_plan(), pl.last_plan()
    assert a.to_dict() == b.to_dict() == df.filter(c("i").rank("ordinal", descending=True).over("k") <= 3).to_dict()
    assert a.height == int((r <= 3).sum()) and np.array_equal(a["i"].to_numpy(), i[r <= 3])
    df.lazy().filter(c("i").rank("ordinal", descending=True).over("k") <= 3).collect()
    assert "cumulative / ranking expression: per-node route" in pl.last_plan(), pl.last_plan()
    # with_columns, arithmetic and when/then around ranks; a null rank makes the comparison null, which when() treats as false
    out = df.with_columns(c("x").rank("dense").over("g").alias("d"), (c("x").rank("max") - c("x").rank("min")).alias("span"),
                          pl.when(c("x").rank("min").over("g") == 1).then(c("i")).otherwise(pl.lit(0)).alias("w"), (c("i") * c("g")).rank("average").alias("avg"))
    assert out.columns == ["k", "g", "x", "i", "d", "span", "w", "avg"] and out.height == n
    R.check_rank(*cells(out["d"]), x, xm, "dense", False, [(g, None)], what="d")
    R.check_rank(*cells(out["avg"]), i * g, None, "average", False, None, what="operand expression")
    mx, _ = R.rank(x, xm, "max")
    mn, _ = R.rank(x, xm, "min")
    span, sok = cells(out["span"])
    assert np.array_equal(sok, xm) and np.array_equal(span[xm], (mx - mn)[xm])
    first, _ = R.rank(x, xm, "min", False, [(g, None)])
    assert np.array_equal(out["w"].to_numpy(), np.where(xm & (first == 1), i, 0))
    # after a filter and after a join
    keep = i > 0
    out = df.lazy().filter(c("i") > 0).with_columns(c("x").rank("ordinal").over("k").alias("r")).collect()
    R.check_rank(*cells(out["r"]), x[keep], xm[keep], "ordinal", False, [(k[keep], km[keep])], what="after filter")
    right = frame_of(pl, {"g": (np.arange(5, dtype=np.int64), None), "w": (np.array([3, 1, 3, 2, 1], np.int32), None)})
    out = df.lazy().join(right.lazy(), on="g", how="inner", maintain_order="left").select(c("i"), c("x").rank("min", descending=True).over("w").alias("r")).collect()
    w = np.array([3, 1, 3, 2, 1], np.int32)[g]
    assert np.array_equal(out["i"].to_numpy(), i)
    R.check_rank(*cells(out["r"]), x, xm, "min", True, [(w, None)], what="after join")
    # ranks and cumulative functions over the same keys in one node; an empty frame
    out = df.select(c("i").cum_sum().over("k").alias("s"), c("i").rank("dense").over("k").alias("r"))
    assert "Cumulative{keys=[k]" in pl.last_plan() and "Rank{keys=[k]" in pl.last_plan(), pl.last_plan()
    out = df.filter(c("i") > 10_000).select(c("x").rank().alias("a"), c("x").rank("ordinal").over("k").alias("o"))
    assert out.height == 0 and (out["a"].dtype, out["o"].dtype) == (pl.Float64, pl.UInt32) and EMPTY in pl.last_plan(), pl.last_plan()
    # two runs of the same input: the same bits
    e = [c("x").rank("average").over("k").alias("a"), c("x").rank("ordinal", descending=True).alias("o")]
    u, v = df.select(*e), df.select(*e)
    assert u.to_dict() == v.to_dict()


def test_refusals(pl, table):
    df = frame_of(pl, table)
    c = pl.col
    for bad in ("random", "first", None, 3):
        with pytest.raises(ValueError, match=r"average.*min.*max.*dense.*ordinal"):
            c("x").rank(bad)
    with pytest.raises(TypeError, match="descending"):
        c("x").rank("min", descending="yes")
    with pytest.raises(TypeError, match="group_by"):
        df.lazy().group_by("g").agg(c("x").rank()).collect()
    with pytest.raises(TypeError, match="an aggregate"):
        df.select(c("x").max().rank())
    with pytest.raises(TypeError, match="inside the operand of another one"):
        df.select(c("x").rank().cum_sum())
    with pytest.raises(TypeError, match="mixes a cumulative / ranking expression"):
        df.select((c("x").rank() / pl.len()).over("k"))
    d = pl.DataFrame([pl.Series("d", np.array([3, 1, 2, 1, 5], np.int32), pl.Date), pl.Series("s", np.array([0, 1, 0, 1, 0], np.uint8), pl.Categorical(["a", "b"], pl.UInt8))])
    with pytest.raises(TypeError, match="rank"):
        d.select(c("s").rank())
    out = d.select(c("d").rank("min").alias("r"))          # Date / Datetime operands are ranked as their days / ticks
    assert out["r"].dtype == pl.UInt32 and out["r"].to_numpy().tolist() == [4, 1, 3, 1, 5]


def test_example_query(pl):
    from polars_amd import queries as QQ
    rng = np.random.default_rng(4196)
    n = 3000
    flag, status = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
    price = rng.uniform(900.0, 100000.0, n)
    price[rng.integers(0, n, 50)] = 50000.0                       # ties among the candidates: ordinal ranks still keep exactly three rows
    df = frame_of(pl, {"l_returnflag": (flag, None), "l_linestatus": (status, None), "l_extendedprice": (price, None), "l_orderkey": (np.arange(n, dtype=np.int64), None)})
    out = QQ.top3_price_per_flag(df.lazy()).collect()
    assert "Rank{" in pl.last_plan() and "method=ordinal, descending" in pl.last_plan(), pl.last_plan()
    r, _ = R.rank(price, None, "ordinal", True, [(flag, None), (status, None)])
    assert out.height == 18 and np.array_equal(out["l_orderkey"].to_numpy(), np.flatnonzero(r <= 3))


def test_series_c_entry_and_plugin_symbol(pl):
    rng = np.random.default_rng(4197)
    n = 2100
    k, km = rng.integers(0, 9, n).astype(np.int32), rng.random(n) > 0.1
    x, xm = rng.integers(0, 40, n).astype(np.float64), rng.random(n) > 0.2
    ks, xs = pl.Series("k", k, validity=km), pl.Series("x", x, validity=xm)
    for m in R.METHODS:
        s = xs.rank(m, descending=True)
        assert s.dtype == (pl.Float64 if m == "average" else pl.UInt32) and s.name == "x" and ROUTE in pl.last_plan()
        R.check_rank(*cells(s), x, xm, m, True, None, what=("Series", m))
    out = C.c_uint64()
    F.check(F.lib().plx_rank((C.c_uint64 * 1)(ks._h), 1, xs._h, F.RANK_DENSE, 0, C.byref(out)))
    plan = F.lib().plx_last_plan_description().decode()
    assert "Rank{keys=[1 columns], fns=1" in plan and "method=dense" in plan and ROUTE in plan, plan
    R.check_rank(*cells(pl.Series._from_handle("r", out.value, pl.UInt32)), x, xm, "dense", False, [(k, km)], what="C over")
    empty = pl.Series("e", np.zeros(0, np.int64))
    for col in (xs, empty):
        assert F.lib().plx_rank(None, 0, col._h, 5, 0, C.byref(out)) == 1 and "no plx_rank_method" in F.lib().plx_last_error().decode()
        assert F.lib().plx_rank(None, 0, col._h, F.RANK_MIN, -1, C.byref(out)) == 1 and "descending must be 0 or 1" in F.lib().plx_last_error().decode()
    F.check(F.lib().plx_rank(None, 0, empty._h, F.RANK_AVERAGE, 1, C.byref(out)))
    e = pl.Series._from_handle("r", out.value, pl.Float64)
    assert len(e) == 0 and EMPTY in F.lib().plx_last_plan_description().decode()
    nine = (C.c_uint64 * 9)(*([ks._h] * 9))
    assert F.lib().plx_rank(nine, 9, xs._h, F.RANK_MIN, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in F.lib().plx_last_error().decode()
    arr_x, arr_k = pa.array(x, mask=~xm), pa.array(k, mask=~km)
    res, inp = P.call("plx_rank", [arr_x, arr_k], {"method": "average", "descending": True}, names=["x", "k"])
    assert res is not None and inp.released == 2 and inp.out_name == b"x" and res.type == pa.float64() and len(res) == n, P.last_error()
    R.check_rank(np.asarray(res.fill_null(0.0)), ~np.asarray(res.is_null()), x, xm, "average", True, [(k, km)], what="plugin over")
    res, _ = P.call("plx_rank", [arr_x], {"method": "ordinal"})
    assert res is not None and res.type == pa.uint32(), P.last_error()
    R.check_rank(np.asarray(res.fill_null(0)), ~np.asarray(res.is_null()), x, xm, "ordinal", False, None, what="plugin whole")
    for arrs in ([arr_x, arr_k], [arr_x.slice(0, 0), arr_k.slice(0, 0)]):
        res, inp = P.call("plx_rank", arrs, {"method": "random"})
        assert res is None and inp.released == 2 and "kwargs must carry method in {average, min, max, dense, ordinal}" in P.last_error(), P.last_error()
