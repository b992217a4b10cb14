"""shift / diff on the device, plain and under `.over(keys)`, against tests/rolling_ref.py: every row in row order, the validity bitmap bit for bit.

n in 0, +-1, +-63, +-64, +-65, +-(rows - 1), +-rows, +-(rows + 5) at sizes around the wave, the workgroup and a 2048-row tile, with and without fill_value; Int8,
Int64, Float32, Boolean, Date and a Categorical column (its dictionary travels); every operand dtype of diff with its widened result dtype and integer wrap at the
type bounds; nullable keys and the segment patterns of the cumulative tests; the places an expression may stand; the C entry and the plugin symbols."""
import ctypes as C
import datetime as dt

import numpy as np
import pyarrow as pa
import pytest

from polars_amd import _ffi as F
from tests import plugin_abi as P
from tests import rolling_ref as R
from tests.test_gpu_cumulative import cells, contiguous_keys, frame_of

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5)
WHOLE, SORTED, EMPTY = "shift[whole column]", "shift[sorted rows:", "shift[empty]"


def shifts_for(rows):
    return sorted({0, 1, -1, 63, -63, 64, -64, 65, -65, rows - 1, -(rows - 1), rows, -rows, rows + 5, -(rows + 5)})


# ---- sizes and every n -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_whole_column_and_over(pl, n):
    rng = np.random.default_rng(4201 + n)
    x, xm = rng.normal(5.0, 2.0, n), rng.random(n) > 0.2
    i = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    k, km = rng.integers(-2, max(n // 5, 1) - 2, n).astype(np.int32), rng.random(n) > 0.1
    df = frame_of(pl, {"k": (k, km), "i": (i, None), "x": (x, xm)})
    c = pl.col
    picks = [s for s in shifts_for(n) if abs(s) in (0, 1, 64, n - 1, n, n + 5)] if n > 300 else shifts_for(n)
    for sh in picks:
        out = df.select(c("x").shift(sh).alias("s"), c("x").shift(sh, fill_value=-1.5).alias("sf"), c("i").shift(sh).alias("si"), c("x").diff(sh).alias("d"), c("i").diff(sh).alias("di"))
        plan = pl.last_plan()
        assert plan.count("Shift{") == 1 and "fns=5" in plan and (EMPTY if n == 0 else WHOLE) in plan and "keys=[]" in plan and f"rows={n}" in plan, plan
        R.check_shift(*cells(out["s"]), x, xm, sh, None, None, what=(n, sh, "s"))
        R.check_shift(*cells(out["sf"]), x, xm, sh, -1.5, None, what=(n, sh, "sf"))
        R.check_shift(*cells(out["si"]), i, None, sh, None, None, what=(n, sh, "si"))
        R.check_diff(*cells(out["d"]), x, xm, sh, None, what=(n, sh, "d"))
        R.check_diff(*cells(out["di"]), i, None, sh, None, what=(n, sh, "di"))
    for sh in (0, 1, -1, 3, -64, n + 5):
        out = df.select(c("x").shift(sh).over("k").alias("s"), c("i").shift(sh, fill_value=7).over("k").alias("sf"), c("x").diff(sh).over("k").alias("d"))
        plan = pl.last_plan()
        assert plan.count("Shift{") == 1 and "fns=3" in plan and (EMPTY if n == 0 else SORTED) in plan and "keys=[k]" in plan, plan
        R.check_shift(*cells(out["s"]), x, xm, sh, None, [(k, km)], what=(n, sh, "over s"))
        R.check_shift(*cells(out["sf"]), i, None, sh, 7, [(k, km)], what=(n, sh, "over sf"))
        R.check_diff(*cells(out["d"]), x, xm, sh, [(k, km)], what=(n, sh, "over d"))


def test_shift_zero_is_the_operand_and_a_null_free_result_has_no_bitmap(pl):
    x, xm = np.arange(200, dtype=np.float64), np.arange(200) % 3 != 0
    s = pl.Series("x", x, validity=xm)
    R.check_shift(*cells(s.shift(0)), x, xm, 0, None, None, what="shift(0)")
    v, ok = cells(pl.Series("y", x).shift(3, fill_value=0.5))
    assert ok is None or ok.all()
    R.check_shift(v, ok, x, None, 3, 0.5, None, what="filled")
    assert s.shift(0).name == "x" and s.shift(1).dtype == pl.Float64 and s.diff().name == "x"


# ---- the six column dtypes of shift, the bitmap bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("int8", "int64", "float32", "boolean", "date", "categorical"))
def test_shift_dtypes_with_and_without_fill(pl, kind):
    rng = np.random.default_rng(4202)
    rows = 2049
    ok = rng.random(rows) > 0.3
    k = rng.integers(0, 6, rows).astype(np.int32)
    cats = ["A", "N", "R"]
    x, dtype, fill, fill_phys = {
        "int8": (rng.integers(-128, 128, rows).astype(np.int8), None, -128, -128),
        "int64": (rng.integers(-(1 << 62), 1 << 62, rows, dtype=np.int64), None, (1 << 63) - 1, (1 << 63) - 1),
        "float32": (rng.normal(size=rows).astype(np.float32), None, 0.5, np.float32(0.5)),
        "boolean": (rng.random(rows) < 0.5, None, True, True),
        "date": (rng.integers(8000, 11000, rows).astype(np.int32), pl.Date, dt.date(1970, 1, 11), 10),
        "categorical": (rng.integers(0, 3, rows).astype(np.uint8), pl.Categorical(cats, pl.UInt8), "R", 2)}[kind]
    df = pl.DataFrame([pl.Series("k", k), pl.Series("x", x, dtype, validity=ok)])
    c = pl.col
    for sh in shifts_for(rows):
        out = df.select(c("x").shift(sh).alias("s"), c("x").shift(sh, fill_value=fill).alias("sf"))
        for name, f in (("s", None), ("sf", fill_phys)):
            assert out[name].dtype == df["x"].dtype, (kind, out[name].dtype)
            R.check_shift(*cells(out[name]), x, ok, sh, f, None, what=(kind, sh, name))
    for sh in (1, -1, 5, -400, 2049):
        out = df.select(c("x").shift(sh).over("k").alias("s"), c("x").shift(sh, fill_value=fill).over("k").alias("sf"))
        assert SORTED in pl.last_plan(), pl.last_plan()
        R.check_shift(*cells(out["s"]), x, ok, sh, None, [(k, None)], what=(kind, sh, "over"))
        R.check_shift(*cells(out["sf"]), x, ok, sh, fill_phys, [(k, None)], what=(kind, sh, "over filled"))
    s = df["x"].shift(2, fill_value=fill)                                  # the Series method, the same kernel
    assert s.dtype == df["x"].dtype and WHOLE in pl.last_plan(), pl.last_plan()
    R.check_shift(*cells(s), x, ok, 2, fill_phys, None, what=(kind, "series"))
    if kind == "categorical":                                              # the dictionary travels with the codes
        assert list(out["sf"].dtype.categories) == cats and list(s.dtype.categories) == cats
        want, want_ok = R.shift(x, ok, 2, 2, None)
        assert s.to_list() == [cats[v] if o else None for v, o in zip(want.tolist(), want_ok.tolist())]
        with pytest.raises(TypeError, match="cannot hold this fill_value exactly"):
            df.select(c("x").shift(1, fill_value="Z"))
    if kind == "int8":
        with pytest.raises(TypeError, match="cannot hold this fill_value exactly"):
            df["x"].shift(1, fill_value=128)


# ---- diff: every operand dtype, its result dtype, wrap at the bounds -----------------------------------------------------------------------------------------
DIFF_DTYPES = (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64)


@pytest.mark.parametrize("dtype", DIFF_DTYPES, ids=lambda d: np.dtype(d).name)
def test_diff_dtypes_and_values_at_the_bounds(pl, dtype):
    rng = np.random.default_rng(4203)
    rows = 2049
    d = np.dtype(dtype)
    if d.kind == "f":
        x = rng.normal(0.0, 1000.0, rows).astype(d)
        x[rng.random(rows) < 0.03] = np.inf
        x[rng.random(rows) < 0.03] = np.nan
        x[rng.random(rows) < 0.03] = -0.0
    else:
        info = np.iinfo(d)
        x = rng.integers(info.min, info.max, rows, dtype=d, endpoint=True)
        x[rng.random(rows) < 0.2] = info.max               # the bounds of the type: signed differences wrap, unsigned ones widen
        x[rng.random(rows) < 0.2] = info.min
    ok = rng.random(rows) > 0.1
    k = rng.integers(0, 9, rows).astype(np.int32)
    df = frame_of(pl, {"k": (k, None), "x": (x, ok)})
    c = pl.col
    for sh in (1, -1, 2, 64, -65, rows - 1, rows):
        out = df.select(c("x").diff(sh).alias("d"), c("x").diff(sh).over("k").alias("o"))
        v, vm = cells(out["d"])
        assert v.dtype == R.result_dtype("diff", d) and out["d"].dtype == pl.datatypes.NP_TO_DTYPE[R.result_dtype("diff", d)], (d, v.dtype, out["d"].dtype)
        R.check_diff(v, vm, x, ok, sh, None, what=(d.name, sh))
        R.check_diff(*cells(out["o"]), x, ok, sh, [(k, None)], what=(d.name, sh, "over"))
    s = pl.Series("x", x, validity=ok).diff(3)
    R.check_diff(*cells(s), x, ok, 3, None, what=(d.name, "series"))


def test_diff_refuses_what_has_no_difference(pl):
    c = pl.col
    d = pl.DataFrame([pl.Series("d", np.arange(5, dtype=np.int32), pl.Date), pl.Series("s", np.array([0, 1, 0, 1, 0], np.uint8), pl.Categorical(["a", "b"], pl.UInt8)),
                      pl.Series("b", np.array([True, False, True, True, False])), pl.Series("t", np.arange(5, dtype=np.int64), pl.Datetime)])
    for name in ("d", "s", "b", "t"):
        with pytest.raises(TypeError, match=r"diff\(\) needs"):
            d.select(c(name).diff())
        with pytest.raises(TypeError, match=r"diff\(\) needs"):
            d[name].diff()
    with pytest.raises(ValueError, match="null_behavior"):
        d.select(c("d").cast(pl.Int32).diff(1, "drop"))
    out = C.c_uint64()
    assert F.lib().plx_shift(None, 0, d["b"]._h, 1, None, 1, C.byref(out)) == F.ERR_UNSUPPORTED and "diff of a" in F.lib().plx_last_error().decode()


# ---- segment patterns, through .over -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ("one", "each", "three_tiles", "tile_first", "tile_last", "wave_edges", "random"))
def test_segment_patterns(pl, pattern):
    rng = np.random.default_rng(4204)
    n = 2 * 2048 + 5
    k = contiguous_keys(pattern, n, rng)
    x = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    xm = rng.random(n) > 0.15
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    c = pl.col
    for sh in (1, -1, 8, -504, 2048):
        out = df.select(c("x").shift(sh).over("k").alias("s"), c("x").shift(sh, fill_value=0).over("k").alias("sf"), c("x").diff(sh).over("k").alias("d"))
        assert SORTED in pl.last_plan() and pl.last_plan().count("Shift{") == 1, pl.last_plan()
        R.check_shift(*cells(out["s"]), x, xm, sh, None, [(k, None)], what=(pattern, sh))
        R.check_shift(*cells(out["sf"]), x, xm, sh, 0, [(k, None)], what=(pattern, sh, "filled"))
        R.check_diff(*cells(out["d"]), x, xm, sh, [(k, None)], what=(pattern, sh, "diff"))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_in_select_with_columns_filter_and_inside_expressions(pl):
    rng = np.random.default_rng(4205)
    n = 1000
    k, km = rng.integers(0, 40, n).astype(np.int32), rng.random(n) > 0.05
    g = rng.integers(0, 5, n).astype(np.int64)
    i = rng.integers(-500, 500, n).astype(np.int64)
    df = frame_of(pl, {"k": (k, km), "g": (g, None), "i": (i, None)})
    c = pl.col
    out = df.with_columns((c("i") * c("g")).shift(2).over("k").alias("prev"), c("i").diff().alias("d"), c("i").shift(-1, fill_value=0).over("g", "k").alias("next"))
    plan = pl.last_plan()
    assert out.columns == ["k", "g", "i", "prev", "d", "next"] and out.height == n and plan.count("Shift{") == 3, plan
    assert "keys=[k]" in plan and "keys=[g, k]" in plan and "keys=[]" in plan and WHOLE in plan and SORTED in plan, plan
    R.check_shift(*cells(out["prev"]), i * g, None, 2, None, [(k, km)], what="operand expression")
    R.check_diff(*cells(out["d"]), i, None, 1, None, what="d")
    R.check_shift(*cells(out["next"]), i, None, -1, 0, [(g, None), (k, km)], what="next")
    # x - x.shift(1).over(k) is x.diff().over(k); twins are computed once; when / then / otherwise around them
    out = df.select((c("i") - c("i").shift(1).over("k")).alias("a"), c("i").diff().over("k").alias("b"), c("i").shift(1).over("k").alias("p"),
                    pl.when(c("i").shift(1, fill_value=0).over("k") > 0).then(c("i")).otherwise(c("i").shift(-1, fill_value=0).over("k")).alias("w"))
    plan = pl.last_plan()
    assert plan.count("Shift{") == 1 and "fns=5" in plan, plan
    a, am = cells(out["a"])
    b, bm = cells(out["b"])
    assert np.array_equal(am, bm) and np.array_equal(a[am], b[bm])
    prev, _ = R.shift(i, None, 1, 0, [(k, km)])
    nxt, _ = R.shift(i, None, -1, 0, [(k, km)])
    assert np.array_equal(out["w"].to_numpy(), np.where(prev > 0, i, nxt))
    # as a filter predicate: rows whose value rose against the row of their partition before them (a null predicate row is dropped)
    kept = df.filter(c("i").diff().over("k") > 0)
    assert "Shift{" in pl.last_plan() and "shift / diff / rolling expression: per-node route" in pl.last_plan(), pl.last_plan()
    dv, dm = R.diff(i, None, 1, [(k, km)])
    assert np.array_equal(kept["i"].to_numpy(), i[dm & (dv > 0)])
    keep = i > 0
    q = df.lazy().filter(c("i") > 0).with_columns(c("i").shift(1).over("k").alias("s"))
    for res in (q.collect(), q.collect(no_fusion=True)):
        R.check_shift(*cells(res["s"]), i[keep], None, 1, None, [(k[keep], km[keep])], what="after filter")
    out = df.filter(c("i") > 10_000).select(c("i").shift(1).over("k").alias("s"), c("g").cast(pl.UInt8).diff().alias("w"))
    assert out.height == 0 and (out["s"].dtype, out["w"].dtype) == (pl.Int64, pl.Int16) and EMPTY in pl.last_plan(), pl.last_plan()
    with pytest.raises(TypeError, match="group_by"):
        df.lazy().group_by("g").agg(c("i").shift()).collect()
    with pytest.raises(TypeError, match="inside the operand of another one"):
        df.select(c("i").shift().diff())
    with pytest.raises(TypeError, match="mixes a cumulative / ranking expression"):
        df.select((c("i") - c("i").shift()).over("k"))


def test_example_query(pl):
    from polars_amd import queries as QQ
    rng = np.random.default_rng(4206)
    n = 3000
    flag = rng.integers(0, 3, n).astype(np.uint8)
    qty = rng.integers(1, 51, n).astype(np.float64)
    df = frame_of(pl, {"l_returnflag": (flag, None), "l_quantity": (qty, None)})
    out = QQ.quantity_change_by_flag(df.lazy()).collect()
    assert pl.last_plan().count("Shift{") == 1 and "fns=2" in pl.last_plan() and SORTED in pl.last_plan(), pl.last_plan()
    R.check_diff(*cells(out["quantity_change"]), qty, None, 1, [(flag, None)], what="change")
    R.check_shift(*cells(out["previous_quantity"]), qty, None, 1, None, [(flag, None)], what="previous")


# ---- the C entry and the plugin symbols ----------------------------------------------------------------------------------------------------------------------
def test_c_entry_and_plugin_symbols(pl):
    rng = np.random.default_rng(4207)
    n = 2100
    k, km = rng.integers(0, 9, n).astype(np.int32), rng.random(n) > 0.1
    x, xm = rng.normal(2.0, 1.0, n), rng.random(n) > 0.2
    u = rng.integers(0, 256, n).astype(np.uint8)
    ks, xs, us = pl.Series("k", k, validity=km), pl.Series("x", x, validity=xm), pl.Series("u", u)
    out = C.c_uint64()
    fill = F.Scalar()
    fill.f64 = -2.5
    F.check(F.lib().plx_shift((C.c_uint64 * 1)(ks._h), 1, xs._h, -3, C.byref(fill), 0, C.byref(out)))
    plan = F.lib().plx_last_plan_description().decode()
    assert "Shift{keys=[1 columns], fns=1" in plan and SORTED in plan and "n=-3" in plan, plan
    R.check_shift(*cells(pl.Series._from_handle("s", out.value, pl.Float64)), x, xm, -3, -2.5, [(k, km)], what="C over, filled")
    F.check(F.lib().plx_shift(None, 0, us._h, 2, None, 1, C.byref(out)))
    assert WHOLE in F.lib().plx_last_plan_description().decode() and "diff" in F.lib().plx_last_plan_description().decode()
    R.check_diff(*cells(pl.Series._from_handle("d", out.value, pl.Int16)), u, None, 2, None, what="C whole diff")
    F.check(F.lib().plx_shift(None, 0, xs._h, -(1 << 63), None, 0, C.byref(out)))              # any int64: every row vacated
    assert cells(pl.Series._from_handle("v", out.value, pl.Float64))[1].sum() == 0
    # parameters are refused by name before anything runs, an empty input included
    empty = pl.Series("e", np.zeros(0, np.int64))
    err = lambda: F.lib().plx_last_error().decode()
    for col in (xs, empty):
        assert F.lib().plx_shift(None, 0, col._h, 1, None, 2, C.byref(out)) == 1 and "diff must be 0 or 1" in err()
        assert F.lib().plx_shift(None, 0, col._h, 1, C.byref(fill), 1, C.byref(out)) == 1 and "fill must be NULL" in err()
        assert F.lib().plx_shift(None, 3, col._h, 1, None, 0, C.byref(out)) == 1 and "n_keys" in err()
    F.check(F.lib().plx_shift(None, 0, empty._h, 1, None, 0, C.byref(out)))
    e = pl.Series._from_handle("n", out.value, pl.Int64)
    assert len(e) == 0 and EMPTY in F.lib().plx_last_plan_description().decode()
    nine = (C.c_uint64 * 9)(*([ks._h] * 9))
    assert F.lib().plx_shift(nine, 9, xs._h, 1, None, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in err()
    # the plugin symbols: the value series, then the key series
    arr_x, arr_k = pa.array(x, mask=~xm), pa.array(k, mask=~km)
    res, inp = P.call("plx_shift", [arr_x, arr_k], {"n": -2}, names=["x", "k"])
    assert res is not None and inp.released == 2 and inp.out_name == b"x" and res.type == pa.float64() and len(res) == n, P.last_error()
    R.check_shift(np.asarray(res.fill_null(0.0)), ~np.asarray(res.is_null()), x, xm, -2, None, [(k, km)], what="plugin shift over")
    res, _ = P.call("plx_shift", [pa.array(u)], {})
    assert res is not None and res.type == pa.uint8(), P.last_error()
    R.check_shift(np.asarray(res.fill_null(0)), ~np.asarray(res.is_null()), u, None, 1, None, None, what="plugin shift, n absent")
    res, _ = P.call("plx_diff", [pa.array(u), arr_k], {"n": 3})
    assert res is not None and res.type == pa.int16(), P.last_error()
    R.check_diff(np.asarray(res.fill_null(0)), ~np.asarray(res.is_null()), u, None, 3, [(k, km)], what="plugin diff over")
    for arrs in ([arr_x, arr_k], [arr_x.slice(0, 0), arr_k.slice(0, 0)]):
        for sym in ("plx_shift", "plx_diff"):
            res, inp = P.call(sym, arrs, {"n": "two"})
            assert res is None and inp.released == 2 and "kwargs n must be an integer" in P.last_error(), P.last_error()
