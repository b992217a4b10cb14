"""shift / diff and the rolling functions without a GPU: the arithmetic of csrc/rolling.hpp as a stand-alone program under -fsanitize=address,undefined against a
direct loop (both routes, lane by lane); the numpy reference's own check and its cross-check against pandas; the validators and reprs; the lowering to
PLX_AE_SHIFT = 18 / PLX_AE_ROLLING = 19 with the packed literal; the header's numbering, plx_aexpr's size and the prototypes through a compiled C caller; every
refusal by message; explain(); no predicate or slice pushed through; the fused compiler declining by name; the visitor's function nodes through the engine shim;
the plugin fields; the example queries; the kernels' registers and LDS."""
import ctypes as C
import datetime as dt
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import rolling_ref as R
from tests.test_program_eval_cpu import frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
REASON = "shift / diff / rolling expression: per-node route"
LDS_BUDGET = 64 * 1024          # static LDS of the tile route stays at or below 64 KiB, so two workgroups fit a CU's 160 KiB


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_under_sanitizers_against_a_direct_loop(tmp_path):
    """tests/emu/rolling_main.cpp: the tile-halo route (region, forward and backward scan, LDS slots at their exact size, combine) and the two-scan route (tile
    aggregates, their chunked scan, tiles with carry, mirrored) lane by lane over the sizes, windows, segment and validity patterns of the GPU tests; the shifted
    bitmap at every bit offset."""
    exe = str(tmp_path / "rolling_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "rolling_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 10_000_000, r.stdout


def test_the_reference():
    assert R.self_check() == 22
    x = np.array([1.5, 2.5, -1.0, 4.0], np.float32)
    R.check_rolling(np.array([0, 4.0, 1.5, 3.0], np.float32), np.array([0, 1, 1, 1], bool), "rolling_sum", x, None, 2)
    with pytest.raises(AssertionError):
        R.check_rolling(np.array([0, 4.0, 1.5, 3.5], np.float32), np.array([0, 1, 1, 1], bool), "rolling_sum", x, None, 2)
    with pytest.raises(AssertionError):                                   # the result dtype is part of the check
        R.check_rolling(np.array([0, 4.0, 1.5, 3.0]), np.array([0, 1, 1, 1], bool), "rolling_sum", x, None, 2)
    with pytest.raises(AssertionError):                                   # ... and so is every validity bit
        R.check_rolling(np.array([0, 4.0, 1.5, 3.0], np.float32), np.array([1, 1, 1, 1], bool), "rolling_sum", x, None, 2)
    R.check_rolling(np.array([0, 2.0, 0.75, 1.5], np.float32), np.array([0, 1, 1, 1], bool), "rolling_mean", x, None, 2)
    R.check_shift(np.array([0, 1.5, 2.5, -1.0], np.float32), np.array([0, 1, 1, 1], bool), x, None, 1)
    R.check_diff(np.array([0, 1.0, -3.5, 5.0], np.float32), np.array([0, 1, 1, 1], bool), x, None, 1)
    with pytest.raises(AssertionError):
        R.check_diff(np.array([0, 1.0, -3.5, 5.5], np.float32), np.array([0, 1, 1, 1], bool), x, None, 1)


def test_the_reference_against_pandas():
    """NaN-free data, nulls as NaN: pandas rolling(w, min_periods=m, center=c), shift and diff, whole column and per group"""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(419)
    n = 400
    x, ok = rng.integers(-50, 50, n).astype(np.float64), rng.random(n) > 0.2
    k = rng.integers(0, 7, n)
    s = pd.Series(np.where(ok, x, np.nan))
    for keys, g in ((None, None), ([(k, None)], pd.Series(k))):
        for w in (1, 2, 3, 7, 64, 500):
            for center in (False, True):
                if center and w % 2 == 0:
                    continue                        # (pandas centers an even window half a row to the other side: offset w // 2 where this contract has (w - 1) // 2)
                for m in sorted({1, w, (w + 1) // 2}):
                    for op, fn in (("rolling_sum", "sum"), ("rolling_mean", "mean"), ("rolling_min", "min"), ("rolling_max", "max")):
                        want = getattr(s.rolling(w, min_periods=m, center=center) if g is None else s.groupby(g).rolling(w, min_periods=m, center=center), fn)()
                        want = want.to_numpy() if g is None else want.reset_index(level=0, drop=True).sort_index().to_numpy()
                        got, got_ok, _, _ = R.rolling(op, x, ok, w, m, center, keys)
                        assert np.array_equal(got_ok, ~np.isnan(want)), (op, w, m, center, g is None)
                        assert np.allclose(got[got_ok], want[got_ok], rtol=1e-12, atol=1e-9), (op, w, m, center)
        for sh in (0, 1, -1, 5, -63, n - 1, n, n + 5):
            want = (s.shift(sh) if g is None else s.groupby(g).shift(sh)).to_numpy()
            got, got_ok = R.shift(x, ok, sh, None, keys)
            assert np.array_equal(got_ok, ~np.isnan(want)) and np.array_equal(got[got_ok], want[got_ok]), sh
            if sh:
                want = (s.diff(sh) if g is None else s.groupby(g).diff(sh)).to_numpy()
                got, got_ok = R.diff(x, ok, sh, keys)
                assert np.array_equal(got_ok, ~np.isnan(want)) and np.array_equal(got[got_ok], want[got_ok]), sh


# ---- the mirror API ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def df():
    rng = np.random.default_rng(419)
    n = 301
    cols = {"k": (rng.integers(0, 7, n).astype(np.int64), None), "k2": (rng.integers(0, 3, n).astype(np.int32), rng.random(n) < 0.9), "x": (rng.normal(3.0, 2.0, n), None),
            "a": (rng.integers(-300, 300, n).astype(np.int8), None), "f": (rng.normal(size=n).astype(np.float32), None), "flag": (rng.random(n) < 0.5, None),
            "d": (rng.integers(8000, 11000, n).astype(np.int32), None), "s": (rng.integers(0, 3, n).astype(np.uint8), None), "u": (rng.integers(0, 9, n).astype(np.uint32), None),
            "u8": (rng.integers(0, 200, n).astype(np.uint8), None), "u16": (rng.integers(0, 9, n).astype(np.uint16), None), "u64": (rng.integers(0, 9, n).astype(np.uint64), None),
            "t": (rng.integers(0, 10 ** 15, n).astype(np.int64), None)}
    return frame_like(cols, {"d": pl.Date, "s": pl.Categorical(["A", "N", "R"], pl.UInt8), "f": pl.Float32, "t": pl.Datetime})


def test_validators_and_reprs():
    e = c("x").shift()
    assert (e.kind, e.op, e.value) == ("shift", F.SHIFT_SHIFT, (1, None)) and repr(e) == "col('x').shift(1)"
    assert repr(c("x").shift(-3, fill_value=0.5)) == "col('x').shift(-3, fill_value=0.5)" and repr(c("x").diff(2)) == "col('x').diff(2)"
    assert c("x").shift(np.int64(-7)).value == (-7, None) and c("x").shift(2 ** 70).value[0] == 2 ** 70 and c("x").diff(np.uint8(3)).value == (3, None)
    assert c("x").shift(1, fill_value=pl.lit(3)).value == (1, 3)                                   # a plain literal expression is its value
    for fn in (c("x").shift, c("x").diff):
        for bad in (True, 1.0, None, "1", np.bool_(False)):
            with pytest.raises(TypeError, match="n="):
                fn(bad)
    with pytest.raises(TypeError, match="an expression as fill_value"):
        c("x").shift(1, fill_value=c("a"))
    with pytest.raises(TypeError, match="an expression as fill_value"):
        c("x").shift(1, fill_value=pl.lit(1) + 1)
    with pytest.raises(ValueError, match=r"null_behavior='drop'.*height"):
        c("x").diff(1, "drop")
    r = c("x").rolling_mean(7)
    assert (r.kind, r.op, r.value) == ("rolling", F.ROLLING_MEAN, (7, 7, False)) and repr(r) == "col('x').rolling_mean(7)"
    assert repr(c("x").rolling_sum(5, min_samples=2, center=True).over("k")) == "col('x').rolling_sum(5, min_samples=2, center=True).over([col('k')])"
    assert [getattr(c("x"), nm)(3).op for nm in R.OPS] == [0, 1, 2, 3] == [F.ROLLING_OPS[nm] for nm in R.OPS]
    assert (F.AE_SHIFT, F.AE_ROLLING, F.SHIFT_SHIFT, F.SHIFT_DIFF) == (18, 19, 0, 1)
    for nm in R.OPS:
        fn = getattr(c("x"), nm)
        assert fn(np.int32(4), min_samples=np.int64(2)).value == (4, 2, False)
        for bad in (0, -1, 2 ** 31):
            with pytest.raises(ValueError, match="window_size"):
                fn(bad)
        for bad in (2.0, None, True):
            with pytest.raises(TypeError, match="window_size"):
                fn(bad)
        with pytest.raises(ValueError, match="temporal window"):
            fn("7d")
        with pytest.raises(ValueError, match=r"weights"):
            fn(3, [1.0, 2.0, 3.0])
        for bad in (0, 4, -2):
            with pytest.raises(ValueError, match="min_samples"):
                fn(3, min_samples=bad)
        with pytest.raises(TypeError, match="min_samples"):
            fn(3, min_samples=1.5)
        for bad in (1, "yes", None):
            with pytest.raises(TypeError, match="center"):
                fn(3, center=bad)
    assert not any(hasattr(pl.Expr, nm) for nm in ("rolling_var", "rolling_std", "rolling_median", "rolling_quantile", "pct_change"))
    # the module-level shorthands mirror the methods
    assert repr(pl.shift("x", 2, fill_value=1)) == repr(c("x").shift(2, fill_value=1)) and repr(pl.diff("x", -1)) == repr(c("x").diff(-1))
    for nm in R.OPS:
        assert repr(getattr(pl, nm)("x", 5, min_samples=2, center=True)) == repr(getattr(c("x"), nm)(5, min_samples=2, center=True))
    assert all(name in pl.__all__ for name in ("shift", "diff") + R.OPS) and all(hasattr(pl.Series, name) for name in ("shift", "diff") + R.OPS)
    # the packed literal
    assert F.rolling_pack(2048, 7, True) == 2048 | (7 << 32) | (1 << 63) and F.rolling_unpack(F.rolling_pack(5, 5, False)) == (5, 5, False)
    w = c("x").rolling_min(3).over("k")
    assert w.kind == "window" and w.lhs.kind == "rolling" and w.lhs.children() == [w.lhs.lhs]


def test_lowering_into_the_two_kinds_with_the_packed_literal(df):
    lf = df.lazy().select(c("a").shift(2).alias("s"), c("x").shift(-1, fill_value=0).alias("sf"), c("s").shift(1, fill_value="R").alias("cat"), c("d").shift(3).alias("ds"),
                          c("flag").shift(1, fill_value=True).alias("b"), c("u8").diff().alias("d8"), c("u16").diff(2).alias("d16"), c("u").diff().alias("d32"),
                          c("u64").diff().alias("d64"), c("a").diff(-1).alias("da"), c("f").diff().alias("df"),
                          c("a").rolling_sum(3).alias("rs"), c("flag").rolling_sum(3).alias("rb"), c("f").rolling_sum(3).alias("rf"), c("a").rolling_mean(4, min_samples=2).alias("rm"),
                          c("f").rolling_mean(4).alias("rmf"), c("d").rolling_min(5, center=True).alias("rd"), c("t").rolling_max(2).alias("rt"), c("flag").rolling_max(2).alias("rfl"))
    low, root, schema = lf._lower()
    assert schema == {"s": pl.Int8, "sf": pl.Float64, "cat": pl.Categorical(), "ds": pl.Date, "b": pl.Boolean, "d8": pl.Int16, "d16": pl.Int32, "d32": pl.Int64, "d64": pl.Int64,
                      "da": pl.Int8, "df": pl.Float32, "rs": pl.Int64, "rb": pl.UInt32, "rf": pl.Float32, "rm": pl.Float64, "rmf": pl.Float32, "rd": pl.Date, "rt": pl.Datetime,
                      "rfl": pl.Boolean}
    assert list(schema["cat"].categories) == ["A", "N", "R"]                     # the dictionary travels with a shifted Categorical
    tops = []
    for e in low.irs[root]["exprs"]:
        d = low.aexprs[e]
        while d["kind"] == F.AE_ALIAS:
            d = low.aexprs[d["lhs"]]
        tops.append(d)
    P = F.rolling_pack
    assert [(d["kind"], d["op"], d["lit"]) for d in tops] == [(18, 0, 2), (18, 0, -1), (18, 0, 1), (18, 0, 3), (18, 0, 1), (18, 1, 1), (18, 1, 2), (18, 1, 1), (18, 1, 1), (18, 1, -1),
                                                              (18, 1, 1), (19, 0, P(3, 3, False)), (19, 0, P(3, 3, False)), (19, 0, P(3, 3, False)), (19, 1, P(4, 2, False)),
                                                              (19, 1, P(4, 4, False)), (19, 2, P(5, 5, True)), (19, 3, P(2, 2, False)), (19, 3, P(2, 2, False))]
    fills = [low.aexprs[d["rhs"]] if d["rhs"] >= 0 else None for d in tops]
    assert [None if f is None else (f["kind"], f["dtype"], f["lit"], f["is_null"]) for f in fills[:5]] == [None, (F.AE_LITERAL, F.F64, 0.0, 0), (F.AE_LITERAL, F.U8, 2, 0), None,
                                                                                                           (F.AE_LITERAL, F.BOOL, True, 0)]
    assert all(f is None for f in fills[5:]) and all(d["cond"] == -1 and low.aexprs[d["lhs"]]["kind"] == F.AE_COLUMN for d in tops)
    # the parameters travel in fields the struct has: op, n in lit.i, the packed triple in lit.u; plx_aexpr keeps its 48 bytes
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr._fields_[-1][0] == "cond"
    assert [(ae[i].op, ae[i].lit.i) for i in range(n_ae) if ae[i].kind == 18] == [(d["op"], d["lit"]) for d in tops if d["kind"] == 18]
    assert [(ae[i].op, ae[i].lit.u) for i in range(n_ae) if ae[i].kind == 19] == [(d["op"], d["lit"]) for d in tops if d["kind"] == 19]
    assert [F.rolling_unpack(ae[i].lit.u) for i in range(n_ae) if ae[i].kind == 19][-3] == (5, 5, True)
    # an n beyond 64 bits is clamped in the node (every row is vacated either way)
    low, root, _ = df.lazy().select(c("x").shift(2 ** 70), c("a").shift(-2 ** 70))._lower()
    assert sorted(d["lit"] for d in low.aexprs if d["kind"] == 18) == [-2 ** 63, 2 ** 63 - 1]
    # the window-wrapped form, an operand expression, an alias below .over
    low, root, schema = df.lazy().with_columns((c("a") * c("a")).rolling_sum(5).over("k", "k2").alias("run"), c("x").shift(1).alias("z").over("k")).filter(
        c("x").diff().over("k") > 0.0)._lower()
    assert schema["run"] == pl.Int64 and schema["z"] == pl.Float64
    wins = [d for d in low.aexprs if d["kind"] == F.AE_WINDOW]
    fns = []
    for w in wins:
        f = low.aexprs[w["lhs"]]
        while f["kind"] == F.AE_ALIAS:
            f = low.aexprs[f["lhs"]]
        fns.append((f["kind"], f["op"]))
        assert low.aexprs[w["rhs"]]["kind"] == F.AE_WINDOW_KEY
    assert fns == [(19, 0), (18, 0), (18, 1)] and low.aexprs[[d for d in low.aexprs if d["kind"] == 19][0]["lhs"]]["kind"] == F.AE_BINARY
    with pytest.raises(KeyError, match="column not found: zz"):
        df.lazy().select(c("zz").rolling_sum(3))._lower()


def test_fill_values_the_dtype_cannot_hold_are_refused_by_name(df):
    for col, fill in (("a", 300), ("a", 1.5), ("a", "x"), ("a", True), ("u", -1), ("f", 0.1), ("f", 2 ** 24 + 1), ("x", "1"), ("x", 2 ** 53 + 1), ("flag", 1), ("s", "Z"), ("s", 1),
                      ("d", 1.5), ("d", dt.datetime(2020, 1, 1)), ("t", dt.date(2020, 1, 1)), ("u64", 2 ** 64)):
        with pytest.raises(TypeError, match=r"shift\(fill_value=.*cannot hold this fill_value exactly"):
            df.lazy().select(c(col).shift(1, fill_value=fill))._lower()
    ok = (("a", 127), ("a", -128), ("a", 3.0), ("f", 0.5), ("f", float("inf")), ("f", float("nan")), ("x", 0.1), ("x", 7), ("flag", False), ("s", "A"), ("d", dt.date(1999, 1, 2)), ("d", 10),
          ("t", dt.datetime(1999, 1, 2, 3, 4, 5)), ("u64", 2 ** 64 - 1), ("u8", np.uint8(200)))
    for col, fill in ok:
        low, root, schema = df.lazy().select(c(col).shift(1, fill_value=fill))._lower()
        node = [d for d in low.aexprs if d["kind"] == 18][0]
        assert low.aexprs[node["rhs"]]["dtype"] == df.schema[col].physical, (col, fill)
    low, _, _ = df.lazy().select(c("d").shift(1, fill_value=dt.date(1970, 1, 11)), c("t").shift(1, fill_value=dt.datetime(1970, 1, 1, 0, 0, 1)))._lower()
    assert [low.aexprs[d["rhs"]]["lit"] for d in low.aexprs if d["kind"] == 18] == [10, 1_000_000]


def test_operand_dtypes_are_refused_by_name(df):
    for e, word in ((c("flag").diff(), "diff"), (c("d").diff(), "diff"), (c("t").diff(), "diff"), (c("s").diff(), "diff"), (c("s").rolling_sum(2), "rolling_sum"),
                    (c("s").rolling_mean(2), "rolling_mean"), (c("s").rolling_min(2), "rolling_min"), (c("s").rolling_max(2).over("k"), "rolling_max"),
                    (c("d").rolling_sum(2), "rolling_sum"), (c("t").rolling_mean(2), "rolling_mean")):
        with pytest.raises(TypeError, match=word + r"\(\) needs"):
            df.lazy().select(e)._lower()
    with pytest.raises(TypeError, match="Duration"):
        df.lazy().select(c("d").diff())._lower()
    assert df.lazy().select(c("d").rolling_min(2)).collect_schema() == {"d": pl.Date} and df.lazy().select(c("t").rolling_max(2)).collect_schema() == {"t": pl.Datetime}
    assert pl.plan.rolling_result_dtype(F.ROLLING_SUM, pl.UInt16) == pl.Int64 and pl.plan.shift_result_dtype(F.SHIFT_DIFF, pl.UInt64) == pl.Int64


def test_the_header_numbering_and_the_exported_symbols(tmp_path):
    src = tmp_path / "rolling.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AE_SHIFT == 18 && PLX_AE_ROLLING == 19 && PLX_AE_CUMULATIVE == 16 && PLX_AE_RANK == 17, "numbering");
_Static_assert(PLX_ROLLING_SUM == 0 && PLX_ROLLING_MEAN == 1 && PLX_ROLLING_MIN == 2 && PLX_ROLLING_MAX == 3, "plx_rolling_op");
_Static_assert(sizeof(plx_aexpr) == 48, "plx_aexpr did not grow");
_Static_assert(offsetof(plx_aexpr, cond) == 40 && offsetof(plx_aexpr, lit) == 24 && offsetof(plx_aexpr, rhs) == 12, "the fields are where they were");
int (*p1)(const plx_column*, int32_t, plx_column, int64_t, const plx_scalar*, int32_t, plx_column*) = plx_shift;
int (*p2)(const plx_column*, int32_t, plx_column, int32_t, int64_t, int64_t, int32_t, plx_column*) = plx_rolling;
void (*p3)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_shift;
void (*p4)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_shift;
void (*p5)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_diff;
void (*p6)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_diff;
void (*p7)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_rolling;
void (*p8)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_rolling;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "rolling.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("plx_shift", "plx_rolling", "_polars_plugin_plx_shift", "_polars_plugin_field_plx_shift", "_polars_plugin_plx_diff", "_polars_plugin_field_plx_diff",
                 "_polars_plugin_plx_rolling", "_polars_plugin_field_plx_rolling"):
        assert hasattr(F.lib(), name), name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(w in text for w in ("plx_shift", "plx_rolling", "PLX_AE_SHIFT", "PLX_AE_ROLLING", "plx_diff", "PLX_ROLLING_ROUTE"))
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert "4.19" in text and "kRollingMaxWindow" in text and "polars wheel" in text


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def import_error(low, root):
    """what plan import says about the arenas (plx_debug_program_json imports the plan first): (code, message)"""
    buf = C.create_string_buffer(1 << 14)
    ir, n_ir, ae, n_ae, keep = low.to_c()
    rc = F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf))
    return rc, F.lib().plx_last_error().decode()


def test_the_mirror_api_refuses_by_name(df):
    for lf in (df.lazy().group_by("k").agg(c("x").shift()), df.lazy().group_by(c("a").diff()).agg(c("x").sum()), df.lazy().group_by("k").agg(c("x").rolling_sum(3)),
               df.lazy().group_by("k").agg((c("x").sum() + c("x").rolling_max(2).over("k2")).alias("z"))):
        with pytest.raises(TypeError, match=r"group_by: a cumulative / ranking expression or a shift / diff / rolling expression"):
            lf._lower()
    for e, word in ((c("x").sum().shift(), "an aggregate"), (pl.len().rolling_sum(2), "an aggregate"), ((c("x") - c("x").mean()).diff(), "an aggregate"),
                    (c("x").sum().over("k").rolling_max(3), "a window expression"), (c("x").shift().rolling_sum(2), "inside the operand of another one"),
                    (c("x").rolling_sum(2).shift(), "inside the operand of another one"), (c("x").cum_sum().diff(), "inside the operand of another one"),
                    (c("x").rolling_mean(2).rank(), "inside the operand of another one"), (c("x").diff().cum_sum(), "inside the operand of another one"),
                    ((c("x").shift().over("k") + 1).rolling_sum(2), "a window expression")):
        with pytest.raises(TypeError, match=word):
            df.lazy().select(e)._lower()
    for e in ((c("x").rolling_sum(3) / c("x").sum()).over("k"), (c("x").shift() + 1).over("k"), (c("x") - c("x").shift()).alias("z").over("k")):
        with pytest.raises(TypeError, match=r"mixes a cumulative / ranking expression \(or a shift / diff / rolling expression\)"):
            df.lazy().select(e)._lower()
    # the arithmetic outside the .over()s lowers
    low, root, schema = df.lazy().select((c("x") - c("x").shift(1).over("k")).alias("change"), (c("x").rolling_sum(3).over("k") / c("x").sum().over("k")).alias("share"))._lower()
    assert schema == {"change": pl.Float64, "share": pl.Float64} and sum(d["kind"] == F.AE_WINDOW for d in low.aexprs) == 3
    with pytest.raises(ValueError, match="order_by"):
        c("x").shift().over("k", order_by="x")


def test_plan_import_validates_the_new_kinds(df):
    ERR_INVALID = 1
    low, root, _ = df.lazy().select(c("x").shift(1, fill_value=0.5))._lower()
    top = low.irs[root]["exprs"][0]
    col_node = low.aexprs[top]["lhs"]
    for field, value, word in (("op", 2, "neither 0 (shift) nor 1 (diff)"), ("op", -1, "neither 0"), ("lhs", -1, "needs an operand"), ("rhs", col_node, "non-null literal"),
                               ("op", 1, "diff takes none")):
        saved = low.aexprs[top][field]
        low.aexprs[top][field] = value
        rc, msg = import_error(low, root)
        assert rc == ERR_INVALID and word in msg, (field, value, msg)
        low.aexprs[top][field] = saved
    low, root, _ = df.lazy().select(c("x").rolling_min(3, min_samples=2))._lower()
    top = low.irs[root]["exprs"][0]
    for field, value, word in (("op", 4, "no plx_rolling_op"), ("lit", F.rolling_pack(0, 0, False), "window_size"), ("lit", F.rolling_pack(3, 4, False), "min_samples"),
                               ("lit", F.rolling_pack(3, 0, True), "min_samples"), ("lit", 2 ** 31, "window_size"), ("lhs", -1, "needs an operand")):
        saved = low.aexprs[top][field]
        low.aexprs[top][field] = value
        rc, msg = import_error(low, root)
        assert rc == ERR_INVALID and word in msg, (field, value, msg)
        low.aexprs[top][field] = saved
    # in the keys or the aggregate list of a group_by: PLX_ERR_INVALID naming them (arenas a caller other than the mirror API may send)
    low, root, _ = df.lazy().group_by("k").agg(c("x").sum())._lower()
    agg = low.irs[root]["exprs"][0]
    low.aexprs[agg]["kind"], low.aexprs[agg]["op"], low.aexprs[agg]["lit"] = F.AE_ROLLING, F.ROLLING_SUM, F.rolling_pack(3, 3, False)
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "shift / diff / rolling expression" in msg and "aggregate list of a group_by" in msg, msg
    low, root, _ = df.lazy().group_by(c("a").cast(pl.Int64)).agg(c("x").sum())._lower()
    key = low.irs[root]["keys"][0]
    low.aexprs[key]["kind"], low.aexprs[key]["op"], low.aexprs[key]["dtype"], low.aexprs[key]["lit"] = F.AE_SHIFT, 0, 0, 1
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "shift / diff / rolling expression" in msg and "keys of a group_by" in msg, msg
    low, root, _ = df.lazy().select(c("x").rolling_sum(2).over(*["k"] * 9))._lower()
    rc, msg = import_error(low, root)
    assert rc == F.ERR_UNSUPPORTED and "window over 9 keys" in msg and "1..8" in msg, msg


def test_fused_pipelines_decline_by_name(df):
    for lf in (df.lazy().select(c("x").shift()), df.lazy().select(c("x").rolling_mean(3).over("k")), df.lazy().select((c("x") - c("x").shift().over("k")).sum()),
               df.lazy().filter(c("x").diff().over("k") > 0.0).select(c("x").sum()), df.lazy().filter(c("x").rolling_sum(3, min_samples=1) > 1.0).group_by("k").agg(c("x").sum())):
        fused, _, why, _ = lf.describe_fusion()
        assert not fused and why == REASON, why
    fused, _, why, _ = df.lazy().select(c("x").cum_sum()).describe_fusion()                    # the cumulative functions keep their own reason
    assert not fused and why == "cumulative / ranking expression: per-node route", why
    fused, _, why, _ = df.lazy().filter(c("x") > 0).select(c("x").sum()).describe_fusion()      # the same query without one still fuses
    assert fused, why


# ---- explain() and the pushdown rules ---------------------------------------------------------------------------------------------------------------------
def test_explain_lines(df):
    text = df.lazy().with_columns(c("x").shift(2, fill_value=0.0).alias("s"), (c("a") * c("a")).rolling_max(3, min_samples=1, center=True).over("k", "k2").alias("m")).filter(
        c("x").diff().alias("r").over("k") <= 3.0).explain()
    assert "Shift[col('x').shift(2, fill_value=0.0) over the whole column] in with_columns" in text, text
    assert f"Rolling[{(c('a') * c('a'))!r}.rolling_max(3, min_samples=1, center=True) over [col('k'), col('k2')]] in with_columns" in text, text
    assert "Shift[col('x').diff(1) over [col('k')]] in filter" in text, text
    assert "Window[" not in text                                                                # a window of one of these is its line, not a window line ...
    text = df.lazy().select(c("x").sum().over("k"), c("x").rolling_sum(7), c("x").cum_count()).explain()
    assert "Window[col('x').agg0() over [col('k')]" in text and "Rolling[col('x').rolling_sum(7) over the whole column] in select" in text and "Cumulative[" in text, text


def test_no_predicate_and_no_slice_is_pushed_through(tmp_path):
    """A shift / diff / rolling expression reads the rows around each row.  The simple conjuncts of a filter that holds one, and of the filters above it, must not
    reach the scan; a filter BELOW it still prunes.  A slice stops at a node that holds one."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from polars_amd import io
    n = 5000
    path = str(tmp_path / "c.parquet")
    pq.write_table(pa.table({"k": pa.array(np.arange(n) % 7), "x": pa.array(np.arange(n, dtype=np.float64)), "y": pa.array(np.arange(n))}), path, row_group_size=500)

    def scan_of(lf):
        io.reset_scans(lf._node); io.push_down(lf._node)
        node = lf._node
        while node.kind != "scan":
            node = node.input
        return node.frame
    for pred in (c("x").shift(1) > 100.0, c("x").rolling_sum(3).over("k") <= 3.0, c("x").diff().over("k") > 2.0):
        for lf in (pl.scan_parquet(path).filter((c("y") > 2500) & pred), pl.scan_parquet(path).filter(pred).filter(c("y") > 2500)):
            src = scan_of(lf)
            assert src._preds == [] and len(src.selected_row_groups()) == 10, src._preds
            assert "STATISTICS PRUNING" not in lf.explain(), lf.explain()
        lf = pl.scan_parquet(path).filter(c("y") > 2500).filter(pred & (c("y") < 4000))          # below it the rows never reach it: pruned as before
        src = scan_of(lf)
        assert src._preds == [("y", F.OP_GT, 2500)] and len(src.selected_row_groups()) == 5
    for node_lf in (pl.scan_parquet(path).with_columns(c("x").shift(1).alias("s")), pl.scan_parquet(path).select(c("x").rolling_min(3)),
                    pl.scan_parquet(path).select(c("x"), c("y").diff().over("k").alias("m"))):
        assert io.scan_under(node_lf._node) is None
        src = scan_of(node_lf.slice(1000, 10))
        assert len(src.selected_row_groups()) == 10, "a slice above a shifted value was pushed into the scan"


# ---- the plugin symbols and the C entries without a device ---------------------------------------------------------------------------------------------------
def test_plugin_fields_and_entry_points_without_a_device():
    import pyarrow as pa
    import torch

    from tests import plugin_abi as P
    for t in (pa.int8(), pa.uint32(), pa.float32(), pa.bool_(), pa.date32()):
        assert P.field("plx_shift", t, {"n": 2}).type == t, t
    for t, want in ((pa.uint8(), pa.int16()), (pa.uint16(), pa.int32()), (pa.uint32(), pa.int64()), (pa.uint64(), pa.int64()), (pa.int8(), pa.int8()), (pa.int64(), pa.int64()),
                    (pa.float32(), pa.float32()), (pa.float64(), pa.float64())):
        assert P.field("plx_diff", t, {"n": 1}).type == want, t
    assert P.field("plx_diff", pa.bool_(), {}) is None and "integer and float series only" in P.last_error()
    assert P.field("plx_diff", pa.date32(), {}) is None and "integer and float series only" in P.last_error()
    for op, t, want in (("sum", pa.int8(), pa.int64()), ("sum", pa.bool_(), pa.uint32()), ("sum", pa.float32(), pa.float32()), ("sum", pa.uint64(), pa.uint64()),
                        ("mean", pa.int16(), pa.float64()), ("mean", pa.float32(), pa.float32()), ("min", pa.int16(), pa.int16()), ("max", pa.bool_(), pa.bool_()),
                        ("min", pa.date32(), pa.date32())):
        assert P.field("plx_rolling", t, {"op": op, "window_size": 3}).type == want, (op, t)
    assert P.field("plx_rolling", pa.float64(), {"op": "sum", "window_size": 3}, col_name="x").name == "x"
    assert P.field("plx_rolling", pa.float64(), {"op": "var", "window_size": 3}) is None and "kwargs must carry op in {sum, mean, min, max}" in P.last_error()
    assert P.field("plx_rolling", pa.float64(), {}) is None and "kwargs must carry op" in P.last_error()
    if torch.cuda.is_available():
        return
    res, inp = P.call("plx_shift", [pa.array([1.0, 2.0]), pa.array([1, 1])], {"n": 1})
    assert res is None and inp.released == 2 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    # the parameters are refused by name before anything runs
    h = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.I64, 100, 0, 0, 0, 0, C.byref(h)) == 0
    keys, out = (C.c_uint64 * 9)(*([h.value] * 9)), C.c_uint64()
    err = lambda: F.lib().plx_last_error().decode()
    fill = F.Scalar()
    assert F.lib().plx_shift(keys, 1, h.value, 1, None, 2, C.byref(out)) == 1 and "diff must be 0 or 1" in err()
    assert F.lib().plx_shift(keys, 1, h.value, 1, C.byref(fill), 1, C.byref(out)) == 1 and "fill must be NULL" in err()
    assert F.lib().plx_shift(keys, 9, h.value, 1, None, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in err()
    assert F.lib().plx_shift(None, 2, h.value, 1, None, 0, C.byref(out)) == 1 and "n_keys" in err()
    assert F.lib().plx_rolling(keys, 1, h.value, 4, 3, 3, 0, C.byref(out)) == 1 and "no plx_rolling_op" in err()
    assert F.lib().plx_rolling(keys, 1, h.value, 0, 0, 1, 0, C.byref(out)) == 1 and "window_size" in err()
    assert F.lib().plx_rolling(keys, 1, h.value, 0, 3, 4, 0, C.byref(out)) == 1 and "min_samples" in err()
    assert F.lib().plx_rolling(keys, 1, h.value, 0, 3, 0, 0, C.byref(out)) == 1 and "min_samples" in err()
    assert F.lib().plx_rolling(keys, 1, h.value, 0, 3, 3, 2, C.byref(out)) == 1 and "center must be 0 or 1" in err()
    assert F.lib().plx_rolling(keys, 9, h.value, 0, 3, 3, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in err()
    short = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.I64, 99, 0, 0, 0, 0, C.byref(short)) == 0
    assert F.lib().plx_rolling((C.c_uint64 * 1)(short.value), 1, h.value, 0, 3, 3, 0, C.byref(out)) != 0 and "key length mismatch" in err()


def test_the_example_queries_lower():
    from polars_amd import queries as QQ
    rng = np.random.default_rng(12)
    n = 2000
    cols = {"l_returnflag": (rng.integers(0, 3, n).astype(np.uint8), None), "l_quantity": (rng.integers(1, 51, n).astype(np.float64), None),
            "l_discount": (rng.integers(0, 11, n) / 100.0, None), "l_extendedprice": (rng.uniform(900.0, 100000.0, n), None)}
    low, root, schema = QQ.moving_average_revenue_by_flag(frame_like(cols).lazy())._lower()
    assert schema["revenue_ma7"] == pl.Float64 and low.irs[root]["kind"] == F.IR_HSTACK
    roll = [d for d in low.aexprs if d["kind"] == F.AE_ROLLING]
    assert len(roll) == 1 and (roll[0]["op"], roll[0]["lit"]) == (F.ROLLING_MEAN, F.rolling_pack(7, 1, False)) and low.aexprs[roll[0]["lhs"]]["kind"] == F.AE_BINARY
    low, root, schema = QQ.quantity_change_by_flag(frame_like(cols).lazy())._lower()
    assert schema["quantity_change"] == pl.Float64 and schema["previous_quantity"] == pl.Float64
    assert sorted((d["op"], d["lit"]) for d in low.aexprs if d["kind"] == F.AE_SHIFT) == [(0, 1), (1, 1)] and sum(d["kind"] == F.AE_WINDOW for d in low.aexprs) == 2


# ---- the new kernels' registers and LDS ------------------------------------------------------------------------------------------------------------
def test_rolling_kernels_run_without_scratch_and_within_the_lds_budget():
    """every form of the kernels of kernels_rolling.hip: no scratch (a lane's region positions stay in registers); the tile route's static LDS at or below the
    64 KiB of DESIGN.md 4.19 (two workgroups in a CU's 160 KiB); the other kernels hold the four wave totals only."""
    from tests.test_kernel_resources_cpu import resource_usage
    res = resource_usage("kernels_rolling.hip")
    names = ("shift_kernel", "rolling_tile_kernel", "rolling_reduce_kernel", "rolling_aggscan_kernel", "rolling_scan_kernel", "rolling_combine_kernel")
    assert all(any(w in n for n in res) for w in names) and len(res) >= 17 * 5 + 14, len(res)
    for name, r in sorted(res.items()):
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        lds = int(r["LDS Size [bytes/block]"])
        if "rolling_tile_kernel" in name:
            assert 0 < lds <= LDS_BUDGET and 2 * lds <= 160 * 1024, (name, lds)
            assert int(r["VGPRs"]) <= 256, (name, r)                                            # one workgroup of four waves per SIMD set: the register file is not the limit, LDS is
        else:
            assert lds <= 64 and int(r["VGPRs"]) <= 128, (name, r)


# ---- the visitor's function nodes through the engine shim ------------------------------------------------------------------------------------------
def test_polars_engine_maps_the_function_nodes(df):
    """A stand-in NodeTraverser shows PLX_AE_SHIFT / PLX_AE_ROLLING as the visitor's Function node: ("shift",) [x, n], ("shift_and_fill",) [x, n, fill],
    ("diff", null_behavior) [x, n], (rolling name, window_size, min_periods, weights, center) [x].  The shim builds the same arenas back, plain and under a Window
    node; weights, a temporal window, n as an expression and null_behavior="drop" are refused by name."""
    from polars_amd import polars_engine as eng
    from tests import test_polars_engine_cpu as S

    class Node:
        def __init__(self, **kw): self.__dict__.update(kw)

    class Mapping:
        kind = "groups_to_rows"

    NAMES = {v: k for k, v in F.ROLLING_OPS.items()}
    BASE = 1_000_000

    class WithFunctions(S.FakeTraverser):
        weights, window, behavior, n_as_column = None, None, "ignore", False

        def view_expression(self, i):
            if i >= BASE:                                   # the n of a shift / diff: an input expression of its own
                owner = self.low.aexprs[i - BASE]
                return S.Column(name="a") if self.n_as_column else S.Literal(value=owner["lit"], dtype=S.PHYS[F.I64])
            d = self.low.aexprs[i]
            if d["kind"] == F.AE_WINDOW:
                keys, link = [], d["rhs"]
                while link >= 0:
                    keys.append(self.low.aexprs[link]["lhs"])
                    link = self.low.aexprs[link]["rhs"]
                return type("Window", (Node,), {})(function=d["lhs"], partition_by=keys, order_by=None, options=Mapping())
            if d["kind"] == F.AE_SHIFT and d["op"] == F.SHIFT_DIFF:
                return type("Function", (Node,), {})(input=[d["lhs"], BASE + i], function_data=("diff", self.behavior), options=None)
            if d["kind"] == F.AE_SHIFT:
                if d["rhs"] >= 0:
                    return type("Function", (Node,), {})(input=[d["lhs"], BASE + i, d["rhs"]], function_data=("shift_and_fill",), options=None)
                return type("Function", (Node,), {})(input=[d["lhs"], BASE + i], function_data=("shift",), options=None)
            if d["kind"] == F.AE_ROLLING:
                w, m, ctr = F.rolling_unpack(d["lit"])
                return type("Function", (Node,), {})(input=[d["lhs"]], function_data=(NAMES[d["op"]], self.window or w, m, self.weights, ctr), options=None)
            return super().view_expression(i)

    lf = df.lazy().with_columns(c("x").shift(2).alias("s"), c("x").shift(-1, fill_value=0.5).over("k", "k2").alias("sf"), c("a").diff(3).alias("d"),
                                c("x").rolling_mean(7, min_samples=2, center=True).alias("m"), c("a").rolling_sum(3).over("k").alias("r")).filter(c("x").rolling_max(4).over("k") <= 3.0)
    low, root, _ = lf._lower()
    back = eng.Translator(WithFunctions(low, root), frame_of=lambda node: node.df).plan()
    low2, root2, _ = back._lower()
    assert S.canonical(low, root) == S.canonical(low2, root2)
    params = lambda lw: sorted((d["kind"], d["op"], d["lit"]) for d in lw.aexprs if d["kind"] in (F.AE_SHIFT, F.AE_ROLLING))
    assert params(low) == params(low2) == sorted([(18, 0, 2), (18, 0, -1), (18, 1, 3), (19, 1, F.rolling_pack(7, 2, True)), (19, 0, F.rolling_pack(3, 3, False)),
                                                  (19, 3, F.rolling_pack(4, 4, False))])
    for attrs, word in (({"weights": [1.0, 2.0]}, "with weights"), ({"window": "7d"}, "temporal window"), ({"behavior": "drop"}, "null_behavior=drop"),
                        ({"n_as_column": True}, "n must be an integer literal")):
        nt = WithFunctions(low, root)
        for key, value in attrs.items():
            setattr(nt, key, value)
        with pytest.raises(eng.NotSupported, match=word):
            eng.Translator(nt, frame_of=lambda node: node.df).plan()
