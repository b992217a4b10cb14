"""Cumulative and ranking functions without a GPU: the arithmetic of csrc/cumulative.hpp as a stand-alone program under -fsanitize=address,undefined against a
sequential loop; the numpy reference's own check; the validators and reprs; the lowering to PLX_AE_CUMULATIVE = 16 / PLX_AE_RANK = 17 and the window-wrapped form;
the header's numbering, plx_aexpr's size and the prototypes through a compiled C caller; every refusal by message; explain(); no predicate or slice pushed through;
the fused compiler declining by name; the visitor's function nodes through the engine shim; the plugin fields; the example queries; the kernels' registers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import cumulative_ref as R
from tests.test_program_eval_cpu import frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
REASON = "cumulative / ranking expression: per-node route"


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_under_sanitizers_against_a_sequential_loop(tmp_path):
    """tests/emu/cumulative_main.cpp: tile reduce, the scan of the aggregates (its recursive level included) and the tile scan with carry, lane by lane, both index
    directions, over the segment patterns and validity patterns of the GPU tests; the rank formulas against counting."""
    exe = str(tmp_path / "cumulative_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "cumulative_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+) levels=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 1_000_000 and int(m.group(3)) >= 2, r.stdout


def test_the_reference():
    assert R.self_check() == 22
    x = np.array([1.5, 2.5, -1.0], np.float32)
    v, ok, scale = R.cum("cum_sum", x)
    assert v.dtype == np.float64 and v.tolist() == [1.5, 4.0, 3.0] and scale.tolist() == [1.5, 4.0, 5.0] and R.result_dtype("cum_sum", x.dtype) == np.float32
    R.check_cum(np.array([1.5, 4.0, 3.0], np.float32), None, "cum_sum", x)
    with pytest.raises(AssertionError):
        R.check_cum(np.array([1.5, 4.0, 3.5], np.float32), None, "cum_sum", x)
    with pytest.raises(AssertionError):                                   # the result dtype is part of the check
        R.check_cum(np.array([1.5, 4.0, 3.0]), None, "cum_sum", x)
    with pytest.raises(AssertionError):
        R.check_rank(np.array([1, 2, 3], np.uint32), None, np.array([5, 6, 6]), None, "min", False)
    R.check_rank(np.array([1, 2, 2], np.uint32), None, np.array([5, 6, 6]), None, "min", False)


# ---- the mirror API ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def df():
    rng = np.random.default_rng(418)
    n = 301
    cols = {"k": (rng.integers(0, 7, n).astype(np.int64), None), "k2": (rng.integers(0, 3, n).astype(np.int32), rng.random(n) < 0.9), "x": (rng.normal(3.0, 2.0, n), None),
            "a": (rng.integers(-300, 300, n).astype(np.int8), None), "f": (rng.normal(size=n).astype(np.float32), None), "flag": (rng.random(n) < 0.5, None),
            "d": (rng.integers(8000, 11000, n).astype(np.int32), None), "s": (rng.integers(0, 3, n).astype(np.uint8), None), "u": (rng.integers(0, 9, n).astype(np.uint32), None)}
    return frame_like(cols, {"d": pl.Date, "s": pl.Categorical(["A", "N", "R"], pl.UInt8), "f": pl.Float32})


def test_validators_and_reprs():
    e = c("x").cum_sum()
    assert (e.kind, e.op, e.value) == ("cum", F.CUM_SUM, False) and repr(e) == "col('x').cum_sum()"
    assert repr(c("x").cum_min(reverse=True)) == "col('x').cum_min(reverse=True)" and repr(c("x").cum_max()) == "col('x').cum_max()"
    assert repr((c("a") * c("x")).cum_count(reverse=True).over("k")) == f"{(c('a') * c('x'))!r}.cum_count(reverse=True).over([col('k')])"
    r = c("x").rank()
    assert (r.kind, r.op, r.value) == ("rank", F.RANK_AVERAGE, ("average", False)) and repr(r) == "col('x').rank('average')"
    assert repr(c("x").rank("ordinal", descending=True).over("k", "k2")) == "col('x').rank('ordinal', descending=True).over([col('k'), col('k2')])"
    assert [c("x").rank(m).op for m in ("average", "min", "max", "dense", "ordinal")] == [0, 1, 2, 3, 4] == [F.RANK_METHODS[m] for m in R.METHODS]
    assert (F.CUM_SUM, F.CUM_MIN, F.CUM_MAX, F.CUM_COUNT) == (0, 1, 2, 3) and F.AE_CUMULATIVE == 16 and F.AE_RANK == 17
    for bad in ("random", "first", "", None, 1):
        with pytest.raises(ValueError, match=r"\['average', 'min', 'max', 'dense', 'ordinal'\]"):
            c("x").rank(bad)
    for fn in (c("x").cum_sum, c("x").cum_min, c("x").cum_max, c("x").cum_count):
        for bad in (1, "yes", None):
            with pytest.raises(TypeError, match="reverse"):
                fn(reverse=bad)
    with pytest.raises(TypeError, match="descending"):
        c("x").rank("min", descending=1)
    assert pl.expr.check_rank_method("dense") == "dense" and pl.expr.check_reverse(np.bool_(True), "cum_sum") is True
    # the module-level shorthands mirror the methods
    assert repr(pl.cum_sum("x")) == repr(c("x").cum_sum()) and repr(pl.cum_min("x", reverse=True)) == repr(c("x").cum_min(reverse=True))
    assert repr(pl.cum_max("x")) == repr(c("x").cum_max()) and repr(pl.cum_count("x")) == repr(c("x").cum_count())
    assert repr(pl.rank("x", "dense", descending=True)) == repr(c("x").rank("dense", descending=True))
    assert all(name in pl.__all__ for name in ("cum_sum", "cum_min", "cum_max", "cum_count", "rank"))
    assert all(hasattr(pl.Series, name) for name in ("cum_sum", "cum_min", "cum_max", "cum_count", "rank"))
    # the operand and the keys are what walkers see
    w = c("x").cum_sum().over("k")
    assert w.kind == "window" and w.lhs.kind == "cum" and w.lhs.children() == [w.lhs.lhs] and w.children()[-1] is w.value[0]


def test_lowering_into_the_two_kinds_and_the_window_wrapped_form(df):
    lf = df.lazy().select(c("a").cum_sum().alias("s"), c("x").cum_min(reverse=True).alias("m"), c("s").cum_count().alias("n"), c("d").cum_max().alias("dm"),
                          c("flag").cum_sum().alias("t"), c("f").cum_sum().alias("fs"), c("u").cum_sum().alias("us"), c("flag").cum_max().alias("fm"),
                          c("x").rank().alias("r"), c("d").rank("ordinal", descending=True).alias("o"), c("flag").rank("dense").alias("b"))
    low, root, schema = lf._lower()
    assert schema == {"s": pl.Int64, "m": pl.Float64, "n": pl.UInt32, "dm": pl.Date, "t": pl.UInt32, "fs": pl.Float32, "us": pl.UInt32, "fm": pl.Boolean,
                      "r": pl.Float64, "o": pl.UInt32, "b": pl.UInt32}
    tops = []
    for e in low.irs[root]["exprs"]:
        d = low.aexprs[e]
        while d["kind"] == F.AE_ALIAS:
            d = low.aexprs[d["lhs"]]
        tops.append(d)
    assert [(d["kind"], d["op"], d["lit"]) for d in tops] == [(16, F.CUM_SUM, 0), (16, F.CUM_MIN, 1), (16, F.CUM_COUNT, 0), (16, F.CUM_MAX, 0), (16, F.CUM_SUM, 0), (16, F.CUM_SUM, 0),
                                                              (16, F.CUM_SUM, 0), (16, F.CUM_MAX, 0), (17, F.RANK_AVERAGE, 0), (17, F.RANK_ORDINAL, 1), (17, F.RANK_DENSE, 0)]
    assert all(d["rhs"] == -1 and d["cond"] == -1 and low.aexprs[d["lhs"]]["kind"] == F.AE_COLUMN for d in tops)
    # the parameters travel in fields the struct has: op, and reverse / descending in lit.u; plx_aexpr keeps its 48 bytes
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr._fields_[-1][0] == "cond"
    got = [(ae[i].kind, ae[i].op, ae[i].lit.u) for i in range(n_ae) if ae[i].kind in (16, 17)]
    assert got == [(d["kind"], d["op"], d["lit"]) for d in tops]
    # the window-wrapped form: PLX_AE_WINDOW whose lhs is the function; an operand expression; an alias below .over
    low, root, schema = df.lazy().with_columns((c("a") * c("a")).cum_sum().over("k", "k2").alias("run"), c("x").rank("min").alias("z").over("k")).filter(
        c("x").rank("ordinal", descending=True).over("k") <= 3)._lower()
    assert schema["run"] == pl.Int64 and schema["z"] == pl.UInt32
    wins = [d for d in low.aexprs if d["kind"] == F.AE_WINDOW]
    assert len(wins) == 3
    fns = []
    for w in wins:
        f = low.aexprs[w["lhs"]]
        while f["kind"] == F.AE_ALIAS:
            f = low.aexprs[f["lhs"]]
        fns.append((f["kind"], f["op"], f["lit"]))
        assert low.aexprs[w["rhs"]]["kind"] == F.AE_WINDOW_KEY
    assert fns == [(16, F.CUM_SUM, 0), (17, F.RANK_MIN, 0), (17, F.RANK_ORDINAL, 1)]
    assert low.aexprs[[d for d in low.aexprs if d["kind"] == 16][0]["lhs"]]["kind"] == F.AE_BINARY
    assert sum(d["kind"] == F.AE_WINDOW_KEY for d in low.aexprs) == 4
    pred = low.aexprs[low.irs[root]["predicate"]]
    assert pred["kind"] == F.AE_BINARY and low.aexprs[pred["lhs"]]["kind"] == F.AE_WINDOW and low.aexprs[pred["rhs"]]["dtype"] == F.U32      # the literal took the rank's dtype
    with pytest.raises(KeyError, match="column not found: zz"):
        df.lazy().select(c("zz").cum_sum())._lower()


def test_operand_dtypes_are_refused_by_name(df):
    for e, word in ((c("d").cum_sum(), "cum_sum"), (c("s").cum_sum(), "cum_sum"), (c("s").cum_min(), "cum_min"), (c("s").cum_max(), "cum_max"), (c("s").rank(), "rank"),
                    (c("s").rank("dense").over("k"), "rank")):
        with pytest.raises(TypeError, match=word + r"\(\) needs"):
            df.lazy().select(e)._lower()
    assert df.lazy().select(c("s").cum_count(), c("d").cum_min(), c("d").rank("max")).collect_schema() == {"s": pl.UInt32, "d": pl.UInt32}
    # (the last one wins the name; each by itself:)
    assert df.lazy().select(c("d").cum_min()).collect_schema() == {"d": pl.Date}
    assert pl.plan.cum_result_dtype(F.CUM_MAX, pl.Datetime) == pl.Datetime and pl.plan.rank_result_dtype("average", pl.Date) == pl.Float64


def test_the_header_numbering_and_the_exported_symbols(tmp_path):
    src = tmp_path / "cumulative.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AE_CUMULATIVE == 16 && PLX_AE_RANK == 17 && PLX_AE_WINDOW == 14 && PLX_AE_WINDOW_KEY == 15, "numbering");
_Static_assert(PLX_CUM_SUM == 0 && PLX_CUM_MIN == 1 && PLX_CUM_MAX == 2 && PLX_CUM_COUNT == 3, "plx_cum_op");
_Static_assert(PLX_RANK_AVERAGE == 0 && PLX_RANK_MIN == 1 && PLX_RANK_MAX == 2 && PLX_RANK_DENSE == 3 && PLX_RANK_ORDINAL == 4, "plx_rank_method");
_Static_assert(sizeof(plx_aexpr) == 48, "plx_aexpr did not grow");
_Static_assert(offsetof(plx_aexpr, cond) == 40 && offsetof(plx_aexpr, lit) == 24, "the fields are where they were");
int (*p1)(const plx_column*, int32_t, plx_column, int32_t, int32_t, plx_column*) = plx_cumulative;
int (*p2)(const plx_column*, int32_t, plx_column, int32_t, int32_t, plx_column*) = plx_rank;
void (*p3)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_cum;
void (*p4)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_cum;
void (*p5)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_rank;
void (*p6)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_rank;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "cumulative.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("plx_cumulative", "plx_rank", "_polars_plugin_plx_cum", "_polars_plugin_field_plx_cum", "_polars_plugin_plx_rank", "_polars_plugin_field_plx_rank"):
        assert hasattr(F.lib(), name), name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(w in text for w in ("plx_cumulative", "plx_rank", "PLX_AE_CUMULATIVE", "PLX_AE_RANK", "plx_cum"))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def import_error(low, root):
    """what plan import says about the arenas (plx_debug_program_json imports the plan first): (code, message)"""
    buf = C.create_string_buffer(1 << 14)
    ir, n_ir, ae, n_ae, keep = low.to_c()
    rc = F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf))
    return rc, F.lib().plx_last_error().decode()


def test_the_mirror_api_refuses_by_name(df):
    for lf in (df.lazy().group_by("k").agg(c("x").cum_sum()), df.lazy().group_by(c("a").rank("dense")).agg(c("x").sum()),
               df.lazy().group_by("k").agg((c("x").sum() + c("x").cum_max().over("k2")).alias("z"))):
        with pytest.raises(TypeError, match=r"group_by: a cumulative / ranking expression"):
            lf._lower()
    for e, word in ((c("x").sum().cum_sum(), "an aggregate"), (pl.len().cum_sum(), "an aggregate"), ((c("x") - c("x").mean()).rank(), "an aggregate"),
                    (c("x").sum().over("k").cum_max(), "a window expression"), (c("x").cum_sum().rank(), "inside the operand of another one"),
                    (c("x").rank().cum_count(), "inside the operand of another one"), ((c("x").cum_sum().over("k") + 1).cum_sum(), "a window expression")):
        with pytest.raises(TypeError, match=word):
            df.lazy().select(e)._lower()
    for e in ((c("x").cum_sum() / c("x").sum()).over("k"), (c("x").rank() + 1).over("k"), (c("x").cum_sum() * 2).alias("z").over("k")):
        with pytest.raises(TypeError, match="mixes a cumulative / ranking expression"):
            df.lazy().select(e)._lower()
    # the arithmetic outside the two .over()s lowers
    low, root, schema = df.lazy().select((c("x").cum_sum().over("k") / c("x").sum().over("k")).alias("share"))._lower()
    assert schema == {"share": pl.Float64} and sum(d["kind"] == F.AE_WINDOW for d in low.aexprs) == 2
    # what stays refused exactly as before
    with pytest.raises(ValueError, match="order_by"):
        c("x").cum_sum().over("k", order_by="x")
    for strategy in ("join", "explode"):
        with pytest.raises(ValueError, match="mapping_strategy"):
            c("x").rank().over("k", mapping_strategy=strategy)


def test_plan_import_validates_the_new_kinds(df):
    ERR_INVALID = 1
    low, root, _ = df.lazy().select(c("x").cum_sum())._lower()
    top = low.irs[root]["exprs"][0]
    for field, value, word in (("op", 4, "no plx_cum_op"), ("op", -1, "no plx_cum_op"), ("lit", 2, "reverse rides in lit.u"), ("lhs", -1, "needs an operand")):
        saved = low.aexprs[top][field]
        low.aexprs[top][field] = value
        rc, msg = import_error(low, root)
        assert rc == ERR_INVALID and word in msg, (field, value, msg)
        low.aexprs[top][field] = saved
    low, root, _ = df.lazy().select(c("x").rank("min"))._lower()
    top = low.irs[root]["exprs"][0]
    for field, value, word in (("op", 5, "no plx_rank_method"), ("lit", 7, "descending rides in lit.u"), ("lhs", -1, "needs an operand")):
        saved = low.aexprs[top][field]
        low.aexprs[top][field] = value
        rc, msg = import_error(low, root)
        assert rc == ERR_INVALID and word in msg, (field, value, msg)
        low.aexprs[top][field] = saved
    # in the keys or the aggregate list of a group_by: PLX_ERR_INVALID naming the functions (arenas a caller other than the mirror API may send)
    low, root, _ = df.lazy().group_by("k").agg(c("x").sum())._lower()
    agg = low.irs[root]["exprs"][0]
    low.aexprs[agg]["kind"], low.aexprs[agg]["op"], low.aexprs[agg]["lit"] = F.AE_CUMULATIVE, F.CUM_SUM, 0
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "cumulative / ranking expression" in msg and "aggregate list of a group_by" in msg, msg
    low, root, _ = df.lazy().group_by(c("a").cast(pl.Int64)).agg(c("x").sum())._lower()
    key = low.irs[root]["keys"][0]
    low.aexprs[key]["kind"], low.aexprs[key]["op"], low.aexprs[key]["dtype"], low.aexprs[key]["lit"] = F.AE_RANK, F.RANK_DENSE, 0, 0
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "cumulative / ranking expression" in msg and "keys of a group_by" in msg, msg
    # nine keys around a cumulative function: the window's own limit
    low, root, _ = df.lazy().select(c("x").cum_sum().over(*["k"] * 9))._lower()
    rc, msg = import_error(low, root)
    assert rc == F.ERR_UNSUPPORTED and "window over 9 keys" in msg and "1..8" in msg, msg


def test_fused_pipelines_decline_by_name(df):
    for lf in (df.lazy().select(c("x").cum_sum()), df.lazy().select(c("x").rank("dense").over("k")), df.lazy().select((c("x") - c("x").cum_max().over("k")).sum()),
               df.lazy().filter(c("x").rank("ordinal").over("k") <= 3).select(c("x").sum()), df.lazy().filter(c("x").cum_sum() > 1.0).group_by("k").agg(c("x").sum())):
        fused, _, why, _ = lf.describe_fusion()
        assert not fused and why == REASON, why
    fused, _, why, _ = df.lazy().select(c("x").sum().over("k")).describe_fusion()              # a window of an aggregate keeps its own reason
    assert not fused and why == "window expression: per-node route", why
    fused, _, why, _ = df.lazy().filter(c("x") > 0).select(c("x").sum()).describe_fusion()      # the same query without one still fuses
    assert fused, why


# ---- explain() and the pushdown rules ---------------------------------------------------------------------------------------------------------------------
def test_explain_lines(df):
    text = df.lazy().with_columns(c("x").cum_sum().alias("s"), (c("a") * c("a")).cum_max(reverse=True).over("k", "k2").alias("m")).filter(
        c("x").rank("ordinal", descending=True).alias("r").over("k") <= 3).explain()
    assert "Cumulative[col('x').cum_sum() over the whole column] in with_columns" in text, text
    assert f"Cumulative[{(c('a') * c('a'))!r}.cum_max(reverse=True) over [col('k'), col('k2')]] in with_columns" in text, text
    assert "Rank[col('x').rank('ordinal', descending=True) over [col('k')]] in filter" in text, text
    assert "Window[" not in text                                                                # a window of one of these is its line, not a window line ...
    text = df.lazy().select(c("x").sum().over("k"), c("x").cum_count()).explain()
    assert "Window[col('x').agg0() over [col('k')]" in text and "Cumulative[col('x').cum_count() over the whole column] in select" in text, text


def test_no_predicate_and_no_slice_is_pushed_through(tmp_path):
    """A cumulative or ranking expression reads every row of its input.  The simple conjuncts of a filter that holds one, and of the filters above it, must not reach
    the scan (row groups dropped by statistics would change the running values); a filter BELOW it still prunes.  A slice stops at a node that holds one."""
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
    for pred in (c("x").cum_sum() > 100.0, c("x").rank("ordinal", descending=True).over("k") <= 3, c("x").cum_count().over("k") > 2):
        for lf in (pl.scan_parquet(path).filter((c("y") > 2500) & pred), pl.scan_parquet(path).filter(pred).filter(c("y") > 2500),
                   pl.scan_parquet(path).filter(pred).filter(c("y") > 2500).filter(c("y") < 4000).select("x")):
            src = scan_of(lf)
            assert src._preds == [] and len(src.selected_row_groups()) == 10, src._preds
            assert "STATISTICS PRUNING" not in lf.explain(), lf.explain()
            assert {"x", "y"} <= set(src.selected_columns())
        lf = pl.scan_parquet(path).filter(c("y") > 2500).filter(pred & (c("y") < 4000))          # below it the rows never reach it: pruned as before
        src = scan_of(lf)
        assert src._preds == [("y", F.OP_GT, 2500)] and len(src.selected_row_groups()) == 5
    src = scan_of(pl.scan_parquet(path).with_columns(c("x").cum_sum().alias("s")).filter(c("y") > 2500))
    assert src._preds == [] and len(src.selected_row_groups()) == 10
    # slices: through a row-preserving node as before, never through a node that holds a cumulative / ranking expression
    assert io.scan_under(pl.scan_parquet(path).with_columns((c("x") * 2).alias("z"))._node) is not None
    for node_lf in (pl.scan_parquet(path).with_columns(c("x").cum_sum().alias("s")), pl.scan_parquet(path).select(c("x").rank("min")),
                    pl.scan_parquet(path).select(c("x"), c("y").cum_max().over("k").alias("m"))):
        assert io.scan_under(node_lf._node) is None
        src = scan_of(node_lf.slice(1000, 10))
        assert len(src.selected_row_groups()) == 10, "a slice above a running value was pushed into the scan"
    src = scan_of(pl.scan_parquet(path).with_columns((c("x") * 2).alias("z")).slice(1000, 10))
    assert len(src.selected_row_groups()) == 1


# ---- the plugin symbols and the C entries without a device ---------------------------------------------------------------------------------------------------
def test_plugin_fields_and_entry_points_without_a_device():
    import pyarrow as pa
    import torch

    from tests import plugin_abi as P
    for op, t, want in (("sum", pa.int8(), pa.int64()), ("sum", pa.uint16(), pa.int64()), ("sum", pa.bool_(), pa.uint32()), ("sum", pa.float32(), pa.float32()),
                        ("sum", pa.uint64(), pa.uint64()), ("min", pa.int16(), pa.int16()), ("max", pa.float32(), pa.float32()), ("max", pa.bool_(), pa.bool_()),
                        ("count", pa.float64(), pa.uint32()), ("count", pa.bool_(), pa.uint32())):
        assert P.field("plx_cum", t, {"op": op}).type == want, (op, t)
    assert P.field("plx_cum", pa.float64(), {"op": "sum", "reverse": True}, col_name="x").name == "x"
    assert P.field("plx_cum", pa.float64(), {"op": "prod"}) is None and "kwargs must carry op in {sum, min, max, count}" in P.last_error()
    assert P.field("plx_cum", pa.float64(), {}) is None and "kwargs must carry op" in P.last_error()
    for method in ("min", "max", "dense", "ordinal"):
        assert P.field("plx_rank", pa.float32(), {"method": method}).type == pa.uint32(), method
    assert P.field("plx_rank", pa.float32(), {"method": "average", "descending": True}).type == pa.float64()
    assert P.field("plx_rank", pa.int64(), {"method": "average"}, col_name="v").name == "v"
    assert P.field("plx_rank", pa.int64(), {"method": "random"}) is None and "kwargs must carry method in {average, min, max, dense, ordinal}" in P.last_error()
    # what the window plugin keeps refusing
    assert P.field("plx_window_agg", pa.float64(), {"agg": "cum_sum"}) is None and "kwargs must carry agg" in P.last_error()
    if torch.cuda.is_available():
        return
    res, inp = P.call("plx_cum", [pa.array([1.0, 2.0]), pa.array([1, 1])], {"op": "sum"})
    assert res is None and inp.released == 2 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    res, inp = P.call("plx_rank", [pa.array([1.0, 2.0])], {"method": "min"})
    assert res is None and inp.released == 1 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    # the parameters are refused by name before anything runs
    h = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.I64, 100, 0, 0, 0, 0, C.byref(h)) == 0
    keys, out = (C.c_uint64 * 9)(*([h.value] * 9)), C.c_uint64()
    err = lambda: F.lib().plx_last_error().decode()
    assert F.lib().plx_cumulative(keys, 1, h.value, 4, 0, C.byref(out)) == 1 and "no plx_cum_op" in err()
    assert F.lib().plx_cumulative(keys, 1, h.value, F.CUM_SUM, 3, C.byref(out)) == 1 and "reverse must be 0 or 1" in err()
    assert F.lib().plx_cumulative(keys, 9, h.value, F.CUM_SUM, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in err()
    assert F.lib().plx_cumulative(None, 2, h.value, F.CUM_SUM, 0, C.byref(out)) == 1 and "n_keys" in err()
    assert F.lib().plx_rank(keys, 1, h.value, 5, 0, C.byref(out)) == 1 and "no plx_rank_method" in err()
    assert F.lib().plx_rank(keys, 1, h.value, F.RANK_MIN, 2, C.byref(out)) == 1 and "descending must be 0 or 1" in err()
    assert F.lib().plx_rank(keys, 9, h.value, F.RANK_MIN, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 keys" in err()
    short = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.I64, 99, 0, 0, 0, 0, C.byref(short)) == 0
    assert F.lib().plx_rank((C.c_uint64 * 1)(short.value), 1, h.value, F.RANK_MIN, 0, C.byref(out)) != 0 and "key length mismatch" in err()


def test_the_example_queries_lower():
    from polars_amd import queries as QQ
    rng = np.random.default_rng(12)
    n = 2000
    cols = {"l_returnflag": (rng.integers(0, 3, n).astype(np.uint8), None), "l_linestatus": (rng.integers(0, 2, n).astype(np.uint8), None),
            "l_discount": (rng.integers(0, 11, n) / 100.0, None), "l_extendedprice": (rng.uniform(900.0, 100000.0, n), None)}
    low, root, schema = QQ.running_revenue_by_flag(frame_like(cols).lazy())._lower()
    assert schema["running_revenue"] == pl.Float64 and low.irs[root]["kind"] == F.IR_HSTACK
    cum = [d for d in low.aexprs if d["kind"] == F.AE_CUMULATIVE]
    assert len(cum) == 1 and cum[0]["op"] == F.CUM_SUM and low.aexprs[cum[0]["lhs"]]["kind"] == F.AE_BINARY and sum(d["kind"] == F.AE_WINDOW_KEY for d in low.aexprs) == 2
    low, root, schema = QQ.top3_price_per_flag(frame_like(cols).lazy())._lower()
    assert low.irs[root]["kind"] == F.IR_FILTER and list(schema) == list(cols)
    rk = [d for d in low.aexprs if d["kind"] == F.AE_RANK]
    assert len(rk) == 1 and (rk[0]["op"], rk[0]["lit"]) == (F.RANK_ORDINAL, 1)


# ---- the new kernels' registers ------------------------------------------------------------------------------------------------------------
def test_cumulative_kernels_stream_without_scratch():
    """every form of cum_reduce_kernel / cum_scan_kernel and rank_kernel: no scratch (the eight positions of a lane stay in registers), VGPRs below the bound that
    keeps five waves per SIMD, as tests/test_kernel_resources_cpu.py obtains them."""
    from tests.test_kernel_resources_cpu import resource_usage
    res = {n: r for n, r in resource_usage("kernels_cumulative.hip").items() if any(w in n for w in ("cum_reduce_kernel", "cum_scan_kernel", "rank_kernel"))}
    assert len(res) > 100 and any("rank_kernel" in n for n in res), len(res)
    for name, r in sorted(res.items()):
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 96, (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 64, (name, r)          # the four wave totals


# ---- the visitor's function nodes through the engine shim ------------------------------------------------------------------------------------------
def test_polars_engine_maps_the_function_nodes(df):
    """A stand-in NodeTraverser shows PLX_AE_CUMULATIVE / PLX_AE_RANK as the visitor's Function node (input, function_data = (name, arguments...), options): the shim
    builds the same arenas back, plain and under a Window node; another function and another method are refused by name."""
    from polars_amd import polars_engine as eng
    from tests import test_polars_engine_cpu as S

    class Node:
        def __init__(self, **kw): self.__dict__.update(kw)

    class Mapping:
        kind = "groups_to_rows"

    CUM = {F.CUM_SUM: "cum_sum", F.CUM_MIN: "cum_min", F.CUM_MAX: "cum_max", F.CUM_COUNT: "cum_count"}
    METHOD = {v: k for k, v in F.RANK_METHODS.items()}

    class WithFunctions(S.FakeTraverser):
        rename = {}

        def view_expression(self, i):
            d = self.low.aexprs[i]
            if d["kind"] == F.AE_WINDOW:
                keys, link = [], d["rhs"]
                while link >= 0:
                    keys.append(self.low.aexprs[link]["lhs"])
                    link = self.low.aexprs[link]["rhs"]
                return type("Window", (Node,), {})(function=d["lhs"], partition_by=keys, order_by=None, options=Mapping())
            if d["kind"] == F.AE_CUMULATIVE:
                name = CUM[d["op"]]
                return type("Function", (Node,), {})(input=[d["lhs"]], function_data=(self.rename.get(name, name), bool(d["lit"])), options=None)
            if d["kind"] == F.AE_RANK:
                return type("Function", (Node,), {})(input=[d["lhs"]], function_data=("rank", self.rename.get(METHOD[d["op"]], METHOD[d["op"]]), bool(d["lit"]), None), options=None)
            return super().view_expression(i)

    lf = df.lazy().with_columns(c("x").cum_sum().alias("s"), c("a").cum_max(reverse=True).over("k", "k2").alias("m"), c("x").cum_count().alias("n"),
                                c("x").rank("dense").alias("r")).filter(c("x").rank("ordinal", descending=True).over("k") <= 3)
    low, root, _ = lf._lower()
    back = eng.Translator(WithFunctions(low, root), frame_of=lambda node: node.df).plan()
    low2, root2, _ = back._lower()
    assert S.canonical(low, root) == S.canonical(low2, root2)
    params = lambda lw: sorted((d["kind"], d["op"], d["lit"]) for d in lw.aexprs if d["kind"] in (F.AE_CUMULATIVE, F.AE_RANK))
    assert params(low) == params(low2) == [(16, F.CUM_SUM, 0), (16, F.CUM_MAX, 1), (16, F.CUM_COUNT, 0), (17, F.RANK_DENSE, 0), (17, F.RANK_ORDINAL, 1)]
    for rename, word in (({"cum_sum": "cum_prod"}, "function cum_prod"), ({"dense": "random"}, "rank with method random"), ({"cum_count": "shift"}, "function shift")):
        nt = WithFunctions(low, root)
        nt.rename = rename
        with pytest.raises(eng.NotSupported, match=word):
            eng.Translator(nt, frame_of=lambda node: node.df).plan()
