"""n_unique / unique() without a GPU: the arithmetic of csrc/distinct.hpp as a stand-alone program under -fsanitize=address,undefined against brute force; the
numpy reference's own check (against pandas where it is installed); the mirror API and its lowering (aggregate kind 10, the Distinct node of kind 8 with the keep
strategy in the `how` slot); the header's numbering and prototypes; the exported symbols; the plugin field; the fused compiler declining by name; the example
query; the registers of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import distinct_ref as D
from tests.test_program_eval_cpu import frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
REASON = "n_unique: a distinct count (sorted-segment route)"
Q_REASON = "median / quantile: an order statistic (sorted-segment route)"


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_under_sanitizers_against_brute_force(tmp_path):
    """tests/emu/distinct_main.cpp: rank_before at every position of masks of 0, 1, 63, 64, 65 and 4097 bits (heads at the word boundaries among them), segment
    counts as differences of ranks, keep_row for the four strategies over stable sorted classes, the keep check, the bitmap bound."""
    exe = str(tmp_path / "distinct_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "distinct_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 150_000, r.stdout


def test_the_reference():
    nan2 = np.array([0x7FF8000000000001, 0xFFF8000000000000], np.uint64).view(np.float64)
    assert D.n_unique(np.array([])) == 0 and D.n_unique(np.array([0.0, -0.0])) == 1 and D.n_unique(nan2) == 1 and D.n_unique(np.array([1, 1]), np.array([True, False])) == 2
    assert D.n_unique(np.array([(1 << 63) - 1, (1 << 63) - 2], np.int64)) == 2 and D.n_unique(np.array([(1 << 64) - 1, 5], np.uint64), np.array([True, False])) == 2
    k = (np.array([3, 1, 3, 2, 1, 3]), None)
    assert D.unique_rows([k], "first") == [0, 1, 3] == D.unique_rows([k], "any") and D.unique_rows([k], "last") == [3, 4, 5] and D.unique_rows([k], "none") == [3]
    assert D.unique_rows([(np.array([1, 1]), np.array([True, False])), (np.array([np.nan, np.nan]), None)], "first") == [0, 1]
    done = D.self_check()
    try:
        import pandas  # noqa: F401
        assert done == 7 * 14
    except ImportError:
        assert done == 0


# ---- the mirror API and its lowering ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def df():
    rng = np.random.default_rng(416)
    n = 301
    cols = {"k": (rng.integers(0, 7, n).astype(np.int64), None), "x": (rng.normal(3.0, 2.0, n), None), "a": (rng.integers(-300, 300, n).astype(np.int64), None),
            "b": (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) < 0.9), "f": (rng.normal(size=n).astype(np.float32), None), "flag": (rng.random(n) < 0.5, None),
            "d": (rng.integers(8000, 11000, n).astype(np.int32), None), "t": (rng.integers(0, 1 << 40, n).astype(np.int64), None), "s": (rng.integers(0, 3, n).astype(np.uint8), None)}
    return frame_like(cols, {"d": pl.Date, "t": pl.Datetime, "s": pl.Categorical(["A", "N", "R"], pl.UInt8), "f": pl.Float32})


def lowered(df, expr):
    low, root, schema = df.lazy().select(expr)._lower()
    return low, low.aexprs[low.irs[root]["exprs"][0]], schema


def test_expr_and_frame_api_and_the_keep_check(df):
    assert repr(c("x").n_unique()) == "col('x').n_unique()" == repr(pl.n_unique("x"))
    e = c("x").n_unique()
    assert (e.kind, e.op, e.value) == ("agg", F.AGG_N_UNIQUE, None) and F.AGG_N_UNIQUE == 10 and F.IR_DISTINCT == 8
    assert F.UNIQUE_KEEPS == {"any": 0, "first": 1, "last": 2, "none": 3}
    for name in ("n_unique", "unique"):
        assert hasattr(pl.Series, name), name
    assert hasattr(pl.GroupBy, "n_unique") and hasattr(pl.DataFrame, "unique") and hasattr(pl.LazyFrame, "unique") and "n_unique" in pl.__all__
    for bad in ("some", "First", "", None, 1):
        with pytest.raises(ValueError, match="keep must be one of"):
            df.lazy().unique(keep=bad)
    for bad in ([], [1], 3):
        with pytest.raises((ValueError, TypeError)):
            df.lazy().unique(bad)
    with pytest.raises(KeyError, match="column not found: zz"):
        df.lazy().unique(["k", "zz"])._lower()


def test_arena_node_op_10_for_every_dtype(df):
    for col in ("x", "a", "b", "f", "flag", "d", "t", "s"):          # no dtype is refused
        low, top, schema = lowered(df, c(col).n_unique())
        assert list(schema.items()) == [(col, pl.UInt32)]
        assert (top["kind"], top["op"], top["lit"], top["dtype"]) == (F.AE_AGG, F.AGG_N_UNIQUE, None, 0) and low.aexprs[top["lhs"]]["kind"] == F.AE_COLUMN
    low, top, schema = lowered(df, (c("a") * c("b")).n_unique().alias("ab"))
    assert schema == {"ab": pl.UInt32} and low.aexprs[top["lhs"]]["op"] == F.AGG_N_UNIQUE and low.aexprs[low.aexprs[top["lhs"]]["lhs"]]["kind"] == F.AE_BINARY
    low, root, schema = df.lazy().group_by("k").agg(c("x").median().alias("m"), c("x").n_unique().alias("nu"), c("x").mean().alias("avg"))._lower()
    assert schema == {"k": pl.Int64, "m": pl.Float64, "nu": pl.UInt32, "avg": pl.Float64}
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert [ae[i].op for i, d in enumerate(low.aexprs) if d["kind"] == F.AE_AGG] == [F.AGG_QUANTILE, 10, F.AGG_MEAN]
    assert C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr._fields_[-1][0] == "cond"      # plx_aexpr is what it was


def test_distinct_node_kind_8_keep_in_how(df):
    size = C.sizeof(F.IR)
    for keep, code in F.UNIQUE_KEEPS.items():
        for subset, names in ((None, list(df.schema)), ("k", ["k"]), (["a", "flag"], ["a", "flag"])):
            for mo in (False, True):
                low, root, schema = df.lazy().unique(subset, keep=keep, maintain_order=mo)._lower()
                node = low.irs[root]
                assert (node["kind"], node["how"], node["maintain_order"], node["exprs"]) == (8, code, int(mo), []) and schema == df.schema
                assert [(low.aexprs[i]["kind"], low.aexprs[i]["name"]) for i in node["keys"]] == [(F.AE_COLUMN, nm) for nm in names]
                ir, n_ir, ae, n_ae, keepalive = low.to_c()
                assert (ir[root].kind, ir[root].how, ir[root].n_keys, ir[root].maintain_order) == (F.IR_DISTINCT, code, len(names), int(mo))
    assert C.sizeof(F.IR) == size
    assert df.lazy().unique("k").explain().splitlines()[-1] == "Distinct[subset=[k], keep=first (asked: any), order=rows]"
    assert "Distinct[subset=all columns, keep=none, order=rows]" in df.lazy().filter(c("a") > 0).unique(keep="none").select("k").explain()
    assert df.lazy().unique("k").select("x").collect_schema() == {"x": pl.Float64}
    # the engine checks the node when the arena is imported: an unknown keep is PLX_ERR_INVALID, nine subset columns PLX_ERR_UNSUPPORTED naming the limit
    buf = C.create_string_buffer(1 << 14)
    low, root, _ = df.lazy().unique("k")._lower()
    low.irs[root]["how"] = 4
    ir, n_ir, ae, n_ae, keepalive = low.to_c()
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) == 1 and "plx_unique_keep" in F.lib().plx_last_error().decode()
    low, root, _ = df.lazy().unique()._lower()
    assert len(low.irs[root]["keys"]) == 9
    ir, n_ir, ae, n_ae, keepalive = low.to_c()
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) == F.ERR_UNSUPPORTED and "subset of 9 columns" in F.lib().plx_last_error().decode()


def test_the_header_numbering_and_the_exported_symbols(tmp_path):
    src = tmp_path / "distinct.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AGG_N_UNIQUE == 10 && PLX_IR_DISTINCT == 8 && sizeof(plx_aexpr) == 48, "numbering; plx_aexpr did not grow");
_Static_assert(PLX_AGG_QUANTILE == 9 && PLX_IR_SLICE == 7, "the kinds before are where they were");
_Static_assert(PLX_UNIQUE_ANY == 0 && PLX_UNIQUE_FIRST == 1 && PLX_UNIQUE_LAST == 2 && PLX_UNIQUE_NONE == 3, "plx_unique_keep numbering");
int (*p1)(plx_column, uint32_t*) = plx_reduce_n_unique;
int (*p2)(const plx_column*, int32_t, int32_t, plx_column*) = plx_distinct_mask;
void (*p3)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_n_unique;
void (*p4)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_n_unique;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "distinct.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("plx_reduce_n_unique", "plx_distinct_mask", "_polars_plugin_plx_n_unique", "_polars_plugin_field_plx_n_unique"):
        assert hasattr(F.lib(), name), name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(w in text for w in ("plx_n_unique", "plx_reduce_n_unique", "plx_distinct_mask"))


def test_plugin_field_and_entry_points_without_a_device():
    import pyarrow as pa
    import torch

    from tests import plugin_abi as P
    for t in (pa.int32(), pa.float32(), pa.float64(), pa.bool_(), pa.uint64()):
        assert P.field("plx_n_unique", t).type == pa.uint32()
    assert P.field("plx_n_unique", pa.float64(), col_name="x").name == "x"
    if torch.cuda.is_available():
        return
    res, inp = P.call("plx_n_unique", [pa.array([1.0, 2.0])], {})
    assert res is None and inp.released == 1 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    h = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.F64, 100, 0, 0, 0, 0, C.byref(h)) == 0
    v, dt, ok = F.Scalar(), C.c_int32(), C.c_int32()
    assert F.lib().plx_reduce(F.AGG_N_UNIQUE, h.value, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "plx_reduce_n_unique" in F.lib().plx_last_error().decode()
    keys, out = (C.c_uint64 * 9)(*([h.value] * 9)), C.c_uint64()
    assert F.lib().plx_distinct_mask(keys, 1, 4, C.byref(out)) == 1 and "plx_unique_keep" in F.lib().plx_last_error().decode()
    assert F.lib().plx_distinct_mask(keys, 1, -1, C.byref(out)) == 1
    assert F.lib().plx_distinct_mask(keys, 9, 0, C.byref(out)) == F.ERR_UNSUPPORTED and "1..8 columns, got 9" in F.lib().plx_last_error().decode()


# ---- the fused compiler declines by name ---------------------------------------------------------------------------------------------------
def test_describe_fusion_names_both_reasons(df):
    for lf in (df.lazy().group_by("k").agg(c("x").n_unique()), df.lazy().group_by("k").agg(c("x").var(), c("flag").n_unique()), df.lazy().select(c("s").n_unique()),
               df.lazy().filter(c("a") > 0).select(c("x").std(), c("d").n_unique())):
        fused, _, why, _ = lf.describe_fusion()
        assert not fused and why == REASON, why
    # a quantile in the list keeps the quantile's reason, whichever comes first
    for aggs in ((c("x").median(), c("x").n_unique()), (c("x").n_unique(), c("a").quantile(0.9, "higher"))):
        fused, _, why, _ = df.lazy().group_by("k").agg(*aggs).describe_fusion()
        assert not fused and why == Q_REASON, why
    fused, _, why, _ = df.lazy().group_by("k").agg(c("x").mean()).describe_fusion()          # the same query with a mean still fuses
    assert fused, why


def test_lineitem_distinct_lowers():
    from polars_amd import queries as QQ
    rng = np.random.default_rng(10)
    n = 2000
    cols = {"l_returnflag": (rng.integers(0, 3, n).astype(np.uint8), None), "l_linestatus": (rng.integers(0, 2, n).astype(np.uint8), None),
            "l_quantity": (rng.integers(1, 51, n).astype(np.int64), None), "l_shipdate": (rng.integers(0, 1 << 40, n).astype(np.int64), None)}
    lf = QQ.lineitem_distinct(frame_like(cols, {"l_shipdate": pl.Datetime}).lazy())
    low, root, schema = lf._lower()
    assert schema == {"l_returnflag": pl.UInt8, "l_linestatus": pl.UInt8, "n_quantities": pl.UInt32, "n_shipdates": pl.UInt32, "count_order": pl.UInt32}
    assert [d["op"] for d in low.aexprs if d["kind"] == F.AE_AGG] == [F.AGG_N_UNIQUE, F.AGG_N_UNIQUE]
    fused, _, why, _ = lf.describe_fusion()
    assert not fused and why == REASON


# ---- the new kernels' registers ------------------------------------------------------------------------------------------------------------
def test_distinct_kernels_stream_without_scratch():
    """distinct_bitmap_kernel, run_heads_count_kernel, distinct_heads_kernel, mask_word_counts_kernel, segment_distinct_kernel, distinct_keep_kernel: VGPRs and scratch
    bytes as tests/test_kernel_resources_cpu.py obtains them."""
    from tests.test_kernel_resources_cpu import resource_usage
    names = ("distinct_bitmap_kernel", "run_heads_count_kernel", "distinct_heads_kernel", "mask_word_counts_kernel", "segment_distinct_kernel", "distinct_keep_kernel")
    res = {n: r for n, r in resource_usage("kernels_sort.hip").items() if any(w in n for w in names)}
    assert len(res) == len(names), sorted(res)
    for name, r in sorted(res.items()):
        print(name, "VGPRs", r["VGPRs"], "scratch", r["ScratchSize [bytes/lane]"], "LDS", r["LDS Size [bytes/block]"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r)          # they stream: eight waves per SIMD
