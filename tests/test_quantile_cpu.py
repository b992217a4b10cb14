"""median / quantile without a GPU: the arithmetic of csrc/quantile.hpp as a stand-alone program under -fsanitize=address,undefined against a sort-and-index
computation; the numpy reference's own check against np.quantile; the mirror API and its lowering (kind 9 with q in the literal slot and the interpolation in the
dtype slot, output dtypes, the refusals); the fused compiler declining the kind by name; the sharded operators' refusal; the registers of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import dist
from tests import quantile_ref as Q
from tests.test_program_eval_cpu import frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
REASON = "median / quantile: an order statistic (sorted-segment route)"


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_under_sanitizers_against_sort_and_index(tmp_path):
    """tests/emu/quantile_main.cpp: rank_of / combine over sizes 0..70, five interpolations, six q; the value codes' round trips at the dtype edges."""
    exe = str(tmp_path / "quantile_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "quantile_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 80_000, r.stdout


def test_the_reference_against_numpy():
    """tests/quantile_ref.py on NaN-free data: lower / higher / midpoint bit-equal to np.quantile, linear within 4 * 2^-53 relative, nearest equal off the ties and
    half away from zero on them."""
    assert Q.self_check() == 720
    v = np.array([3.0, 1.0, 2.0, 4.0])
    assert Q.accept(2.5, v, 0.5, "linear") and not Q.accept(2.5000001, v, 0.5, "linear") and Q.accept(None, np.array([]), 0.5, "linear") and not Q.accept(None, v, 0.5, "linear")
    assert Q.accept(float("nan"), np.array([1.0, np.nan]), 1.0, "higher") and not Q.accept(1.0, np.array([1.0, np.nan]), 1.0, "higher")
    assert Q.accept(float(np.float32(0.1)), np.array([0.1], np.float32), 0.5, "linear", f32=True)


# ---- the mirror API and its lowering ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def df():
    rng = np.random.default_rng(415)
    n = 301
    cols = {"k": (rng.integers(0, 7, n).astype(np.int64), None), "x": (rng.normal(3.0, 2.0, n), None), "a": (rng.integers(-300, 300, n).astype(np.int64), None),
            "b": (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) < 0.9), "i": (rng.integers(-1000, 1000, n).astype(np.int32), None),
            "u": (rng.integers(0, 60000, n).astype(np.uint16), None), "f": (rng.normal(size=n).astype(np.float32), None), "flag": (rng.random(n) < 0.5, None),
            "d": (rng.integers(8000, 11000, n).astype(np.int32), None), "t": (rng.integers(0, 1 << 40, n).astype(np.int64), None), "s": (rng.integers(0, 3, n).astype(np.uint8), None)}
    return frame_like(cols, {"d": pl.Date, "t": pl.Datetime, "s": pl.Categorical(["A", "N", "R"], pl.UInt8), "f": pl.Float32})


def lowered(df, expr):
    low, root, schema = df.lazy().select(expr)._lower()
    return low, low.aexprs[low.irs[root]["exprs"][0]], schema


def test_expr_api_and_the_checks_of_q_and_interpolation():
    assert repr(c("x").median()) == "col('x').median()" and repr(pl.quantile("x", 0.25, "lower")) == "col('x').quantile(0.25, 'lower')" and repr(pl.median("x")) == "col('x').median()"
    e = c("x").quantile(0.75)
    assert (e.kind, e.op, e.value) == ("agg", F.AGG_QUANTILE, (0.75, "nearest")) and F.AGG_QUANTILE == 9
    assert c("x").median().value == (0.5, "linear") and c("x").quantile(1).value == (1.0, "nearest") and c("x").quantile(np.float32(0.5), "midpoint").value == (0.5, "midpoint")
    assert F.QUANTILE_INTERPOLATIONS == {"nearest": 0, "lower": 1, "higher": 2, "midpoint": 3, "linear": 4}
    for bad in (float("nan"), -0.01, 1.01, 2, "0.5", None, True):
        with pytest.raises(ValueError, match=r"real number in \[0, 1\]"):
            c("x").quantile(bad)
    for bad in ("equiprobable", "Linear", "", None, 4):
        with pytest.raises(ValueError, match="interpolation must be one of"):
            c("x").quantile(0.5, bad)
    assert hasattr(pl.Series, "median") and hasattr(pl.Series, "quantile") and hasattr(pl.GroupBy, "median")


def test_arena_node_q_in_the_literal_slot_interpolation_in_the_dtype_slot(df):
    for col, out in (("x", pl.Float64), ("i", pl.Float64), ("u", pl.Float64), ("a", pl.Float64), ("f", pl.Float32)):
        for it, code in F.QUANTILE_INTERPOLATIONS.items():
            low, top, schema = lowered(df, c(col).quantile(0.25, it))
            assert list(schema.items()) == [(col, out)]                         # Float64 (Float32 stays), named like the source column
            assert (top["kind"], top["op"], top["lit"], top["dtype"]) == (F.AE_AGG, F.AGG_QUANTILE, 0.25, code) and low.aexprs[top["lhs"]]["kind"] == F.AE_COLUMN
    low, top, schema = lowered(df, (c("a") * c("b")).median().alias("ab"))
    assert schema == {"ab": pl.Float64} and low.aexprs[top["lhs"]]["op"] == F.AGG_QUANTILE and low.aexprs[low.aexprs[top["lhs"]]["lhs"]]["kind"] == F.AE_BINARY
    low, root, _ = df.lazy().group_by("k").agg(c("x").median().alias("m"), c("i").quantile(1 / 3, "higher").alias("q"), c("x").mean().alias("avg"))._lower()
    ir, n_ir, ae, n_ae, keep = low.to_c()
    seen = [(ae[i].op, ae[i].lit.f64, ae[i].dtype, ae[i].cond) for i, d in enumerate(low.aexprs) if d["kind"] == F.AE_AGG and d["op"] == F.AGG_QUANTILE]
    assert seen == [(9, 0.5, F.QUANTILE_LINEAR, -1), (9, 1 / 3, F.QUANTILE_HIGHER, -1)]
    assert C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr._fields_[-1][0] == "cond"      # plx_aexpr is what it was


def test_refusals_name_the_dtype(df):
    for col, name in (("flag", "Boolean"), ("d", "Date"), ("t", "Datetime"), ("s", "Categorical")):
        with pytest.raises(TypeError, match=f"median\\(\\) needs a numeric expression, got {name}"):
            lowered(df, c(col).median())
        with pytest.raises(TypeError, match=f"quantile\\(\\) needs a numeric expression, got {name}"):
            lowered(df, c(col).quantile(0.1))
    with pytest.raises(TypeError, match="Boolean"):
        df.lazy().group_by("k").agg((c("x") > 0).median())._lower()
    # the engine itself: q and the interpolation are checked when the arena is imported; a Boolean operand reaches the fused compiler, which declines the kind
    # before it looks at operands (the per-node evaluator then refuses the dtype: PLX_ERR_UNSUPPORTED, tests/test_gpu_quantile.py)
    buf = C.create_string_buffer(1 << 14)
    for field, value, word in (("lit", 1.5, "q in [0, 1]"), ("lit", float("nan"), "q in [0, 1]"), ("dtype", 5, "plx_quantile_interpolation"), ("dtype", -1, "plx_quantile_interpolation")):
        low, root, _ = df.lazy().select(c("x").median())._lower()
        [d for d in low.aexprs if d["kind"] == F.AE_AGG][0][field] = value
        ir, n_ir, ae, n_ae, keep = low.to_c()
        assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) == 1 and word in F.lib().plx_last_error().decode(), F.lib().plx_last_error().decode()
    low, root, _ = df.lazy().select(c("flag").sum())._lower()
    agg = [d for d in low.aexprs if d["kind"] == F.AE_AGG][0]
    agg["op"], agg["lit"], agg["dtype"] = F.AGG_QUANTILE, 0.5, F.QUANTILE_LINEAR
    ir, n_ir, ae, n_ae, keep = low.to_c()
    fus, sid, why = C.c_int32(), C.c_int32(), C.create_string_buffer(512)
    assert F.lib().plx_describe_fusion(ir, n_ir, ae, n_ae, root, C.byref(fus), C.byref(sid), why, len(why)) == 0 and fus.value == 0 and why.value.decode() == REASON


def test_the_header_numbering_and_the_exported_symbols(tmp_path):
    src = tmp_path / "quantile.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AGG_FIRST == 6 && PLX_AGG_VAR == 7 && PLX_AGG_STD == 8 && PLX_AGG_QUANTILE == 9, "plx_agg_op numbering");
_Static_assert(PLX_QUANTILE_NEAREST == 0 && PLX_QUANTILE_LOWER == 1 && PLX_QUANTILE_HIGHER == 2 && PLX_QUANTILE_MIDPOINT == 3 && PLX_QUANTILE_LINEAR == 4, "plx_quantile_interpolation numbering");
_Static_assert(sizeof(plx_aexpr) == 48, "plx_aexpr did not grow");
int (*p1)(plx_column, double, int32_t, plx_scalar*, plx_dtype*, int32_t*) = plx_reduce_quantile;
int (*p2)(const plx_column*, int32_t, const plx_column*, const plx_agg_op*, int32_t, int32_t, const int32_t*, const double*, const int32_t*, plx_column*, plx_column*) = plx_groupby_agg_params;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "quantile.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("plx_reduce_quantile", "plx_groupby_agg_params", "_polars_plugin_plx_median", "_polars_plugin_field_plx_median"):
        assert hasattr(F.lib(), name), name
    assert not hasattr(F.lib(), "_polars_plugin_plx_quantile")          # float kwargs: not part of this
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(w in text for w in ("plx_median", "plx_reduce_quantile", "plx_groupby_agg_params"))


def test_plugin_field_and_entry_points_without_a_device():
    import pyarrow as pa
    import torch

    from tests import plugin_abi as P
    assert P.field("plx_median", pa.int32()).type == pa.float64() and P.field("plx_median", pa.float32()).type == pa.float32() and P.field("plx_median", pa.float64(), col_name="x").name == "x"
    if torch.cuda.is_available():
        return
    res, inp = P.call("plx_median", [pa.array([1.0, 2.0])], {})
    assert res is None and inp.released == 1 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    h, hb = C.c_uint64(), C.c_uint64()
    assert F.lib().plx_column_placeholder(F.F64, 100, 0, 0, 0, 0, C.byref(h)) == 0 and F.lib().plx_column_placeholder(F.BOOL, 100, 0, 0, 0, 0, C.byref(hb)) == 0
    v, dt, ok = F.Scalar(), C.c_int32(), C.c_int32()
    out = (v, dt, ok)
    refs = [C.byref(x) for x in out]
    assert F.lib().plx_reduce(F.AGG_QUANTILE, h.value, *refs) == 1 and "plx_reduce_quantile" in F.lib().plx_last_error().decode()
    for q in (float("nan"), -0.5, 1.5):
        assert F.lib().plx_reduce_quantile(h.value, q, F.QUANTILE_LINEAR, *refs) == 1 and "[0, 1]" in F.lib().plx_last_error().decode()
    assert F.lib().plx_reduce_quantile(h.value, 0.5, 5, *refs) == 1 and "interpolation" in F.lib().plx_last_error().decode()
    assert F.lib().plx_reduce_quantile(hb.value, 0.5, F.QUANTILE_LINEAR, *refs) == F.ERR_UNSUPPORTED and "bool" in F.lib().plx_last_error().decode().lower()
    keys, vals, aggs = (C.c_uint64 * 1)(h.value), (C.c_uint64 * 1)(h.value), (C.c_int32 * 1)(F.AGG_QUANTILE)
    ok_, oa_ = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    assert F.lib().plx_groupby_agg_ddof(keys, 1, vals, aggs, 1, 0, None, ok_, oa_) == 1 and "plx_groupby_agg_params" in F.lib().plx_last_error().decode()
    assert F.lib().plx_groupby_agg(keys, 1, vals, aggs, 1, 0, ok_, oa_) == 1 and "plx_groupby_agg_params" in F.lib().plx_last_error().decode()
    qs = (C.c_double * 1)(1.5)
    assert F.lib().plx_groupby_agg_params(keys, 1, vals, aggs, 1, 0, None, qs, None, ok_, oa_) == 1 and "[0, 1]" in F.lib().plx_last_error().decode()
    vb = (C.c_uint64 * 1)(hb.value)
    assert F.lib().plx_groupby_agg_params(keys, 1, vb, aggs, 1, 0, None, None, None, ok_, oa_) == F.ERR_UNSUPPORTED and "bool" in F.lib().plx_last_error().decode().lower()


# ---- the fused compiler declines by name ---------------------------------------------------------------------------------------------------
def describe(lf):
    return lf.describe_fusion()


def test_describe_fusion_names_the_sorted_segment_route(df):
    fused, _, why, _ = describe(df.lazy().group_by("k").agg(c("x").median()))
    assert not fused and why == REASON
    # beside a var: declined before the pivot pre-pass, by the same reason; and a whole-column select
    for lf in (df.lazy().group_by("k").agg(c("x").var(), c("x").quantile(0.9, "higher")), df.lazy().select(c("x").median()), df.lazy().filter(c("i") > 0).select(c("x").std(), c("a").quantile(0.5))):
        fused, _, why, _ = describe(lf)
        assert not fused and why == REASON, why
    fused, _, why, _ = describe(df.lazy().group_by("k").agg(c("x").mean()))          # the same query without the order statistic still fuses
    assert fused, why


def test_h2o_median_sd_lowers():
    from polars_amd import queries as QQ
    rng = np.random.default_rng(9)
    n = 2000
    cols = {"id4": (rng.integers(1, 9, n).astype(np.int32), None), "id5": (rng.integers(1, 5, n).astype(np.int32), None), "v3": (rng.uniform(0, 100, n), None)}
    lf = QQ.h2o_median_sd(frame_like(cols).lazy())
    low, root, schema = lf._lower()
    assert schema == {"id4": pl.Int32, "id5": pl.Int32, "v3_median": pl.Float64, "v3_sd": pl.Float64}
    aggs = [(d["op"], d["lit"], d["dtype"]) for d in low.aexprs if d["kind"] == F.AE_AGG]
    assert aggs == [(F.AGG_QUANTILE, 0.5, F.QUANTILE_LINEAR), (F.AGG_STD, 1, 0)]
    fused, _, why, _ = describe(lf)
    assert not fused and why == REASON


def test_sharded_group_by_refuses_by_name():
    """dist.py refuses unknown aggregates by name: `median` and `quantile` get that ValueError, not a KeyError.  (This passes without the feature: dist.py is not
    changed by it.)"""
    for op in ("median", "quantile"):
        with pytest.raises(ValueError, match=op):
            dist.GroupBySpec("k", [("o", "v", op)])
        with pytest.raises(ValueError, match=op):
            dist.JoinGroupBySpec("pk", "bk", "pk", [("o", op)])


# ---- the new kernels' registers ------------------------------------------------------------------------------------------------------------
def test_quantile_kernels_use_no_scratch():
    """select_first_kernel, select_next_kernel, segment_heads_kernel, segment_quantile_kernel, invert_permutation_kernel: VGPRs and scratch bytes as
    tests/test_kernel_resources_cpu.py obtains them."""
    from tests.test_kernel_resources_cpu import resource_usage
    names = ("select_first_kernel", "select_next_kernel", "segment_heads_kernel", "segment_quantile_kernel", "invert_permutation_kernel")
    res = {n: r for n, r in resource_usage("kernels_sort.hip").items() if any(w in n for w in names)}
    assert len(res) == len(names), sorted(res)
    for name, r in sorted(res.items()):
        print(name, "VGPRs", r["VGPRs"], "scratch", r["ScratchSize [bytes/lane]"], "LDS", r["LDS Size [bytes/block]"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r)          # eight waves per SIMD: they stream, nothing is kept
