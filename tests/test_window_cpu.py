"""Window expressions (`f.over(keys)`) without a GPU: the arithmetic of csrc/window.hpp as a stand-alone program under -fsanitize=address,undefined against a brute-force
map; the numpy reference's own check; Expr.over's argument validation and repr; the lowering to PLX_AE_WINDOW = 14 with its chain of PLX_AE_WINDOW_KEY = 15 links; the
header's numbering, plx_aexpr's size and the prototypes through a compiled C caller; what plan import refuses; the fused compiler declining by name; the plugin field;
the example query; the registers of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import window_ref as W
from tests.test_program_eval_cpu import frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
REASON = "window expression: per-node route"


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_under_sanitizers_against_brute_force(tmp_path):
    """tests/emu/window_main.cpp: 0, 1, 63, 64, 65 and 129 rows, one to three key parts with and without null parts; slot_store / row_code against a brute-force map with
    a slot table of exactly R entries; sorted_group over a head mask and prefix of exact size; the broadcast's per-lane body wave by wave for every output width;
    the rule at its bound and one beyond it."""
    exe = str(tmp_path / "window_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "window_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 100_000, r.stdout


def test_the_reference():
    assert W.self_check() == 6
    x = np.array([3, 1, 2, 5], np.int64)
    want, ids = W.over([(np.array([7, 7, 8, 8]), None)], x, None, "quantile", q=0.5, interpolation="lower")
    assert want == [1.0, 1.0, 2.0, 2.0] and ids.tolist() == [0, 0, 1, 1]
    want, _ = W.over([(np.array([True, False, True]), None)], np.array([1.0, np.nan, 1.0]), None, "n_unique")
    assert want == [1, 1, 1]
    want, _ = W.over([(np.array([0, 0, 0]), None)], np.array([True, False, True]), np.array([True, True, False]), "sum")
    assert want == [1, 1, 1]


# ---- the mirror API ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def df():
    rng = np.random.default_rng(417)
    n = 301
    cols = {"k": (rng.integers(0, 7, n).astype(np.int64), None), "k2": (rng.integers(0, 3, n).astype(np.int32), rng.random(n) < 0.9), "x": (rng.normal(3.0, 2.0, n), None),
            "a": (rng.integers(-300, 300, n).astype(np.int8), None), "f": (rng.normal(size=n).astype(np.float32), None), "flag": (rng.random(n) < 0.5, None),
            "d": (rng.integers(8000, 11000, n).astype(np.int32), None), "s": (rng.integers(0, 3, n).astype(np.uint8), None)}
    return frame_like(cols, {"d": pl.Date, "s": pl.Categorical(["A", "N", "R"], pl.UInt8), "f": pl.Float32})


def test_over_arguments_and_repr():
    e = c("x").sum().over("k")
    assert e.kind == "window" and e.lhs.kind == "agg" and [k.name for k in e.value] == ["k"] and e.children()[-1] is e.value[0]
    assert repr(e) == repr(c("x").sum()) + ".over([col('k')])"                          # "<f>.over([k, ...])"
    assert repr(c("x").median().over("k", c("d").dt.month())) == "col('x').median().over([col('k'), col('d').dt.month()])"
    assert repr(c("x").sum().over(["k", "k2"])) == repr(c("x").sum().over("k", "k2")) == repr(c("x").sum().over(("k", c("k2"))))
    assert repr((c("x").sum() / pl.len()).over("k").alias("m")).endswith(".over([col('k')]).alias('m')")
    assert pl.len().over("k").kind == "window"
    for strategy in ("join", "explode", "groups_to_rows", None):
        with pytest.raises(ValueError, match="mapping_strategy"):
            c("x").sum().over("k", mapping_strategy=strategy)
    with pytest.raises(ValueError, match="order_by"):
        c("x").sum().over("k", order_by="x")
    for empty in ((), ([],)):
        with pytest.raises(ValueError, match="at least one partition key"):
            c("x").sum().over(*empty)
    for bad in (3, None, 2.5):
        with pytest.raises(TypeError, match="partition key"):
            c("x").sum().over("k", bad)
    assert c("x").sum().over("k", mapping_strategy="group_to_rows", order_by=None).kind == "window"


def test_lowering_window_node_and_key_chain(df):
    low, root, schema = df.lazy().select(c("x").sum().over("k", "k2", c("d").dt.month()))._lower()
    assert schema == {"x": pl.Float64}
    top = low.aexprs[low.irs[root]["exprs"][0]]
    assert top["kind"] == F.AE_WINDOW == 14 and F.AE_WINDOW_KEY == 15
    f = low.aexprs[top["lhs"]]
    assert (f["kind"], f["op"]) == (F.AE_AGG, F.AGG_SUM)
    chain, link = [], top["rhs"]
    while link >= 0:
        node = low.aexprs[link]
        assert node["kind"] == F.AE_WINDOW_KEY and node["lhs"] < link and node["rhs"] < link      # topological
        chain.append(low.aexprs[node["lhs"]])
        link = node["rhs"]
    assert [(k["kind"], k["name"]) for k in chain[:2]] == [(F.AE_COLUMN, "k"), (F.AE_COLUMN, "k2")] and chain[2]["kind"] == F.AE_TEMPORAL      # the keys in their order
    # dtypes are those of the same aggregate in group_by; the name is the function's root, an alias outside renames
    lf = df.lazy().with_columns(c("a").sum().over("k").alias("asum"), c("f").mean().over("k"), c("flag").n_unique().over("s").alias("nu"), pl.len().over("k").alias("n"),
                                c("a").median().over("k").alias("med"), (c("x") / c("x").sum().over("k")).alias("share"), c("d").max().over("k2").alias("dmax"))
    schema = lf.collect_schema()
    assert (schema["asum"], schema["f"], schema["nu"], schema["n"], schema["med"], schema["share"], schema["dmax"]) == \
           (pl.Int64, pl.Float32, pl.UInt32, pl.UInt32, pl.Float64, pl.Float64, pl.Date)
    low, root, _ = df.lazy().filter(c("x") > c("x").median().over("k"))._lower()
    pred = low.aexprs[low.irs[root]["predicate"]]
    assert pred["kind"] == F.AE_BINARY and low.aexprs[pred["rhs"]]["kind"] == F.AE_WINDOW
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr._fields_[-1][0] == "cond"      # plx_aexpr is what it was
    assert [ae[i].kind for i in range(n_ae)].count(14) == 1
    assert "Window[col('x').median() over [col('k')], mapping=group_to_rows] in filter" in df.lazy().filter(c("x") > c("x").median().over("k")).explain()
    with pytest.raises(KeyError, match="column not found: zz"):
        df.lazy().select(c("x").sum().over("zz"))._lower()


def test_the_header_numbering_and_the_exported_symbols(tmp_path):
    src = tmp_path / "window.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AE_WINDOW == 14 && PLX_AE_WINDOW_KEY == 15 && PLX_AE_TEMPORAL == 13, "numbering");
_Static_assert(sizeof(plx_aexpr) == 48, "plx_aexpr did not grow");
_Static_assert(offsetof(plx_aexpr, cond) == 40 && offsetof(plx_aexpr, cond) > offsetof(plx_aexpr, name), "cond is the last field, behind the name");
int (*p1)(const plx_column*, int32_t, const plx_column*, const plx_agg_op*, int32_t, const int32_t*, const double*, const int32_t*, plx_column*) = plx_window_agg;
void (*p2)(const plx_series_export*, size_t, const uint8_t*, size_t, plx_series_export*, const void*) = _polars_plugin_plx_window_agg;
void (*p3)(const struct ArrowSchema*, size_t, struct ArrowSchema*, const uint8_t*, size_t) = _polars_plugin_field_plx_window_agg;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "window.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("plx_window_agg", "_polars_plugin_plx_window_agg", "_polars_plugin_field_plx_window_agg"):
        assert hasattr(F.lib(), name), name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(w in text for w in ("plx_window_agg", "PLX_AE_WINDOW", "PLX_AE_WINDOW_KEY"))


def import_error(low, root):
    """what plan import says about the arenas (plx_debug_program_json imports the plan first): (code, message)"""
    buf = C.create_string_buffer(1 << 14)
    ir, n_ir, ae, n_ae, keep = low.to_c()
    rc = F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf))
    return rc, F.lib().plx_last_error().decode()


def test_plan_import_refuses_misplaced_links_and_windows(df):
    ERR_INVALID = 1
    # nine keys: PLX_ERR_UNSUPPORTED naming the limit
    low, root, _ = df.lazy().select(c("x").sum().over(*["k"] * 9))._lower()
    rc, msg = import_error(low, root)
    assert rc == F.ERR_UNSUPPORTED and "window over 9 keys" in msg and "1..8" in msg, msg
    # a window without a key; a link whose next is no link; a link below something that is no window; a link as an output expression
    low, root, _ = df.lazy().select(c("x").sum().over("k"))._lower()
    top = low.irs[root]["exprs"][0]
    link = low.aexprs[top]["rhs"]
    low.aexprs[top]["rhs"] = -1
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "without a key" in msg, msg
    low.aexprs[top]["rhs"] = low.aexprs[top]["lhs"]
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "without a key" in msg, msg
    low.aexprs[top]["rhs"] = link
    low.aexprs[top]["kind"] = F.AE_ALIAS
    low.aexprs[top]["name"] = "z"
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "outside a window expression's key list" in msg, msg
    low.aexprs[top]["kind"] = F.AE_WINDOW
    low.irs[root]["exprs"][0] = link
    rc, msg = import_error(low, root)
    assert rc == ERR_INVALID and "outside a window expression's key list" in msg, msg
    # in the aggregate list or the keys of a group_by: PLX_ERR_INVALID naming the window
    for lf in (df.lazy().group_by("k").agg(c("x").sum().over("k2")), df.lazy().group_by(c("x").sum().over("k2")).agg(c("x").sum())):
        low, root, _ = lf._lower()
        rc, msg = import_error(low, root)
        assert rc == ERR_INVALID and "window expression (.over)" in msg and "group_by" in msg, msg


def test_fused_pipelines_decline_by_name(df):
    for lf in (df.lazy().select(c("x").sum().over("k")), df.lazy().select((c("x") / c("x").sum().over("k")).sum()),
               df.lazy().filter(c("x") > c("x").mean().over("k")).select(c("x").sum())):
        fused, _, why, _ = lf.describe_fusion()
        assert not fused and why == REASON, why
    fused, _, why, _ = df.lazy().filter(c("x") > 0).select(c("x").sum()).describe_fusion()      # the same query without a window still fuses
    assert fused, why


def test_plugin_field_and_entry_points_without_a_device():
    import pyarrow as pa
    import torch

    from tests import plugin_abi as P
    for agg, t, want in (("sum", pa.int8(), pa.int64()), ("sum", pa.float32(), pa.float32()), ("mean", pa.int32(), pa.float64()), ("std", pa.float32(), pa.float32()),
                         ("median", pa.int64(), pa.float64()), ("n_unique", pa.float64(), pa.uint32()), ("len", pa.bool_(), pa.uint32()), ("max", pa.int16(), pa.int16())):
        assert P.field("plx_window_agg", t, {"agg": agg}).type == want, agg
    assert P.field("plx_window_agg", pa.float64(), {"agg": "sum"}, col_name="x").name == "x"
    assert P.field("plx_window_agg", pa.float64(), {"agg": "cum_sum"}) is None and "kwargs must carry agg" in P.last_error()
    if torch.cuda.is_available():
        return
    res, inp = P.call("plx_window_agg", [pa.array([1.0, 2.0]), pa.array([1, 1])], {"agg": "sum"})
    assert res is None and inp.released == 2 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    h = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.I64, 100, 0, 0, 0, 0, C.byref(h)) == 0
    keys, vals, out = (C.c_uint64 * 9)(*([h.value] * 9)), (C.c_uint64 * 1)(h.value), (C.c_uint64 * 1)()
    aggs = (C.c_int32 * 1)(F.AGG_SUM)
    assert F.lib().plx_window_agg(keys, 9, vals, aggs, 1, None, None, None, out) == F.ERR_UNSUPPORTED and "1..8 keys" in F.lib().plx_last_error().decode()
    assert F.lib().plx_window_agg(keys, 0, vals, aggs, 1, None, None, None, out) == 1
    # the parameters are refused by name before anything runs, whatever the height
    qa, bad_q, bad_ip, bad_ddof = (C.c_int32 * 1)(F.AGG_QUANTILE), (C.c_double * 1)(1.5), (C.c_int32 * 1)(7), (C.c_int32 * 1)(300)
    assert F.lib().plx_window_agg(keys, 1, vals, qa, 1, None, bad_q, None, out) == 1 and "window: quantile q" in F.lib().plx_last_error().decode()
    assert F.lib().plx_window_agg(keys, 1, vals, qa, 1, None, None, bad_ip, out) == 1 and "window: interpolation 7" in F.lib().plx_last_error().decode()
    assert F.lib().plx_window_agg(keys, 1, vals, (C.c_int32 * 1)(F.AGG_STD), 1, bad_ddof, None, None, out) == 1 and "window: ddof" in F.lib().plx_last_error().decode()
    assert F.lib().plx_window_agg(keys, 1, vals, (C.c_int32 * 1)(F.AGG_FIRST), 1, None, None, None, out) == 1 and "no window aggregate" in F.lib().plx_last_error().decode()


def test_share_of_flag_total_lowers():
    from polars_amd import queries as QQ
    rng = np.random.default_rng(11)
    n = 2000
    cols = {"l_returnflag": (rng.integers(0, 3, n).astype(np.uint8), None), "l_linestatus": (rng.integers(0, 2, n).astype(np.uint8), None),
            "l_quantity": (rng.integers(1, 51, n).astype(np.int64), None), "l_extendedprice": (rng.uniform(900.0, 100000.0, n), None)}
    lf = QQ.share_of_flag_total(frame_like(cols).lazy())
    low, root, schema = lf._lower()
    assert schema == {"l_returnflag": pl.UInt8, "l_linestatus": pl.UInt8, "l_quantity": pl.Int64, "l_extendedprice": pl.Float64, "share": pl.Float64}
    wins = [d for d in low.aexprs if d["kind"] == F.AE_WINDOW]
    assert len(wins) == 2 and [low.aexprs[w["lhs"]]["op"] for w in wins] == [F.AGG_SUM, F.AGG_QUANTILE]
    assert sum(d["kind"] == F.AE_WINDOW_KEY for d in low.aexprs) == 3
    assert low.irs[root]["kind"] == F.IR_FILTER and low.irs[low.irs[root]["input"]]["kind"] == F.IR_HSTACK


# ---- the new kernels' registers ------------------------------------------------------------------------------------------------------------
def test_window_kernels_stream_without_scratch():
    """window_slots_kernel, window_group_ids_kernel and both forms of window_broadcast_kernel: VGPRs and scratch bytes as tests/test_kernel_resources_cpu.py obtains
    them."""
    from tests.test_kernel_resources_cpu import resource_usage
    names = ("window_slots_kernel", "window_group_ids_kernel", "window_broadcast_kernel")
    res = {n: r for n, r in resource_usage("kernels_window.hip").items() if any(w in n for w in names)}
    assert len(res) == 4, sorted(res)
    for name, r in sorted(res.items()):
        print(name, "VGPRs", r["VGPRs"], "scratch", r["ScratchSize [bytes/lane]"], "LDS", r["LDS Size [bytes/block]"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r)          # they stream: eight waves per SIMD


# ---- the reference's Window node through the engine shim ------------------------------------------------------------------------------------------
def test_polars_engine_lowers_the_window_node_and_refuses_order_and_mappings(df):
    """A stand-in NodeTraverser shows PLX_AE_WINDOW as the visitor's Window node (function, partition_by, order_by, options = the mapping): the shim builds the same
    arenas back; an order_by and a mapping other than groups-to-rows are refused by name."""
    from polars_amd import polars_engine as eng
    from tests import test_polars_engine_cpu as S

    class Mapping:
        def __init__(self, kind): self.kind = kind

    class Window:
        def __init__(self, **kw): self.__dict__.update(kw)

    class WithWindow(S.FakeTraverser):
        order_by, mapping = None, "groups_to_rows"

        def view_expression(self, i):
            d = self.low.aexprs[i]
            if d["kind"] != F.AE_WINDOW:
                return super().view_expression(i)
            keys, link = [], d["rhs"]
            while link >= 0:
                keys.append(self.low.aexprs[link]["lhs"])
                link = self.low.aexprs[link]["rhs"]
            return Window(function=d["lhs"], partition_by=keys, order_by=self.order_by, order_by_descending=False, order_by_nulls_last=False, options=Mapping(self.mapping))

    lf = df.lazy().with_columns((c("x") / c("x").sum().over("k", "k2")).alias("share")).filter(c("x") > c("x").mean().over("k"))
    low, root, _ = lf._lower()
    back = eng.Translator(WithWindow(low, root), frame_of=lambda node: node.df).plan()
    low2, root2, _ = back._lower()
    assert S.canonical(low, root) == S.canonical(low2, root2)
    assert sum(d["kind"] == F.AE_WINDOW for d in low2.aexprs) == 2 and sum(d["kind"] == F.AE_WINDOW_KEY for d in low2.aexprs) == 3
    for attr, value, word in (("order_by", 0, "order_by"), ("mapping", "join", "mapping join"), ("mapping", "explode", "mapping explode")):
        nt = WithWindow(low, root)
        setattr(nt, attr, value)
        with pytest.raises(eng.NotSupported, match=word):
            eng.Translator(nt, frame_of=lambda node: node.df).plan()


# ---- a window above a file scan: nothing is pruned below it ------------------------------------------------------------------------------------------
def test_no_predicate_is_pushed_to_a_scan_past_a_window(tmp_path):
    """A window reads every row of its filter's input.  The simple conjuncts of a filter that holds a window, and of the filters above it, must not reach the scan
    (row groups dropped by statistics would change the window's sums); a filter BELOW the window still prunes."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from polars_amd import io
    n = 5000
    path = str(tmp_path / "w.parquet")
    pq.write_table(pa.table({"k": pa.array(np.arange(n) % 7), "x": pa.array(np.arange(n, dtype=np.float64)), "y": pa.array(np.arange(n))}), path, row_group_size=500)

    def scan_of(lf):
        io.reset_scans(lf._node); io.push_down(lf._node)
        node = lf._node
        while node.kind != "scan":
            node = node.input
        return node.frame
    above_mean = c("x") > c("x").mean().over("k")
    for lf in (pl.scan_parquet(path).filter((c("y") > 2500) & above_mean),                      # one predicate
               pl.scan_parquet(path).filter(above_mean).filter(c("y") > 2500),                  # the simple filter above the window's
               pl.scan_parquet(path).filter(above_mean).filter(c("y") > 2500).filter(c("y") < 4000).select("x")):
        src = scan_of(lf)
        assert src._preds == [] and len(src.selected_row_groups()) == 10, src._preds
        assert "STATISTICS PRUNING" not in lf.explain(), lf.explain()
        assert {"k", "x", "y"} <= set(src.selected_columns())
    # below the window the rows never reach it: pruned as before, and only the lower filter's conjunct
    lf = pl.scan_parquet(path).filter(c("y") > 2500).filter(above_mean & (c("y") < 4000))
    src = scan_of(lf)
    assert src._preds == [("y", F.OP_GT, 2500)] and len(src.selected_row_groups()) == 5
    assert "STATISTICS PRUNING: [y > 2500]" in lf.explain(), lf.explain()
    # a window in with_columns: the filter above it was never pushed through, and is not now
    src = scan_of(pl.scan_parquet(path).with_columns(c("x").sum().over("k").alias("s")).filter(c("y") > 2500))
    assert src._preds == [] and len(src.selected_row_groups()) == 10
    # without a window nothing changed
    src = scan_of(pl.scan_parquet(path).filter(c("x") > 1.0).filter(c("y") > 2500))
    assert sorted(src._preds) == [("x", F.OP_GT, 1.0), ("y", F.OP_GT, 2500)] and len(src.selected_row_groups()) == 5
