"""join_asof without a GPU: the reference loop (its hand-written vectors, pandas.merge_asof), asof.hpp walked lane by lane under ASan + UBSan, the lowering into
PLX_IR_JOIN_ASOF, the argument errors, the plan importer's refusals, and the kernels' registers and LDS."""
import ctypes as C
import datetime as dt
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import asof_ref as A
from tests.test_program_eval_cpu import frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
ERR_INVALID = 1


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------
def test_the_reference_checks_itself():
    assert A.self_check() > 700
    idx, ok = A.join_asof(np.array([5, 1]), np.array([3, 7]), strategy="nearest")
    A.check(np.array([1, 0], np.uint32), None, idx, ok)
    with pytest.raises(AssertionError):
        A.check(np.array([0, 0], np.uint32), None, idx, ok)                       # the matched row is part of the check
    with pytest.raises(AssertionError):
        A.check(np.array([1, 0], np.uint32), np.array([True, False]), idx, ok)    # ... and so is every validity bit
    idx, ok = A.join_asof(np.array([5, 1]), np.array([3, 7]), strategy="backward")
    with pytest.raises(AssertionError):
        A.check(np.array([0, 0], np.uint32), None, idx, ok)                       # a column without validity claims that every row matched


def pandas_asof(pd, lo, ro, lb, rb, direction, exact, tolerance):
    left = pd.DataFrame({"on": lo, "i": np.arange(len(lo))})
    right = pd.DataFrame({"on": ro, "j": np.arange(len(ro))})
    by = None
    if lb is not None:
        left["by"], right["by"], by = lb, rb, "by"
    m = pd.merge_asof(left, right, on="on", by=by, direction=direction, allow_exact_matches=exact, tolerance=tolerance)
    assert np.array_equal(m["i"].to_numpy(), np.arange(len(lo)))
    j = m["j"].to_numpy()
    return np.where(np.isnan(j), 0, j).astype(np.int64), ~np.isnan(j)


def test_the_reference_against_pandas_merge_asof():
    """pandas.merge_asof needs both sides sorted by `on` and free of nulls; on those inputs the contract is its behaviour, but for the two documented differences of
    `nearest`: pandas sends an equidistant pair backward and takes the first row of a duplicated forward value."""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(7)
    rows = 0
    # sparse values: the rule itself (nearest_tie="forward") on every row it shares with pandas
    for with_by in (False, True):
        for tolerance in (None, 40):
            n, m = 700, 600
            lo, ro = np.sort(rng.integers(0, 100 * (n + m), n)), np.sort(rng.integers(0, 100 * (n + m), m))
            lb, rb = (rng.integers(0, 4, n), rng.integers(0, 4, m)) if with_by else (None, None)
            by = dict(left_by=[lb], right_by=[rb]) if with_by else {}
            for exact in (True, False):
                for direction in A.STRATEGIES:
                    got = A.join_asof(lo, ro, strategy=direction, strict=not exact, tolerance=tolerance, **by)
                    want = pandas_asof(pd, lo, ro, lb, rb, direction, exact, tolerance)
                    if direction == "nearest":
                        # leave out the rows with an equidistant pair of distinct values or a duplicated forward value: where the two tie rules part
                        same = A.join_asof(lo, ro, strategy=direction, strict=not exact, tolerance=tolerance, nearest_tie="backward", **by)
                        keep = (same[0] == got[0]) & (same[1] == got[1])
                        assert 1.0 - keep.mean() <= 0.05, (with_by, tolerance, exact, 1.0 - keep.mean())
                    else:
                        keep = np.ones(n, bool)
                    assert np.array_equal(got[1][keep], want[1][keep]) and np.array_equal(got[0][keep & got[1]], want[0][keep & got[1]]), (with_by, tolerance, exact, direction)
                    rows += int(keep.sum())
    # small dense ranges, full of ties and duplicates: every row, with the switch that sends ties where pandas sends them
    for with_by in (False, True):
        for tolerance in (None, 1):
            n, m = 400, 300
            lo, ro = np.sort(rng.integers(0, 60, n)), np.sort(rng.integers(0, 60, m))
            lb, rb = (rng.integers(0, 3, n), rng.integers(0, 3, m)) if with_by else (None, None)
            by = dict(left_by=[lb], right_by=[rb]) if with_by else {}
            for exact in (True, False):
                for direction in A.STRATEGIES:
                    got = A.join_asof(lo, ro, strategy=direction, strict=not exact, tolerance=tolerance, nearest_tie="backward", **by)
                    want = pandas_asof(pd, lo, ro, lb, rb, direction, exact, tolerance)
                    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0][got[1]], want[0][got[1]]), (with_by, tolerance, exact, direction)
                    rows += n
    assert rows > 25_000
    # floats
    lo, ro = np.sort(rng.normal(0, 5, 300)), np.sort(rng.normal(0, 5, 200))
    for direction in A.STRATEGIES:
        got = A.join_asof(lo, ro, strategy=direction, tolerance=0.5, nearest_tie="backward")
        want = pandas_asof(pd, lo, ro, None, None, direction, True, 0.5)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0][got[1]], want[0][got[1]]), direction


def test_the_arithmetic_under_sanitizers_against_a_direct_loop(tmp_path):
    """tests/emu/asof_main.cpp: asof.hpp lane by lane -- the sample stage over an array of exactly W * ns words, the global stage, pick and the tolerance -- against a
    loop over the candidates, with S = samples_for(W) and with S = 0, at the sizes and value edges of the GPU tests."""
    exe = str(tmp_path / "asof_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "asof_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 400_000, r.stdout


# ---- lowering -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    n, m = 6, 5
    left = frame_like({"sym": (np.zeros(n, np.int32), None), "ok": (np.zeros(n, bool), None), "t": (np.zeros(n, np.int64), None), "w": (np.zeros(n, np.int16), None),
                       "x": (np.zeros(n), None), "d": (np.zeros(n, np.int32), None), "ms": (np.zeros(n, np.int64), None), "ns": (np.zeros(n, np.int64), None),
                       "u": (np.zeros(n, np.uint64), None), "cat": (np.zeros(n, np.uint32), None), "price": (np.zeros(n), None)},
                      {"t": pl.Datetime, "d": pl.Date, "ms": pl.Datetime("ms"), "ns": pl.Datetime("ns"), "cat": pl.Categorical(["a", "b"])})
    right = frame_like({"sym": (np.zeros(m, np.int32), None), "ok": (np.zeros(m, bool), None), "t": (np.zeros(m, np.int64), None), "w": (np.zeros(m, np.int64), None),
                        "x": (np.zeros(m), None), "d": (np.zeros(m, np.int32), None), "ms": (np.zeros(m, np.int64), None), "ns": (np.zeros(m, np.int64), None),
                        "u": (np.zeros(m, np.uint64), None), "cat": (np.zeros(m, np.uint32), None), "price": (np.zeros(m), None), "bid": (np.zeros(m), None)},
                       {"t": pl.Datetime, "d": pl.Date, "ms": pl.Datetime("ms"), "ns": pl.Datetime("ns"), "cat": pl.Categorical(["a", "b"])})
    return left, right


def lowered(lf):
    low, root, schema = lf._lower()
    return low, low.irs[root], schema


def test_lowering_by_parts_first_on_last_strategy_bits_and_the_tolerance_literal(frames):
    L, R = frames
    low, node, schema = lowered(L.lazy().join_asof(R.lazy(), on="t", by=["sym", "ok"], strategy="nearest", allow_exact_matches=False, tolerance=5))
    assert node["kind"] == F.IR_JOIN_ASOF == 9 and node["how"] == (F.ASOF_NEAREST | F.ASOF_STRICT) == 6 and node["maintain_order"] == 0 and node["coalesce"] == 0
    assert [low.aexprs[k]["name"] for k in node["keys"]] == ["sym", "ok", "t"] == [low.aexprs[k]["name"] for k in node["keys_right"]]
    tol = low.aexprs[node["predicate"]]
    assert (tol["kind"], tol["dtype"], tol["lit"], tol["is_null"]) == (F.AE_LITERAL, F.I64, 5, 0)
    assert list(schema) == list(L.schema) + ["w_right", "x_right", "d_right", "ms_right", "ns_right", "u_right", "cat_right", "price_right", "bid"]
    for strategy, strict, how in (("backward", False, 0), ("forward", False, 1), ("nearest", False, 2), ("backward", True, 4), ("forward", True, 5)):
        _, node, _ = lowered(L.lazy().join_asof(R.lazy(), on="t", strategy=strategy, allow_exact_matches=not strict))
        assert node["how"] == how and node["predicate"] == -1 and len(node["keys"]) == 1
    # the tolerance in the family of `on`: exact timedelta conversions, a float for floats, an unsigned literal for an unsigned `on`
    for on, tolerance, dtype, lit in (("t", dt.timedelta(seconds=1), F.I64, 1_000_000), ("ms", dt.timedelta(seconds=1, milliseconds=3), F.I64, 1003),
                                      ("ns", dt.timedelta(days=1, microseconds=7), F.I64, 86_400_000_007_000), ("d", dt.timedelta(days=3), F.I64, 3), ("d", 2, F.I64, 2),
                                      ("x", 0.25, F.F64, 0.25), ("x", 2, F.F64, 2.0), ("u", 2 ** 64 - 1, F.U64, 2 ** 64 - 1), ("t", 0, F.I64, 0), ("t", np.int64(9), F.I64, 9)):
        low, node, _ = lowered(L.lazy().join_asof(R.lazy(), on=on, tolerance=tolerance))
        tol = low.aexprs[node["predicate"]]
        assert (tol["kind"], tol["dtype"], tol["lit"]) == (F.AE_LITERAL, dtype, lit), (on, tolerance, tol)
    for on, tolerance, word in (("ms", dt.timedelta(microseconds=1500), "no whole number"), ("d", dt.timedelta(hours=36), "no whole number"), ("x", dt.timedelta(1), "needs a Date or Datetime"),
                                ("t", 1.5, "an int in the column's own unit"), ("t", 2 ** 63, "does not fit"), ("t", "2h", "duration strings"), ("x", "1s", "duration strings")):
        with pytest.raises(ValueError, match=word):
            L.lazy().join_asof(R.lazy(), on=on, tolerance=tolerance)._lower()
    # integers of different width meet in their supertype, as in join
    low, node, _ = lowered(L.lazy().join_asof(R.lazy(), on="w"))
    lk, rk = low.aexprs[node["keys"][0]], low.aexprs[node["keys_right"][0]]
    assert (lk["kind"], lk["dtype"]) == (F.AE_CAST, F.I64) and rk["kind"] == F.AE_COLUMN
    # to_c carries the node as it is
    ir, n_ir, ae, n_ae, keep = L.lazy().join_asof(R.lazy(), on="t", by="sym", tolerance=3, strategy="forward", suffix="_q", coalesce=False)._lower()[0].to_c()
    top = ir[n_ir - 1]
    assert (top.kind, top.how, top.n_keys, top.n_keys_right, top.coalesce, top.suffix, top.maintain_order) == (9, 1, 2, 2, F.JOIN_KEEP_BOTH, b"_q", 0) and ae[top.predicate].lit.i == 3


def test_the_abi_did_not_grow(tmp_path):
    src = tmp_path / "asof.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_IR_JOIN_ASOF == 9 && PLX_IR_DISTINCT == 8, "numbering");
_Static_assert(PLX_ASOF_BACKWARD == 0 && PLX_ASOF_FORWARD == 1 && PLX_ASOF_NEAREST == 2 && PLX_ASOF_STRICT == 4, "plx_asof_strategy");
_Static_assert(sizeof(plx_ir) == 128 && offsetof(plx_ir, coalesce) == 120, "plx_ir did not grow, coalesce is its trailing field");
int (*p1)(int32_t, const plx_column*, const plx_column*, int32_t, plx_column, plx_column, const plx_scalar*, plx_column*) = plx_join_asof_indices;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "asof.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert hasattr(F.lib(), "plx_join_asof_indices")
    assert C.sizeof(F.IR) == 128 and F.IR.coalesce.offset == 120
    assert F.asof_samples_for(1) == 8192 and F.asof_samples_for(3) == 2730 and F.asof_samples_for(8) == 1024 and F.asof_samples_for(9) == 0
    for name, word in (("INTEGRATION.md", "plx_join_asof_indices"), ("DESIGN.md", "4.20"), ("README.md", "join_asof")):
        with open(os.path.join(ROOT, name)) as f:
            assert word in f.read(), name


def test_collect_schema_follows_the_left_join_column_rules(frames):
    L, R = frames
    l2 = L.lazy().select("sym", "t", "price")
    r2 = R.lazy().select("sym", "t", "price", "bid")
    assert list(l2.join_asof(r2, on="t", by="sym").collect_schema()) == ["sym", "t", "price", "price_right", "bid"]
    assert list(l2.join_asof(r2, on="t", by="sym", coalesce=True, suffix="_q").collect_schema()) == ["sym", "t", "price", "price_q", "bid"]
    assert list(l2.join_asof(r2, on="t", by="sym", coalesce=False, suffix="_q").collect_schema()) == ["sym", "t", "price", "sym_q", "t_q", "price_q", "bid"]
    got = l2.join_asof(r2.rename({"t": "qt", "sym": "qsym"}), left_on="t", right_on="qt", by_left="sym", by_right="qsym").collect_schema()
    assert list(got) == ["sym", "t", "price", "price_right", "bid"] and got["t"] == pl.Datetime and got["bid"] == pl.Float64
    # a key expression that is no plain column never merges
    assert list(l2.join_asof(r2, left_on=c("t") + 1, right_on="t", by="sym").collect_schema()) == ["sym", "t", "price", "t_right", "price_right", "bid"]
    lines = l2.join_asof(r2, on="t", by="sym", strategy="nearest", tolerance=dt.timedelta(seconds=2)).explain()
    assert "JoinAsof[strategy=nearest" in lines and "tolerance=datetime.timedelta(seconds=2)" in lines and "order=left rows" in lines


def test_every_argument_error_fires_with_its_message(frames):
    L, R = frames
    l, r = L.lazy(), R.lazy()
    for kw, word in ((dict(on="t", left_on="t"), "`on` .* given together with `left_on` / `right_on`"), (dict(on="t", right_on="t"), "given together with `left_on` / `right_on`"),
                     (dict(on="t", by="sym", by_left="sym"), "`by` .* given together with `by_left` / `by_right`"), (dict(on="t", by_left=["sym", "ok"], by_right=["sym"]), r"`by_left` \(2\) does not match the length of `by_right` \(1\)"),
                     (dict(on="t", by=["sym"] * 8), "8 by parts"), (dict(on="t", tolerance=-1), "tolerance=-1 is negative"), (dict(on="x", tolerance=float("nan")), "tolerance=nan"),
                     (dict(on="x", tolerance=-0.5), "tolerance=-0.5 is negative"), (dict(on="t", tolerance=dt.timedelta(seconds=-1)), "is negative"), (dict(on="t", strategy="closest"), "strategy must be one of .* got 'closest'"),
                     (dict(on="t", check_sortedness=1), "check_sortedness must be a bool, got 1"), (dict(on="t", allow_parallel="yes"), "allow_parallel must be a bool, got 'yes'"),
                     (dict(on="t", force_parallel=None), "force_parallel must be a bool, got None"), (dict(on="t", tolerance="2h"), "tolerance='2h': duration strings"), (dict(left_on="t"), "needs `on`"),
                     (dict(on="t", coalesce=1), "coalesce must be None, True or False")):
        with pytest.raises(ValueError, match=word):
            l.join_asof(r, **kw)
    with pytest.raises(ValueError, match="tolerance=-1"):
        L.join_asof(R, on="t", tolerance=-1)                                      # the eager form checks before it runs anything
    for kw, word in ((dict(on="ok"), "`on` is Boolean"), (dict(on="cat"), "`on` is Categorical"), (dict(on="t", by="cat"), r"by part 0 .* is Categorical: Categorical by parts are not on this path yet"),
                     (dict(left_on="ms", right_on="ns"), r"join keys Datetime\[ms\] and Datetime\[ns\]"), (dict(left_on="d", right_on="t"), "`on` is Date on the left and Datetime on the right"),
                     (dict(left_on="d", right_on="sym"), "`on` is Date on the left and Int32 on the right")):
        with pytest.raises(TypeError, match=word):
            l.join_asof(r, **kw)._lower()
    l.join_asof(r, on="t", check_sortedness=False, allow_parallel=False, force_parallel=True)._lower()      # accepted: they have nothing to do


# ---- the plan importer ---------------------------------------------------------------------------------------------------------------------------------
def execute_error(low, root):
    """what plx_execute_plan says about the arenas: plan import comes first, before any column is touched (these are placeholders: no device is bound)"""
    ir, n_ir, ae, n_ae, keep = low.to_c()
    out = C.c_uint64()
    rc = F.lib().plx_execute_plan(ir, n_ir, ae, n_ae, root, 0, C.byref(out))
    return rc, F.lib().plx_last_error().decode()


def test_plan_import_refuses_before_it_needs_a_device(frames):
    L, R = frames
    low, root, _ = L.lazy().join_asof(R.lazy(), on="t", by="sym", tolerance=3)._lower()
    node = low.irs[root]
    tol = node["predicate"]
    for field, value, code, word in (("how", 3, ERR_INVALID, "no plx_asof_strategy"), ("how", 7, ERR_INVALID, "no plx_asof_strategy"), ("how", 8, ERR_INVALID, "no plx_asof_strategy"),
                                     ("how", -1, ERR_INVALID, "no plx_asof_strategy"), ("keys_right", node["keys_right"][:1], ERR_INVALID, "2 left keys against 1 right keys"),
                                     ("keys", [], ERR_INVALID, "0 left keys"), ("maintain_order", 1, ERR_INVALID, "maintain_order must be 0"), ("predicate", node["keys"][0], ERR_INVALID, "non-null literal"),
                                     ("predicate", len(low.aexprs), ERR_INVALID, "non-null literal"), ("predicate", -2, ERR_INVALID, "non-null literal"), ("coalesce", 3, ERR_INVALID, "coalesce outside 0..2"),
                                     ("keys", node["keys"][:1] * 9, F.ERR_UNSUPPORTED, "9 keys")):
        saved = node[field]
        node[field] = value
        if field == "keys" and len(value) == 9:
            node["keys_right"], saved_right = node["keys_right"][:1] * 9, node["keys_right"]
        rc, msg = execute_error(low, root)
        assert rc == code and word in msg, (field, value, rc, msg)
        node[field] = saved
        if field == "keys" and len(value) == 9:
            node["keys_right"] = saved_right
    for dtype, lit, word in ((F.I64, -1, ">= 0, got -1"), (F.F64, -0.5, ">= 0, got -0.5"), (F.F64, float("nan"), ">= 0")):
        saved = dict(low.aexprs[tol])
        low.aexprs[tol]["dtype"], low.aexprs[tol]["lit"] = dtype, lit
        rc, msg = execute_error(low, root)
        assert rc == ERR_INVALID and "tolerance" in msg and word in msg, (dtype, lit, msg)
        low.aexprs[tol].update(saved)
    low.aexprs[tol]["is_null"] = 1
    rc, msg = execute_error(low, root)
    assert rc == ERR_INVALID and "non-null literal" in msg, msg


def test_the_example_query_lowers():
    from polars_amd import queries as QQ
    n = 50
    cols = {"sym": (np.zeros(n, np.int32), None), "ts": (np.zeros(n, np.int64), None), "price": (np.zeros(n), None)}
    low, root, schema = QQ.quote_before_trade(frame_like(cols, {"ts": pl.Datetime}).lazy(), frame_like(cols, {"ts": pl.Datetime}).lazy())._lower()
    assert list(schema) == ["sym", "trades", "quoted", "mean_over_quote", "max_quote"] and low.irs[root]["kind"] == F.IR_GROUPBY
    j = low.irs[low.irs[root]["input"]]
    assert j["kind"] == F.IR_JOIN_ASOF and j["how"] == F.ASOF_BACKWARD and low.aexprs[j["predicate"]]["lit"] == 1_000_000
    with pytest.raises(F.UnsupportedError, match="source must be a scan"):          # the fused pipelines do not look at the node: the group_by runs per node on its output
        QQ.quote_before_trade(frame_like(cols, {"ts": pl.Datetime}).lazy(), frame_like(cols, {"ts": pl.Datetime}).lazy()).describe_fusion()


# ---- the kernels' registers and LDS ----------------------------------------------------------------------------------------------------------------
def test_asof_kernels_run_without_scratch_and_within_the_lds_budget():
    """kernels_asof.hip, every instantiation (W = 1..8; the search with and without the LDS stage): no scratch; LDS at most 64 KiB, so that two workgroups share a
    CU's 160 KiB; the search kernel within 128 VGPRs."""
    from tests.test_kernel_resources_cpu import resource_usage
    res = resource_usage("kernels_asof.hip")
    assert all(sum(w in n for n in res) >= 8 for w in ("asof_order_check_kernel", "asof_encode_kernel")) and sum("asof_search_kernel" in n for n in res) == 16, sorted(res)
    staged = 0
    for name, r in sorted(res.items()):
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        lds = int(r["LDS Size [bytes/block]"])
        assert lds <= 64 * 1024 and 2 * lds <= 160 * 1024, (name, lds)
        if "asof_search_kernel" in name:
            assert int(r["VGPRs"]) <= 128, (name, r)
            staged += lds == 64 * 1024
        else:
            assert lds == 0, (name, lds)
    assert staged == 8
