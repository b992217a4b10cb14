"""when / then / otherwise without a GPU: the mirror API and its lowering (dtypes, names, chains, the trailing plx_aexpr.cond field), the fused programs the
C++ compiler emits for queries that contain a conditional (interpreted row by row: tests/program_eval_select.py adds OP_SELECT to tests/program_eval.py) against
numpy's np.where(predicate value & predicate validity, then, otherwise) for values and validity alike, the run-time compiled kernel's source (jit_selftest) and
the Polars attachment's Ternary node."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import polars_engine as eng
from tests import program_eval
from tests import program_eval_select as pes
from tests.test_polars_engine_cpu import FakeTraverser, _cls
from tests.test_program_eval_cpu import by_key, close, frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col


@pytest.fixture
def pe(monkeypatch):
    """program_eval whose run_rows knows OP_SELECT (evaluate and split_matches call it through the module)."""
    monkeypatch.setattr(program_eval, "run_rows", pes.run_rows)
    return program_eval


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(28)
    n = 3001
    cols = {"a": (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) < 0.8), "b": (rng.integers(-50, 50, n).astype(np.int64), None),
            "x": (rng.normal(size=n), rng.random(n) < 0.7), "y": (rng.normal(size=n), None), "k": (rng.integers(0, 5, n).astype(np.int64), None),
            "flag": (rng.random(n) < 0.5, rng.random(n) < 0.75), "i32": (rng.integers(-9, 9, n).astype(np.int32), None)}
    return cols, frame_like(cols)


def where(pred, then, other):
    """The reference of every check: (values, validity) arrays in, (values, validity) out; a null predicate row takes `other`."""
    (pv, pm), (av, am), (bv, bm) = pred, then, other
    t = pv & pm
    return np.where(t, av, bv), np.where(t, am, bm)


def full(cols, name):
    v, m = cols[name]
    return v, np.ones(len(v), bool) if m is None else m


def lit_col(n, value, valid=True):
    return np.full(n, value), np.full(n, valid)


# ---- the mirror API and its lowering ---------------------------------------------------------------------------------------------
def lowered(df, expr):
    low, root, schema = df.lazy().select(expr)._lower()
    return low, low.aexprs[low.irs[root]["exprs"][0]], schema


def test_dtype_table_and_output_names(data):
    _, df = data
    table = [
        (pl.when(c("flag")).then(c("a")).otherwise(3), pl.Int64, "a"),                       # a python int takes the other branch's dtype
        (pl.when(c("flag")).then(2).otherwise(c("a")), pl.Int64, "literal"),
        (pl.when(c("flag")).then(c("a")).otherwise(2.5), pl.Float64, "a"),                   # int column vs python float: the column is cast
        (pl.when(c("flag")).then(c("a")).otherwise(c("x")), pl.Float64, "a"),
        (pl.when(c("flag")).then(c("i32")).otherwise(c("a")), pl.Int64, "i32"),              # supertype of the two columns
        (pl.when(c("a") > 0).then(c("flag")).otherwise(c("b") < 0), pl.Boolean, "flag"),
        (pl.when(c("flag")).then(1).otherwise(0), pl.Int32, "literal"),                      # two python ints
        (pl.when(c("flag")).then(1.5).otherwise(0.0), pl.Float64, "literal"),
        (pl.when(c("flag")).then(c("x")), pl.Float64, "x"),                                  # open otherwise: a null of the then dtype
        (pl.when(c("flag")).then(None).otherwise(c("i32")), pl.Int32, "literal"),
        (pl.when(c("flag")).then(c("a")).otherwise(0).alias("z"), pl.Int64, "z"),
    ]
    for expr, want_dt, want_name in table:
        low, top, schema = lowered(df, expr)
        assert list(schema.items()) == [(want_name, want_dt)], (repr(expr), schema)
        t = top if top["kind"] == F.AE_TERNARY else low.aexprs[top["lhs"]]
        assert t["kind"] == F.AE_TERNARY and min(t["lhs"], t["rhs"], t["cond"]) >= 0
    # the branches reach the engine with one dtype: casts sit under the node
    low, top, _ = lowered(df, pl.when(c("flag")).then(c("i32")).otherwise(c("a")))
    assert low.aexprs[top["lhs"]]["kind"] == F.AE_CAST and low.aexprs[top["lhs"]]["dtype"] == F.I64 and low.aexprs[top["rhs"]]["kind"] == F.AE_COLUMN
    low, top, _ = lowered(df, pl.when(c("flag")).then(c("x")))
    assert low.aexprs[top["rhs"]]["kind"] == F.AE_LITERAL and low.aexprs[top["rhs"]]["is_null"] == 1 and low.aexprs[top["rhs"]]["dtype"] == F.F64


def test_chains_nest_in_the_falsy_branch_and_errors(data):
    _, df = data
    chain = pl.when(c("a") > 5).then(1).when(c("a") > 0).then(2).otherwise(3)
    assert isinstance(pl.when(c("flag")), pl.When) and isinstance(pl.when(c("flag")).then(1), pl.Then) and isinstance(pl.when(c("flag")).then(1), pl.Expr)
    assert chain.kind == "ternary" and chain.rhs.kind == "ternary" and chain.rhs.rhs.kind == "lit" and chain.rhs.rhs.value == 3
    assert repr(chain) == "when((col('a') <4> lit(5))).then(lit(1)).otherwise(when((col('a') <4> lit(0))).then(lit(2)).otherwise(lit(3)))"
    assert repr(pl.when(c("flag")).then(c("a"))) == "when(col('flag')).then(col('a'))" and repr(pl.when(c("flag"))) == "when(col('flag'))"
    open_chain = pl.when(c("a") > 5).then(c("b")).when(c("a") > 0).then(c("a"))                 # no otherwise: the innermost falsy branch is the null
    low, top, schema = lowered(df, open_chain)
    inner = low.aexprs[top["rhs"]]
    assert schema == {"b": pl.Int64} and inner["kind"] == F.AE_TERNARY and low.aexprs[inner["rhs"]]["is_null"] == 1
    with pytest.raises(TypeError, match="Boolean predicate"):
        lowered(df, pl.when(c("a")).then(1).otherwise(0))
    with pytest.raises(TypeError):
        lowered(df, pl.when(c("flag")).then(pl.lit(1, pl.Date)).otherwise(pl.lit(1, pl.Datetime)))
    # projection pushdown and the other walkers see all three children
    from polars_amd import io
    assert io.expr_columns(pl.when(c("flag")).then(c("a")).otherwise(c("x"))) == {"flag", "a", "x"}


def test_cond_is_the_trailing_field_of_plx_aexpr(data, tmp_path):
    _, df = data
    low, root, _ = df.lazy().select(pl.when(c("flag")).then(c("a")).otherwise(0), (c("a") + 1).alias("p"))._lower()
    ir, n_ir, ae, n_ae, keep = low.to_c()
    for i, d in enumerate(low.aexprs):
        assert ae[i].cond == d["cond"] and (d["cond"] >= 0) == (d["kind"] == F.AE_TERNARY)
    assert F.AE_TERNARY == 11 and F.AExpr._fields_[-1][0] == "cond" and F.AExpr._fields_[-2][0] == "name"
    assert F.AExpr.cond.offset == F.AExpr.name.offset + 8
    src = tmp_path / "ternary.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "polars_amd.h"
_Static_assert(PLX_AE_TERNARY == 11 && PLX_AE_FILL_NULL == 10, "plx_aexpr_kind numbering");
_Static_assert(offsetof(plx_aexpr, cond) == offsetof(plx_aexpr, name) + sizeof(char*), "cond is the trailing field, after name");
int main(void) {
  plx_aexpr e = {0};
  if (e.cond != 0 || e.kind != PLX_AE_COLUMN) return 1;
  if (plx_version() != ((PLX_ABI_MAJOR << 16) | PLX_ABI_MINOR)) return 10;
  printf("%zu %zu %zu\n", offsetof(plx_aexpr, name), offsetof(plx_aexpr, cond), sizeof(plx_aexpr));
  return 0;
}
''')
    exe = tmp_path / "ternary"
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "polars_amd")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lpolars_amd", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert [int(x) for x in run.stdout.split()] == [F.AExpr.name.offset, F.AExpr.cond.offset, C.sizeof(F.AExpr)]
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "pub cond: i32" in f.read()


def test_the_plan_importer_checks_a_ternary_before_it_needs_a_device(data):
    _, df = data
    low, root, _ = df.lazy().select(pl.when(c("flag")).then(c("a")).otherwise(c("x").cast(pl.Int64)).sum())._lower()
    top = low.aexprs[low.aexprs[low.irs[root]["exprs"][0]]["lhs"]]
    top["rhs"] = low.aexprs[top["rhs"]]["lhs"]          # drop the cast: Int64 against Float64 branches
    ir, n_ir, ae, n_ae, keep = low.to_c()
    buf = C.create_string_buffer(1 << 12)
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) != 0
    assert "different dtypes" in F.lib().plx_last_error().decode()
    top["cond"] = -1
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) != 0
    assert "predicate" in F.lib().plx_last_error().decode()


# ---- the fused programs, row by row ------------------------------------------------------------------------------------------------
def has_select(prog):
    return any(op[0] == pes.OP_SELECT for op in prog["ops"])


def test_filter_and_whole_frame_aggregates(data, pe):
    """a ternary inside the predicate (nullable predicate column, a nullable branch), ternaries as aggregate sources, split order"""
    cols, df = data
    n = len(cols["k"][0])
    q = (df.lazy().filter(pl.when(c("flag")).then(c("a")).otherwise(c("b")) > 3)
         .select(pl.when(c("a") > 0).then(c("x") * c("y")).otherwise(0.0).sum().alias("s"), pl.when(c("flag")).then(c("x")).otherwise(c("y")).count().alias("cnt"),
                 pl.when(c("a") > 0).then(c("a")).otherwise(7).min().alias("mn"), pl.when(c("flag")).then(1).otherwise(0).sum().alias("hits"), pl.len().alias("n")))
    prog = q.debug_program()
    assert has_select(prog) and prog["any_late"] == 1
    got = pe.evaluate(prog, cols)
    (a, am), (b, bm), (x, xm), (y, ym), flag = full(cols, "a"), full(cols, "b"), full(cols, "x"), full(cols, "y"), full(cols, "flag")
    kv, km = where(flag, (a, am), (b, bm))
    keep = km & (kv > 3)
    sv, sm = where((a > 0, am), (x * y, xm), lit_col(n, 0.0))
    assert math.isclose(got["s"][0][0], sv[keep & sm].sum(), rel_tol=1e-9)
    assert got["cnt"][0][0] == int((keep & where(flag, (x, xm), (y, ym))[1]).sum())
    mv, mm = where((a > 0, am), (a, am), lit_col(n, 7))
    assert got["mn"][0][0] == mv[keep & mm].min() and got["hits"][0][0] == int((keep & flag[0] & flag[1]).sum()) and got["n"][0][0] == int(keep.sum())
    assert pe.split_matches(prog, cols)          # the predicate's third source (the flag column's load) must run early


def test_group_key_and_group_aggregates(data, pe):
    cols, df = data
    n = len(cols["k"][0])
    q = (df.lazy().group_by(pl.when(c("a") > 0).then(c("k")).otherwise(-1).alias("g"), pl.when(c("flag")).then(c("a")).otherwise(c("a") * 0).alias("h"))
         .agg(pl.when(c("flag")).then(c("x")).otherwise(c("y")).sum().alias("s"), pl.when(c("b") > 0).then(c("a")).otherwise(c("i32")).mean().alias("m"), pl.len().alias("n")))
    prog = q.debug_program()
    assert has_select(prog)
    got = by_key(pe.evaluate(prog, cols), ["g", "h"])
    (a, am), (b, bm), (x, xm), (y, ym), flag, (k, _), (i32, _) = (full(cols, nm) for nm in ("a", "b", "x", "y", "flag", "k", "i32"))
    gv, gm = where((a > 0, am), (k, np.ones(n, bool)), lit_col(n, -1))
    hv, hm = where(flag, (a, am), (a * 0, am))
    sv, sm = where(flag, (x, xm), (y, ym))
    mv, mm = where((b > 0, bm), (a, am), (i32.astype(np.int64), np.ones(n, bool)))
    assert gm.all()
    want = {}
    for key in {(int(g), int(h) if ok else None) for g, h, ok in zip(gv, hv, hm)}:
        rows = (gv == key[0]) & ((~hm) if key[1] is None else (hm & (hv == key[1])))
        want[key] = {"s": float(sv[rows & sm].sum()), "m": float(mv[rows & mm].mean()) if (rows & mm).any() else None, "n": int(rows.sum())}
    assert set(got) == set(want)
    for key, w in want.items():
        assert got[key]["n"] == w["n"] and close(got[key]["s"], w["s"]) and close(got[key]["m"], w["m"]), (key, got[key], w)


def test_null_branches_lower_without_a_select(data, pe):
    """then(a) without an otherwise = a, valid where the predicate is valid and true (OP_MASKV); then(None).otherwise(b) = b under NOT(ifnull(p, 0))"""
    cols, df = data
    n = len(cols["k"][0])
    q = df.lazy().group_by("k").agg(pl.when(c("a") > 0).then(c("y")).sum().alias("s"), pl.when(c("a") > 0).then(c("y")).count().alias("c1"),
                                   pl.when(c("flag")).then(None).otherwise(c("b")).count().alias("c2"), pl.when(c("flag")).then(None).otherwise(c("b")).max().alias("mx"))
    prog = q.debug_program()
    assert not has_select(prog) and any(op[0] == pe.OP_MASKV for op in prog["ops"])
    got = by_key(pe.evaluate(prog, cols), ["k"])
    (a, am), (b, bm), (y, ym), flag, (k, _) = (full(cols, nm) for nm in ("a", "b", "y", "flag", "k"))
    v1, m1 = where((a > 0, am), (y, ym), lit_col(n, 0.0, False))
    v2, m2 = where(flag, lit_col(n, 0, False), (b, bm))
    for kv in range(5):
        g, rows = got[(kv,)], k == kv
        assert close(g["s"], float(v1[rows & m1].sum())) and g["c1"] == int((rows & m1).sum()) and g["c2"] == int((rows & m2).sum()) and g["mx"] == int(v2[rows & m2].max())
    # a constant predicate folds to the chosen branch
    prog = df.lazy().select(pl.when(pl.lit(True)).then(c("b")).otherwise(c("a")).sum().alias("s")).debug_program()
    assert [op[0] for op in prog["ops"]] == [pe.OP_LOAD] and [i["name"] for i in prog["inputs"]] == ["b"]


def test_a_predicate_whose_operand_has_its_last_use_in_the_select(data, pe):
    """when(b > 0).then(b).otherwise(...): the load of b is read by the compare AND by the select.  A use count that forgets one of the select's three sources frees
    the slot after the compare, and the constant that follows overwrites the then value.  Likewise the compare's result is read by nothing but the select."""
    cols, df = data
    n = len(cols["k"][0])
    for agg in ("sum", "max"):
        e = pl.when(c("b") > 0).then(c("b")).otherwise(c("i32").cast(pl.Int64) * 3)
        q = df.lazy().filter(c("k") < 4).select(getattr(e, agg)().alias("r"), pl.when(c("flag")).then(c("flag")).otherwise(c("a") > 0).sum().alias("t"))
        prog = q.debug_program()
        assert sum(op[0] == pes.OP_SELECT for op in prog["ops"]) == 2
        got = pe.evaluate(prog, cols)
        (a, am), (b, bm), flag, (k, _), (i32, _) = (full(cols, nm) for nm in ("a", "b", "flag", "k", "i32"))
        rv, rm = where((b > 0, bm), (b, bm), (i32.astype(np.int64) * 3, np.ones(n, bool)))
        tv, tm = where(flag, flag, (a > 0, am))
        keep = k < 4
        assert got["r"][0][0] == (rv[keep & rm].sum() if agg == "sum" else rv[keep & rm].max()) and got["t"][0][0] == int((keep & tm & tv).sum())


def test_split_keeps_a_predicate_that_feeds_only_a_late_select(data, pe):
    cols, df = data
    q = df.lazy().filter(c("k") < 3).select(pl.when(c("a") > 0).then(c("x")).otherwise(c("y")).sum().alias("s"), pl.len().alias("n"))
    prog = q.debug_program()
    sel = [i for i, op in enumerate(prog["ops"]) if op[0] == pes.OP_SELECT]
    assert len(sel) == 1 and prog["any_late"] == 1 and not (prog["early_mask"] >> sel[0]) & 1
    cmp_pc = [i for i, op in enumerate(prog["ops"]) if op[1] == prog["ops"][sel[0]][4] and i < sel[0]][-1]      # the producer of the select's predicate slot
    assert not (prog["early_mask"] >> cmp_pc) & 1          # nothing early needs it
    assert pe.split_matches(prog, cols)
    got = pe.evaluate(prog, cols)
    (a, am), (x, xm), (y, ym), (k, _) = (full(cols, nm) for nm in ("a", "x", "y", "k"))
    sv, sm = where((a > 0, am), (x, xm), (y, ym))
    assert math.isclose(got["s"][0][0], sv[(k < 3) & sm].sum(), rel_tol=1e-9) and got["n"][0][0] == int((k < 3).sum())


def test_the_run_time_compiled_kernel_builds(data):
    _, df = data
    df.lazy().filter(pl.when(c("flag")).then(c("a")).otherwise(c("b")) > 3).select(pl.when(c("a") > 0).then(c("x")).otherwise(0.0).sum().alias("s")).jit_selftest()


def test_float32_branches_stay_with_the_per_node_kernels():
    rng = np.random.default_rng(1)
    cols = {"f": (rng.normal(size=100).astype(np.float32), None), "p": (rng.random(100) < 0.5, None)}
    df = frame_like(cols, {"f": pl.Float32})
    fusable, _, why, _ = df.lazy().select(pl.when(c("p")).then(c("f")).otherwise(0.0).sum().alias("s")).describe_fusion()
    assert not fusable and "f32" in why


# ---- the Polars attachment ----------------------------------------------------------------------------------------------------------
Ternary = _cls("Ternary", "predicate", "truthy", "falsy")


class TernaryTraverser(FakeTraverser):
    def view_expression(self, i):
        d = self.low.aexprs[i]
        if d["kind"] == F.AE_TERNARY:
            return Ternary(predicate=d["cond"], truthy=d["lhs"], falsy=d["rhs"])
        return super().view_expression(i)


def canonical(low, root):
    def ex(i):
        if i < 0:
            return None
        d = low.aexprs[i]
        return (d["kind"], d["op"], ex(d["lhs"]), ex(d["rhs"]), ex(d["cond"]), d["dtype"], d["is_null"], d["lit"] if d["kind"] == F.AE_LITERAL and not d["is_null"] else None, d["name"])
    def ir(i):
        d = low.irs[i]
        return (d["kind"], ir(d["input"]) if d["input"] >= 0 else None, ex(d["predicate"]), tuple(ex(e) for e in d["exprs"]), tuple(ex(e) for e in d["keys"]))
    return ir(root)


def test_the_shim_translates_a_ternary_node(data):
    _, df = data
    lf = (df.lazy().filter(pl.when(c("flag")).then(c("a")).otherwise(c("b")) > 3).group_by("k")
          .agg(pl.when(c("a") > 0).then(c("x")).otherwise(0.0).sum().alias("s"), pl.when(c("flag")).then(c("i32")).count().alias("n")))
    low, root, _ = lf._lower()
    back = eng.Translator(TernaryTraverser(low, root), frame_of=lambda node: node.df).plan()
    low2, root2, _ = back._lower()
    assert canonical(low, root) == canonical(low2, root2)
    nt = TernaryTraverser(low, root)
    eng.execute_with_amd(nt, None, frame_of=lambda node: node.df)
    assert nt.udf is not None and nt.get_node() == root

    class NoFalsy(TernaryTraverser):
        def view_expression(self, i):
            x = super().view_expression(i)
            if type(x).__name__ == "Ternary":
                del x.falsy
            return x
    with pytest.raises(eng.NotSupported, match="Ternary"):
        eng.execute_with_amd(NoFalsy(low, root), None, raise_on_fail=True, frame_of=lambda node: node.df)
    nt2 = NoFalsy(low, root)
    eng.execute_with_amd(nt2, None, frame_of=lambda node: node.df)
    assert nt2.udf is None and nt2.get_node() == root
