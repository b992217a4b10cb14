"""var / std without a GPU: the arithmetic of csrc/variance.hpp as a stand-alone program under -fsanitize=address,undefined against a two-pass computation; the
mirror API and its lowering (kinds 7 / 8 with ddof in the literal slot, output dtypes, the refusals); the fused programs the C++ compiler emits for queries that
carry the two aggregates (three cells per source, whatever number of var / std / ddof read it), interpreted row by row in numpy (tests/program_eval_var.py adds the
two finalisation kinds to tests/program_eval.py) against np.var within the accuracy contract of DESIGN.md 4.14 with the pivot 0 a compile without a device uses; the
post_opt_callback shim; the sharded operators' refusal; the registers of the per-node kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import dist
from polars_amd import polars_engine as eng
from tests import program_eval as pe
from tests import program_eval_var as pv
from tests import test_polars_engine_cpu as TE
from tests.test_program_eval_cpu import by_key, frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_under_sanitizers_against_a_two_pass_computation(tmp_path):
    """tests/emu/variance_main.cpp: merge against a two-pass sum over random splits (with and without an offset of 1e15), the n <= ddof rule, the clamp, NaN / inf."""
    exe = str(tmp_path / "variance_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "variance_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 20_000, r.stdout


# ---- the mirror API and its lowering ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(414)
    n = 3001
    cols = {"k": (rng.integers(0, 7, n).astype(np.int64), None),
            "x": (rng.normal(3.0, 2.0, n), None),
            "xn": (rng.normal(-1.0, 0.5, n), rng.random(n) < 0.7),
            "a": (rng.integers(-300, 300, n).astype(np.int64), None), "b": (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) < 0.9),
            "i": (rng.integers(-1000, 1000, n).astype(np.int32), None), "u": (rng.integers(0, 60000, n).astype(np.uint16), None),
            "f": (rng.normal(size=n).astype(np.float32), None),
            "flag": (rng.random(n) < 0.5, None), "d": (rng.integers(8000, 11000, n).astype(np.int32), None), "t": (rng.integers(0, 1 << 40, n).astype(np.int64), None),
            "s": (rng.integers(0, 3, n).astype(np.uint8), None)}
    dtypes = {"d": pl.Date, "t": pl.Datetime, "s": pl.Categorical(["A", "N", "R"], pl.UInt8), "f": pl.Float32}
    return cols, frame_like(cols, dtypes)


def full(cols, name):
    v, m = cols[name]
    return v, np.ones(len(v), bool) if m is None else m


def lowered(df, expr):
    low, root, schema = df.lazy().select(expr)._lower()
    return low, low.aexprs[low.irs[root]["exprs"][0]], schema


def test_expr_api_and_ddof_check():
    assert repr(c("x").var()) == "col('x').var(ddof=1)" and repr(pl.std("x", 0)) == "col('x').std(ddof=0)"
    e = c("x").std(ddof=3)
    assert (e.kind, e.op, e.value) == ("agg", F.AGG_STD, 3) and F.AGG_VAR == 7 and F.AGG_STD == 8
    assert pl.var("x").op == F.AGG_VAR and pl.var("x").value == 1 and c("x").var(np.int64(2)).value == 2 and c("x").var(255).value == 255
    for bad in (1.0, -1, 256, True, "1", None):
        for fn in (c("x").var, c("x").std):
            with pytest.raises(TypeError, match="integer 0..255"):
                fn(bad)


def test_arena_node_output_dtype_and_name(data):
    _, df = data
    for col, out in (("x", pl.Float64), ("i", pl.Float64), ("u", pl.Float64), ("a", pl.Float64), ("f", pl.Float32)):
        for kind, fn, ddof in ((7, "var", 0), (8, "std", 1), (7, "var", 5)):
            low, top, schema = lowered(df, getattr(c(col), fn)(ddof))
            assert list(schema.items()) == [(col, out)]                         # Float64 (Float32 stays), named like the source column
            assert top["kind"] == F.AE_AGG and top["op"] == kind and top["lit"] == ddof and low.aexprs[top["lhs"]]["kind"] == F.AE_COLUMN
    low, top, schema = lowered(df, (c("a") * c("b")).var().alias("ab"))
    assert schema == {"ab": pl.Float64} and low.aexprs[top["lhs"]]["op"] == F.AGG_VAR and low.aexprs[low.aexprs[top["lhs"]]["lhs"]]["kind"] == F.AE_BINARY


def test_refusals_name_the_dtype(data):
    _, df = data
    for col, name in (("flag", "Boolean"), ("d", "Date"), ("t", "Datetime"), ("s", "Categorical")):
        for fn in ("var", "std"):
            with pytest.raises(TypeError, match=f"{fn}\\(\\) needs a numeric expression, got {name}"):
                lowered(df, getattr(c(col), fn)())
    with pytest.raises(TypeError, match="Boolean"):
        df.lazy().group_by("k").agg((c("x") > 0).std())._lower()


def test_the_node_crosses_the_abi_with_ddof_in_the_literal_slot(data, tmp_path):
    _, df = data
    low, root, _ = df.lazy().group_by("k").agg(c("x").var(0).alias("v0"), c("i").std(3).alias("s3"), c("x").mean().alias("m"))._lower()
    ir, n_ir, ae, n_ae, keep = low.to_c()
    seen = []
    for i, d in enumerate(low.aexprs):
        if d["kind"] == F.AE_AGG and d["op"] in (F.AGG_VAR, F.AGG_STD):
            seen.append((ae[i].op, ae[i].lit.u))
            assert ae[i].kind == F.AE_AGG and ae[i].lhs == d["lhs"] and ae[i].cond == -1
    assert seen == [(7, 0), (8, 3)]
    assert C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr._fields_[-1][0] == "cond"      # plx_aexpr is what it was
    src = tmp_path / "var.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AGG_FIRST == 6 && PLX_AGG_VAR == 7 && PLX_AGG_STD == 8, "plx_agg_op numbering");
_Static_assert(sizeof(plx_aexpr) == 48, "plx_aexpr did not grow");
int (*p1)(plx_column, int32_t, int32_t, plx_scalar*, plx_dtype*, int32_t*) = plx_reduce_var;
int (*p2)(const plx_column*, int32_t, const plx_column*, const plx_agg_op*, int32_t, int32_t, const int32_t*, plx_column*, plx_column*) = plx_groupby_agg_ddof;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "var.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the importer checks ddof before anything needs a device; a Boolean operand is refused by dtype inference with its name
    buf = C.create_string_buffer(1 << 14)
    low, root, _ = df.lazy().select(c("x").var())._lower()
    [d for d in low.aexprs if d["kind"] == F.AE_AGG][0]["lit"] = 256
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) == 1 and "ddof 0..255" in F.lib().plx_last_error().decode()
    low, root, _ = df.lazy().select(c("flag").sum())._lower()
    agg = [d for d in low.aexprs if d["kind"] == F.AE_AGG][0]
    agg["op"], agg["lit"] = F.AGG_STD, 1
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) == F.ERR_UNSUPPORTED
    assert "std of a bool" in F.lib().plx_last_error().decode().lower(), F.lib().plx_last_error().decode()
    for name in ("plx_reduce_var", "plx_groupby_agg_ddof", "_polars_plugin_plx_var", "_polars_plugin_field_plx_var", "_polars_plugin_plx_std", "_polars_plugin_field_plx_std"):
        assert hasattr(F.lib(), name), name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(w in text for w in ("plx_var", "plx_std", "plx_reduce_var", "plx_groupby_agg_ddof"))


def test_plugin_fields_and_entry_points_without_a_device():
    import pyarrow as pa
    import torch

    from tests import plugin_abi as P
    for name in ("plx_var", "plx_std"):
        assert P.field(name, pa.int32(), {"ddof": 0}).type == pa.float64() and P.field(name, pa.float32()).type == pa.float32() and P.field(name, pa.float64(), col_name="x").name == "x"
    if torch.cuda.is_available():
        return
    res, inp = P.call("plx_std", [pa.array([1.0, 2.0])], {"ddof": 1})
    assert res is None and inp.released == 1 and ("no HIP device" in P.last_error() or "plx_init" in P.last_error())
    h = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.F64, 100, 0, 0, 0, 0, C.byref(h)) == 0
    v, dt, ok = F.Scalar(), C.c_int32(), C.c_int32()
    assert F.lib().plx_reduce(F.AGG_VAR, h.value, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "plx_reduce_var" in F.lib().plx_last_error().decode()
    assert F.lib().plx_reduce(F.AGG_STD, h.value, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "plx_reduce_var" in F.lib().plx_last_error().decode()
    assert F.lib().plx_reduce_var(h.value, 256, 0, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "ddof" in F.lib().plx_last_error().decode()
    hb = C.c_uint64()
    assert F.lib().plx_column_placeholder(F.BOOL, 100, 0, 0, 0, 0, C.byref(hb)) == 0
    assert F.lib().plx_reduce_var(hb.value, 1, 0, C.byref(v), C.byref(dt), C.byref(ok)) == F.ERR_UNSUPPORTED and "bool" in F.lib().plx_last_error().decode().lower()


# ---- the fused programs, row by row ---------------------------------------------------------------------------------------------------------
def test_var_std_and_two_ddof_over_one_source_are_three_cells(data):
    _, df = data
    q = df.lazy().select(c("x").var().alias("v1"), c("x").std().alias("s1"), c("x").var(0).alias("v0"), c("x").std(2).alias("s2"))
    prog = q.debug_program()
    assert len(prog["aggs"]) == 3 and sorted(k for k, _ in prog["aggs"]) == [pe.AGG_SUM_F, pe.AGG_SUM_F, pe.AGG_LEN]      # sum d, sum d^2, the rows (x has no nulls)
    assert [(f["kind"], f["ddof"]) for f in prog["finals"]] == [(pv.FIN_VAR, 1), (pv.FIN_STD, 1), (pv.FIN_VAR, 0), (pv.FIN_STD, 2)]
    assert len({(f["a"], f["b"], f["c"]) for f in prog["finals"]}) == 1 and all(f["out_dtype"] == pe.F64 for f in prog["finals"])
    codes = [op[0] for op in prog["ops"]]
    assert codes == [pe.OP_LOAD, pe.OP_CONST, pe.OP_SUB_F, pe.OP_MUL_F]                               # no new opcode: d = x - p, q = d * d
    assert float(np.uint64(int(prog["ops"][1][5])).view(np.float64)) == 0.0                              # compiled without a device: the pivot is 0
    # a nullable source counts its own valid rows, and the mean beside it reads the same count cell
    prog = df.lazy().group_by("k").agg(c("xn").std().alias("s"), c("xn").mean().alias("m"), c("xn").var(0).alias("v")).debug_program()
    kinds = sorted(k for k, _ in prog["aggs"])
    assert kinds == sorted([pe.AGG_LEN, pe.AGG_SUM_F, pe.AGG_SUM_F, pe.AGG_COUNT, pe.AGG_SUM_F])      # group len, sum d, sum d^2, count, the mean's sum
    fs, fm = prog["finals"][0], prog["finals"][1]
    assert fs["kind"] == pv.FIN_STD and fm["kind"] == pe.FIN_MEAN and fs["b"] == fm["b"]


def check_groups(got, keys, mask, x, ddof_of, D, f32=False):
    """got: by_key result; every group of `keys` over the rows of `mask` against numpy within the contract"""
    n_checked = 0
    for kv in np.unique(keys[mask]):
        g = got[(int(kv),)]
        for name, (ddof, is_std, valid) in ddof_of.items():
            xs = x[mask & valid & (keys == kv)].astype(np.float64)
            assert pv.within_contract(g[name], xs, ddof, D, want_std=is_std, f32=f32), (int(kv), name, g[name], np.var(xs, ddof=ddof) if len(xs) > ddof else None)
            n_checked += 1
    return n_checked


def test_programs_match_numpy_within_the_contract(data):
    cols, df = data
    (k, _), (x, _), (xn, xnm), (a, _), (b, bm), (i, _) = (full(cols, nm) for nm in ("k", "x", "xn", "a", "b", "i"))
    ones = np.ones(len(k), bool)
    # group-by: a plain column, an integer column, a product, a nullable source; the pivot is 0, so D = max |source|
    aggs = [c("x").var().alias("xv"), c("x").std(0).alias("xs"), c("i").var().alias("iv"), (c("a") * c("b")).var(0).alias("abv"), c("xn").std().alias("xns"), c("xn").var(3).alias("xnv")]
    prog = df.lazy().group_by("k").agg(*aggs).debug_program()
    got = by_key(pv.evaluate(prog, cols), ["k"])
    ab = (a * b).astype(np.float64)
    spec = [(x, {"xv": (1, False, ones), "xs": (0, True, ones)}), (i.astype(np.float64), {"iv": (1, False, ones)}), (ab, {"abv": (0, False, bm)}),
            (xn, {"xns": (1, True, xnm), "xnv": (3, False, xnm)})]
    for src, names in spec:
        valid = list(names.values())[0][2]
        assert check_groups(got, k, ones, src, names, float(np.abs(src[valid]).max())) == 7 * len(names)
    # the same under a predicate (rows with x > 2.5), and with a group the predicate empties
    keep = (x > 2.5) & (k != 3)
    prog = df.lazy().filter((c("x") > 2.5) & (c("k") != 3)).group_by("k").agg(*aggs).debug_program()
    got = by_key(pv.evaluate(prog, cols), ["k"])
    assert set(got) == {(j,) for j in range(7) if j != 3}
    for src, names in spec:
        valid = list(names.values())[0][2]
        check_groups(got, k, keep, src, names, float(np.abs(src[valid]).max()))
    assert pe.split_matches(prog, cols)
    # whole-column select, with and without a filter
    for filt, mask in ((None, ones), (c("i") < 0, i < 0)):
        lf = df.lazy() if filt is None else df.lazy().filter(filt)
        prog = lf.select(c("x").var().alias("xv"), c("xn").std(0).alias("xns"), (c("a") * c("b")).std().alias("abs"), c("i").var(2).alias("iv")).debug_program()
        got = pv.evaluate(prog, cols)
        one = lambda nm: None if not got[nm][1][0] else float(got[nm][0][0])
        assert pv.within_contract(one("xv"), x[mask], 1, float(np.abs(x).max()))
        assert pv.within_contract(one("xns"), xn[mask & xnm], 0, float(np.abs(xn[xnm]).max()), want_std=True)
        assert pv.within_contract(one("abs"), ab[mask & bm], 1, float(np.abs(ab[bm]).max()), want_std=True)
        assert pv.within_contract(one("iv"), i[mask].astype(np.float64), 2, float(np.abs(i).max()))


def test_nulls_small_groups_nan_and_inf_in_the_interpreter():
    rng = np.random.default_rng(5)
    k = np.array([0, 0, 0, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5], dtype=np.int64)
    x = rng.normal(size=len(k))
    valid = np.ones(len(k), bool)
    valid[[4, 5]] = False                      # group 2: every value null
    x[7] = np.nan                              # group 3: a NaN
    x[10] = np.inf                             # group 4: an infinity
    x[12] = x[13] = 2.5                        # group 5: constant
    cols = {"k": (k, None), "x": (x, valid)}
    prog = frame_like(cols).lazy().group_by("k").agg(c("x").var().alias("v1"), c("x").var(0).alias("v0"), c("x").std(2).alias("s2")).debug_program()
    got = by_key(pv.evaluate(prog, cols), ["k"])
    assert got[(1,)] == {"v1": None, "v0": 0.0, "s2": None}                    # one row: null at ddof 1, 0.0 at ddof 0
    assert got[(2,)] == {"v1": None, "v0": None, "s2": None}                   # all null
    assert got[(3,)] == {"v1": "nan", "v0": "nan", "s2": "nan"} and got[(4,)] == {"v1": "nan", "v0": "nan", "s2": "nan"}
    assert got[(5,)] == {"v1": 0.0, "v0": 0.0, "s2": None}
    assert pv.within_contract(got[(0,)]["v1"], x[:3], 1, 3.0) and pv.within_contract(got[(0,)]["s2"], x[:3], 2, 3.0, want_std=True)


# ---- the post_opt_callback shim and the sharded operators ----------------------------------------------------------------------------------
class VarTraverser(TE.FakeTraverser):
    """the stand-in NodeTraverser, showing var / std the way visitor/expr_nodes.rs does: Agg(name, arguments, options = ddof)"""
    def view_expression(self, i):
        d = self.low.aexprs[i]
        if d["kind"] == F.AE_AGG and d["op"] in (F.AGG_VAR, F.AGG_STD):
            return TE.Agg(name="var" if d["op"] == F.AGG_VAR else "std", arguments=[d["lhs"]], options=d["lit"])
        return super().view_expression(i)


def test_the_shim_maps_std_and_var_and_still_refuses_median():
    li, _ = TE.frames()
    lf = li.lazy().filter(c("l_quantity") > 3).group_by("l_returnflag").agg(c("l_tax").std(0).alias("sd0"), c("l_extendedprice").var().alias("v"), c("l_quantity").std(2).alias("q"))
    low, root, _ = lf._lower()
    back = eng.Translator(VarTraverser(low, root), frame_of=lambda node: node.df).plan()
    low2, root2, _ = back._lower()
    lits = lambda lw: [(d["op"], d["lit"]) for d in lw.aexprs if d["kind"] == F.AE_AGG]
    assert TE.canonical(low, root) == TE.canonical(low2, root2) and lits(low2) == [(F.AGG_STD, 0), (F.AGG_VAR, 1), (F.AGG_STD, 2)]
    exprs = {0: TE.Column(name="l_tax"), 1: TE.Agg(name="std", arguments=[0], options=0), 2: TE.Agg(name="median", arguments=[0], options=None),
             3: TE.Agg(name="var", arguments=[0], options=300)}
    tr = eng.Translator(TE.MapTraverser({}, exprs, 0))
    e = tr.expr(1)
    assert (e.kind, e.op, e.value) == ("agg", F.AGG_STD, 0)
    with pytest.raises(eng.NotSupported, match="aggregation median"):
        tr.expr(2)
    with pytest.raises(eng.NotSupported, match="0..255"):
        tr.expr(3)


def test_sharded_group_by_refuses_by_name():
    """dist.py refused unknown aggregates by name before var / std existed; this pins that the two new names get that ValueError, not a KeyError (it passes without the feature)."""
    for op in ("std", "var"):
        with pytest.raises(ValueError, match=op):
            dist.GroupBySpec("k", [("o", "v", op)])
        with pytest.raises(ValueError, match=op):
            dist.JoinGroupBySpec("pk", "bk", "pk", [("o", op)])


def test_h2o_sd_example_lowers_and_compiles():
    from polars_amd import queries as Q
    rng = np.random.default_rng(9)
    n = 2000
    cols = {"id4": (rng.integers(1, 9, n).astype(np.int32), None), "id5": (rng.integers(1, 5, n).astype(np.int32), None), "v3": (rng.uniform(0, 100, n), None)}
    prog = Q.h2o_sd(frame_like(cols).lazy()).debug_program()
    res = pv.evaluate(prog, cols)
    got = by_key(res, ["id4", "id5"])
    assert len(got) == 32
    for (a, b), g in got.items():
        xs = cols["v3"][0][(cols["id4"][0] == a) & (cols["id5"][0] == b)]
        assert pv.within_contract(g["v3_sd"], xs, 1, 100.0, want_std=True) and abs(g["v3_mean"] - xs.mean()) < 1e-9


# ---- the per-node kernels' registers ---------------------------------------------------------------------------------------------------------
def test_var_kernels_use_no_scratch():
    """var_kernel<T> (ten dtypes), var_pivot_kernel<T> and var_finish_kernel: VGPRs and scratch bytes as tests/test_kernel_resources_cpu.py obtains them."""
    from tests.test_kernel_resources_cpu import resource_usage
    res = {n: r for n, r in resource_usage("kernels_reduce.hip").items() if "var_kernel" in n or "var_finish_kernel" in n or "var_pivot_kernel" in n}
    assert sum("var_kernel" in n for n in res) == 10 and sum("var_pivot_kernel" in n for n in res) == 10 and sum("var_finish_kernel" in n for n in res) == 1, sorted(res)
    for name, r in sorted(res.items()):
        print(name, "VGPRs", r["VGPRs"], "scratch", r["ScratchSize [bytes/lane]"], "LDS", r["LDS Size [bytes/block]"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r)          # eight waves per SIMD, as reduce_kernel
