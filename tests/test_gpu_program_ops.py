"""Every opcode of the fused register program that ordinary queries are made of, row by row on the device, at the values where such code goes wrong.

The tables, the reference and the read-out are tests/expr_rows.py (pinned without a GPU by tests/test_expr_rows_cpu.py): group_by("row") makes every row a group of
its own, so min() / sum() / count() of an expression hand back that row's value and validity.  Each query runs three ways -- the generic interpreter
(fused_device.hpp run_program<DynProg>: prefetch_inputs / store_prefetched for inputs 0..7, load_input for 8 and 9), the run-time compiled kernel, and the per-node
kernels (no_fusion) -- and every row of every expression is compared with the reference: validity, integers and Booleans exactly, f64 as bit patterns (a NaN for a
NaN).  There is no tolerance: the library and the run-time compiler build with -ffp-contract=off, so each result is one correctly rounded IEEE operation or a chain of
them.  Every table is run at its full (odd) length and cut to 1, 127, 128, 129 and full - 1 rows; the cuts are views of one upload, so a query is one compiled kernel.
A fused mode that does not report its kernel kind in the plan fails: nothing here may pass by falling back."""
import functools
import math

import numpy as np
import pytest

from tests import expr_rows as R
from tests import expr_trees

pytestmark = pytest.mark.gpu

# the random trees of tests/test_program_eval_cpu.py: seeds 0..39, and the ones of them whose query compiles to one fused program
# (tests/test_expr_rows_cpu.py::test_which_random_trees_fuse recomputes this list without a GPU).  28 of the 40 fuse -- five are longer than 32 ops, seven
# aggregate a bare literal -- so seeds 40..42 are added, with which 30 do.
TREE_SEEDS = list(range(43))
FUSING_SEEDS = [0, 1, 2, 3, 5, 7, 8, 9, 12, 14, 16, 17, 20, 21, 22, 23, 24, 25, 27, 28, 29, 30, 31, 32, 35, 36, 37, 39, 40, 42]
JIT_SEEDS = FUSING_SEEDS[:6]


@pytest.fixture(scope="module")
def device_table(pl):
    cache = {}
    def get(table):
        if table.name not in cache:
            cache[table.name] = R.DeviceTable(pl, table)
        return cache[table.name]
    return get


@functools.lru_cache(maxsize=None)
def want(name, n):
    case = R.CASES[name]
    return R.reference(case.exprs, case.table.head(n))


def run_case(pl, device_table, name):
    """the case's program in all three modes at every length of its table, each against the reference"""
    case = R.CASES[name]
    dev = device_table(case.table)
    compiled = None
    for n in reversed(case.table.sizes()):
        frame = dev.frame(n)
        for mode in R.MODES:
            R.compare(R.observe(pl, frame, case.exprs, mode), want(name, n), (name, n, mode))
        if compiled is None:
            compiled = pl._ffi.jit_stats()[0]
    assert pl._ffi.jit_stats()[0] == compiled, (name, "a shorter table compiled a kernel of its own")


@pytest.mark.parametrize("name", ["i64_ints", "i64_int_literals", "i64_floats", "i64_null_heads_ints", "i64_null_heads_int_literals", "i64_null_heads_floats"])
def test_i64_arithmetic_and_division(pl, device_table, name):
    """OP_ADD_I / SUB_I / MUL_I wrapping, OP_FDIV_I / OP_MOD_I on both divide paths, OP_I2F + OP_DIV_F, col / literal as a multiplication by the reciprocal.
    Named rows of the plain table (regressions are read off them): rows 0..127 all lanes narrow (32-bit divide, zero divisors among them); rows 128 + 61 and 128 + 90
    the two wide lanes that send tile 1 down the 64-bit routine; from row 256 the cross product of expr_rows.E_I64, INT64_MIN // -1 at its row 7.  The second table
    has its nulls on wide values in tiles 0 and 1 (row 0: INT64_MIN // -1 under two nulls).  (The division programs are what takes time here: the run-time compiler
    needs seconds for a kernel with 64-bit divisions in it.)"""
    run_case(pl, device_table, name)
    if name != "i64_ints":
        return
    # the two first tiles of the plain table give the same answers on the 126 rows they share, whichever divide ran
    frame = device_table(R.i64_table(False)).frame(2 * R.TILE)
    same = np.ones(R.TILE, bool)
    same[[R.WIDE_A_ROW, R.WIDE_B_ROW]] = False
    for mode in R.MODES:
        got = R.observe(pl, frame, R.CASES["i64_ints"].exprs, mode)
        for label, (v, m) in got.items():
            assert np.array_equal(m[:R.TILE][same], m[R.TILE:][same]) and np.array_equal(v[:R.TILE][same & m[:R.TILE]], v[R.TILE:][same & m[:R.TILE]]), (mode, label)


@pytest.mark.parametrize("name", ["u64_ints", "u64_int_literals", "u64_floats"])
def test_u64_arithmetic_division_and_conversion(pl, device_table, name):
    """OP_FDIV_U / OP_MOD_U, wrapping + - *, OP_U2F at and above 2^63 (2^64 - 1 rounds to 2^64)"""
    run_case(pl, device_table, name)


def test_f64_arithmetic(pl, device_table):
    """+ - * / over infinities, denormals, signed zeros, NaNs and overflow to infinity; a / 4.0 and a * 2.0 + 1.0 (no contraction); fill_null(2.5)"""
    for name in ("f64_binary", "f64_literals"):
        run_case(pl, device_table, name)


COMPARISONS = {"i64": ("cmp_i64", "cmp_i64_lit"), "u64": ("cmp_u64", "cmp_u64_lit"), "f64": ("cmp_f64", "cmp_f64_nan", "cmp_f64_negzero")}
assert {n for ns in COMPARISONS.values() for n in ns} == {n for n, _ in R.FILTER_PREDICATES}


@pytest.mark.parametrize("cls", list(COMPARISONS))
def test_comparisons_i64_u64_f64(pl, device_table, cls):
    """The six operators per class, column against column and against a literal at an edge (2^31, 2^63 as UInt64, NaN, -0.0): OP_CMP_I / OP_CMP_U / OP_CMP_F with the
    float total order (NaN equals NaN and is greatest, -0.0 equals 0.0).  Read out through sum / count, and a second time through the filter-to-frame pipeline:
    filter(e) keeps the rows where e is valid and true, filter(~e) the rows where it is valid and false.  Every predicate goes through the filter in the generic
    interpreter and per node; a predicate and its negation are a compiled kernel each, so the run-time compiler takes the ones of expr_rows.FILTER_JIT."""
    for name in COMPARISONS[cls]:
        run_case(pl, device_table, name)
    for name, label in R.FILTER_PREDICATES:
        if name not in COMPARISONS[cls]:
            continue
        case = R.CASES[name]
        x = dict(case.exprs)[label]
        dev = device_table(case.table)
        for n in (case.table.n, R.TILE + 1, 1):
            v, m = want(name, n)[label]
            rows = np.arange(n)
            for mode in R.MODES:
                if mode == "jit" and (name, label) not in R.FILTER_JIT:
                    continue
                kept, dropped = R.observe_filter(pl, dev.frame(n), x, mode)
                assert np.array_equal(kept, rows[m & v]) and np.array_equal(dropped, rows[m & ~v]), (name, label, n, mode)


def test_kleene_logic_and_null_tests(pl, device_table):
    """OP_AND / OP_OR (Kleene), OP_XOR, OP_NOT, is_null / is_not_null, fill_null (OP_IFNULL) and a three-deep mix over all nine (true / false / null)^2
    combinations, each at even and odd rows, around the edges of a validity word and in the last partial tile"""
    for name in ("kleene_binary", "kleene_nulls"):
        run_case(pl, device_table, name)


LOAD_CASES = {"ten_inputs_first_order": ["loads_a"], "ten_inputs_second_order": ["loads_b1", "loads_b2"], "signed_against_a_literal": ["cmp_i8_lit", "cmp_i16_lit", "cmp_i32_lit"],
              "unsigned_against_a_literal": ["cmp_u8_lit", "cmp_u16_lit", "cmp_u32_lit"]}
assert sorted(n for ns in LOAD_CASES.values() for n in ns) == sorted(list(R.LOAD_PROGRAMS) + [f"cmp_{k}_lit" for k in R.NARROW_LITS])


@pytest.mark.parametrize("which", list(LOAD_CASES))
def test_input_loads_every_dtype_in_both_load_paths(pl, device_table, which):
    """Ten-input programs (the row id and nine columns) in two column orders: the sum of all columns as f64 and a min per column, so a wrong extension of one column
    cannot cancel against another.  Inputs 8 and 9 (u16, i8 in one order, i32, u32 in the other) take load_input in the generic interpreter, the others
    prefetch_inputs / store_prefetched; the compiled kernel and the per-node kernels load them their own ways.  Then each narrow dtype against a literal of its own."""
    for name in LOAD_CASES[which]:
        run_case(pl, device_table, name)


def test_narrow_integer_arithmetic_stays_per_node_and_wraps(pl, device_table):
    """What the compiler leaves to the per-node kernels on purpose: + - * on dtypes narrower than 64 bits wrap at the column's width (numpy's fixed-width arithmetic
    is the reference), float // and % are floor(a / b) and a - b * floor(a / b) (polars-utils floor_divmod.rs, kernels_elementwise.hip floor_divmod)."""
    loads, floats = R.load_table(), R.f64_table()
    for label, k, sym in R.NON_FUSABLE:
        table = floats if k is None else loads
        out = R.non_fusable_query(pl, device_table(table).frame(table.n), label).collect()
        plan = pl.last_plan()          # the reason, then a group-by over the column the per-node kernels materialised: its scan holds the loads and nothing else
        assert plan.startswith("(not fused: " + ("float floor-div / mod" if k is None else f"arithmetic on {k} wraps at the column width")) and R.per_node_plan(plan), (label, plan)
        got = dict(zip(out.columns, out._download_all()))
        order = np.argsort(got["row"][0], kind="stable")
        assert np.array_equal(got["row"][0][order], np.arange(table.n))
        gv, gm = got["v"][0][order], (np.ones(table.n, bool) if got["v"][1] is None else got["v"][1][order])
        with np.errstate(all="ignore"):
            if k is None:
                (a, va), (b, vb) = table.cols["a"], table.cols["b"]
                d = np.floor(a / b)
                wv, wm = (d if sym == "//" else a - b * d), va & vb
            else:
                v, wm = table.cols[k]
                wv = R._PY[sym](v, np.array(R.NARROW_PARTNER[k], dtype=v.dtype))
                assert wv.dtype == v.dtype
        R.compare({"v": (gv, gm)}, {"v": (wv, wm)}, label)


def check_tree(d, pred, ftree, itree, where):
    """the assertions of tests/test_program_eval_cpu.py::test_random_expression_trees: counts and integers exact, 1e-9 relative on the float sum and the mean"""
    close = lambda a, b: a == b or math.isclose(a, b, rel_tol=1e-9, abs_tol=1e-12)
    (pv, pm), (fv, fm), (iv, im) = pred[1], ftree[1], itree[1]
    keep = pv & pm
    # A tree that is a bare literal: select(lit(k).sum()) aggregates a one-row literal whatever the filter keeps -- sum k, count 1, min / max / mean k (the reference
    # evaluates a literal to a unit-length series and does not broadcast it in front of an aggregation; so does the per-node evaluator, engine.cpp eval PLX_AE_AGG).
    # The generator's numpy evaluation repeats the literal on every row, which is right for a literal inside a larger tree only.
    if ftree[0].kind == "lit":
        fv, fm, fkeep = fv[:1], fm[:1], np.ones(1, bool)
    else:
        fkeep = keep
    if itree[0].kind == "lit":
        iv, im, ikeep = iv[:1], im[:1], np.ones(1, bool)
    else:
        ikeep = keep
    assert d["n"][0] == int(keep.sum()), where
    fsel = fkeep & fm
    assert d["fc"][0] == int(fsel.sum()), where
    with np.errstate(all="ignore"):
        want_fs = float(fv[fsel].sum())
    assert (math.isnan(want_fs) and math.isnan(d["fs"][0])) or close(float(d["fs"][0]), want_fs), (where, d["fs"][0], want_fs)
    ford = fsel & ~np.isnan(fv)
    if not fsel.any():
        assert d["fmin"][0] is None, where
    elif not ford.any():
        assert math.isnan(d["fmin"][0]), where
    else:
        assert d["fmin"][0] == fv[ford].min(), where
    isel = ikeep & im
    assert d["isum"][0] == int(iv[isel].sum()), where
    if isel.any():
        assert d["imax"][0] == int(iv[isel].max()) and close(float(d["imean"][0]), float(iv[isel].mean())), where
    else:
        assert d["imax"][0] is None and d["imean"][0] is None, where


@pytest.mark.parametrize("seed", TREE_SEEDS)
def test_random_expression_trees_on_the_device(pl, seed):
    """filter(pred).select(n, fs, fc, fmin, isum, imax, imean) of the CPU test's trees on real columns: the generic interpreter and the per-node kernels for every
    seed, the run-time compiler for the first six that fuse.  A seed listed as fusing that does not report a fused scan fails."""
    cols, pred, ftree, itree = expr_trees.tree_case(seed)
    df = pl.DataFrame([pl.Series(k, v, validity=m) for k, (v, m) in cols.items()])
    q = expr_trees.tree_query(df.lazy(), pred, ftree, itree)
    if seed in FUSING_SEEDS:
        for mode in ("generic", "jit") if seed in JIT_SEEDS else ("generic",):
            check_tree(R.collect(pl, q, mode).to_dict(), pred, ftree, itree, (seed, mode))
    else:
        check_tree(q.collect().to_dict(), pred, ftree, itree, (seed, "default"))
    check_tree(R.collect(pl, q, "per_node").to_dict(), pred, ftree, itree, (seed, "per_node"))


@pytest.mark.parametrize("seed", [6, 18])
def test_aggregate_of_a_bare_literal_is_a_scalar_on_every_route(pl, seed):
    """Regression, found by the trees above: seed 6 (the float tree is lit(2.75)) and seed 18 (the integer tree is lit(-5), and the filter keeps no row).  The fused
    select used to repeat the literal on every kept row (count = rows kept, sum = rows kept * 2.75; sum = 0 for seed 18) where the per-node evaluator and the
    reference aggregate the one-row literal (count 1, sum 2.75; sum -5).  Such a select is not fused any more, and says why."""
    cols, pred, ftree, itree = expr_trees.tree_case(seed)
    assert (ftree[0].kind == "lit") == (seed == 6) and (itree[0].kind == "lit") == (seed == 18) and seed not in FUSING_SEEDS
    df = pl.DataFrame([pl.Series(k, v, validity=m) for k, (v, m) in cols.items()])
    d = expr_trees.tree_query(df.lazy(), pred, ftree, itree).collect().to_dict()
    plan = pl.last_plan()          # (the filter in front keeps its fused pass; the select behind it is the per-node one)
    assert "(not fused: aggregate of a literal is a scalar" in plan and "Select{per-node kernels}" in plan and "FusedFilterAgg{" not in plan, plan
    if seed == 6:
        assert (d["fs"][0], d["fc"][0], d["fmin"][0]) == (2.75, 1, 2.75) and d["n"][0] > 1
    else:
        assert (d["isum"][0], d["imax"][0], d["imean"][0]) == (-5, -5, -5.0) and d["n"][0] == 0
