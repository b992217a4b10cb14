"""tests/expr_rows.py without a GPU: every query of tests/test_gpu_program_ops.py compiles to a fused program that holds the opcodes it is there for, the
edge tables have the layout the device test relies on, the numpy restatement of the device code (tests/program_eval.py) agrees with the row-by-row reference
on every compiled program over the edge tables, and the ten-input programs put their columns where the two load paths of the generic interpreter need them."""
import numpy as np
import pytest

import polars_amd as pl
from tests import expr_rows as R
from tests import expr_trees
from tests import program_eval
from tests import program_eval_select as pes
from tests.test_program_eval_cpu import frame_like

OPCODE = {name: getattr(program_eval, name) for name in dir(program_eval) if name.startswith("OP_")}
OPCODE["OP_SELECT"] = pes.OP_SELECT
PREFETCHED = 8           # fused_device.hpp kPrefetch: inputs 0..7 go through prefetch_inputs / store_prefetched, the rest through load_input


@pytest.fixture
def pe(monkeypatch):
    """program_eval with OP_SELECT (the ten-input programs hold a when / then / otherwise)"""
    monkeypatch.setattr(program_eval, "run_rows", pes.run_rows)
    return program_eval


def placeholders(table):
    """every column but the row id nullable, as the device frames are at every length (expr_rows.DeviceTable)"""
    return frame_like(table.cols)


def program_of(case):
    return R.query(pl, placeholders(case.table), case.exprs).debug_program()


# ---- fusing ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_query_fuses_and_holds_its_opcodes(name):
    case = R.CASES[name]
    prog = program_of(case)          # raises UnsupportedError if the query would fall back: no case may
    codes = {op[0] for op in prog["ops"]}
    missing = [o for o in case.ops if OPCODE[o] not in codes]
    assert not missing, (name, missing, sorted(codes))
    assert prog["kind"] == "group_by" and prog["inputs"][0]["name"] == "row"
    assert all(i["nullable"] == (i["name"] != "row") for i in prog["inputs"]), prog["inputs"]
    assert len(prog["ops"]) <= 32 and len(prog["aggs"]) <= 16 and len(prog["inputs"]) <= 10


def test_division_and_conversion_opcodes_by_class():
    """the examples of the issue, spelled out: u64 division is OP_FDIV_U / OP_MOD_U, int / int is OP_I2F + OP_DIV_F, u64 -> f64 is OP_U2F"""
    codes = lambda name: {op[0] for op in program_of(R.CASES[name])["ops"]}
    assert {OPCODE["OP_FDIV_U"], OPCODE["OP_MOD_U"]} <= codes("u64_ints") and not {OPCODE["OP_FDIV_I"], OPCODE["OP_MOD_I"]} & codes("u64_ints")
    assert {OPCODE["OP_FDIV_I"], OPCODE["OP_MOD_I"]} <= codes("i64_ints") and {OPCODE["OP_FDIV_I"], OPCODE["OP_MOD_I"]} <= codes("i64_null_heads_ints")
    assert {OPCODE["OP_I2F"], OPCODE["OP_DIV_F"]} <= codes("i64_floats") and OPCODE["OP_U2F"] not in codes("i64_floats")
    assert {OPCODE["OP_U2F"], OPCODE["OP_DIV_F"]} <= codes("u64_floats") and OPCODE["OP_I2F"] not in codes("u64_floats")
    assert OPCODE["OP_CMP_U"] in codes("cmp_u64_lit") and OPCODE["OP_CMP_I"] not in codes("cmp_u64_lit")
    assert OPCODE["OP_CANON_F"] not in codes("cmp_f64")      # (a float KEY is canonicalised; a compare orders the raw values)


def test_filter_predicates_compile_into_a_fused_program():
    """The filter-to-frame pipeline has no compile-only entry point (its root is the Filter); the same predicate in front of a count goes through the same
    predicate lowering, and must fuse -- for e and for ~e."""
    assert set(R.FILTER_JIT) <= set(R.FILTER_PREDICATES)
    for name, label in R.FILTER_PREDICATES:
        case = R.CASES[name]
        x = dict(case.exprs)[label]
        for e in (x.build(pl), ~x.build(pl)):
            prog = placeholders(case.table).lazy().filter(e).select(pl.len().alias("n")).debug_program()
            assert prog["pred"] != program_eval.NONE and any(OPCODE[o] in {op[0] for op in prog["ops"]} for o in case.ops), (name, label)


def test_only_the_named_expressions_fall_back():
    """Arithmetic on dtypes narrower than 64 bits and float // and % go to the per-node kernels on purpose (UnsupportedError, with the reason); nothing else here does:
    the share of unlisted fallbacks is zero."""
    loads, floats = placeholders(R.load_table()), placeholders(R.f64_table())
    for label, k, _ in R.NON_FUSABLE:
        with pytest.raises(pl.UnsupportedError, match="wraps at the column width" if k else "float floor-div / mod"):
            R.non_fusable_query(pl, floats if k is None else loads, label).debug_program()
    fallen = []
    for name, case in R.CASES.items():
        try:
            program_of(case)
        except pl.UnsupportedError as e:
            fallen.append((name, str(e)))
    assert fallen == []


# ---- layout ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_i64_table_layout_against_the_scan_tile():
    t = R.i64_table(False)
    (a, va), (b, vb) = t.cols["a"], t.cols["b"]
    T = R.TILE
    assert (((a[:T] | b[:T]) >> 31) == 0).all() and (b[:T] == 0).any() and va[:2 * T].all() and vb[:2 * T].all()       # tile 0: every lane takes the 32-bit divide
    assert set(a[:T].tolist()) == set(R.NARROW) == set(b[:T].tolist())
    differs = np.nonzero((a[:T] != a[T:2 * T]) | (b[:T] != b[T:2 * T]))[0]
    assert differs.tolist() == [R.WIDE_A_ROW, R.WIDE_B_ROW]                                                                # tile 1: tile 0 with two wide lanes
    assert a[T + R.WIDE_A_ROW] == -1 and b[T + R.WIDE_B_ROW] == 2 ** 31 and R.WIDE_A_ROW // 2 != R.WIDE_B_ROW // 2          # (a lane holds two rows)
    cross = list(zip(a[R.CROSS0:].tolist(), b[R.CROSS0:].tolist()))
    assert cross == [(x, y) for x in R.E_I64 for y in R.E_I64] and len(R.E_I64) == 19
    for pair in ((R.I64_MIN, -1), (R.I64_MIN, 0), (2 ** 31 - 1, 2 ** 31), (2 ** 31 + 1, 2 ** 31 - 1), (R.I64_MIN, R.I64_MAX), (-7, 2), (7, -2)):
        i = R.CROSS0 + cross.index(pair)
        assert va[i] and vb[i], pair                                                                                       # the named pairs are not under a null
    k = np.arange(len(cross))
    assert np.array_equal(va[R.CROSS0:], k % 5 != 4) and np.array_equal(vb[R.CROSS0:], k % 7 != 6)
    # the second variant: the same valid lanes; its nulls sit on wide values, so no tile of it has only narrow lanes
    h = R.i64_table(True)
    (ha, hva), (hb, hvb) = h.cols["a"], h.cols["b"]
    assert np.array_equal(ha[hva], a[hva]) and np.array_equal(hb[hvb], b[hvb]) and not hva[0] and not hvb[0] and (ha[0], hb[0]) == (R.I64_MIN, -1)
    for tile in (0, 1):
        s = slice(tile * T, (tile + 1) * T)
        wide = ((ha[s] | hb[s]) >> 31) != 0
        assert wide.any() and not (wide & hva[s] & hvb[s]).any() and (((np.where(hva[s], ha[s], 0) | np.where(hvb[s], hb[s], 0)) >> 31) == 0).all()
        assert 0 < (~hva[s]).sum() <= 3 and 0 < (~hvb[s]).sum() <= 3


@pytest.mark.parametrize("table", [R.i64_table(False), R.i64_table(True), R.u64_table(), R.f64_table(), R.bool_table(), R.load_table()], ids=lambda t: t.name)
def test_tables_end_in_a_partial_tile_and_an_odd_row(table):
    assert table.n % R.TILE != 0 and table.n > R.TILE + 1 and table.n < 700
    assert table.n % 2 == 1                  # full length: the last lane's second row is clamped; full - 1: it is not
    assert table.sizes() == sorted({1, 127, 128, 129, table.n - 1, table.n})
    for name, (v, m) in table.cols.items():
        assert len(v) == table.n and (name == "row") == (m is None)
    assert np.array_equal(table.cols["row"][0], np.arange(table.n)) and table.cols["row"][0].dtype == np.int64


def test_cross_product_tables():
    for t, edges, bits in ((R.u64_table(), R.E_U64, False), (R.f64_table(), R.E_F64_BITS, True)):
        a, b = t.cols["a"][0], t.cols["b"][0]
        if bits:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert list(zip(a.tolist(), b.tolist())) == [(x, y) for x in edges for y in edges]
        k = np.arange(t.n)
        assert np.array_equal(t.cols["a"][1], k % 5 != 4) and np.array_equal(t.cols["b"][1], k % 7 != 6)
    assert len(R.E_U64) == 13 and len(R.E_F64_BITS) == 15
    f = np.array(R.E_F64_BITS, np.uint64).view(np.float64)
    assert np.isnan(f[-2:]).all() and np.signbit(f[-1]) and not np.signbit(f[-2]) and np.signbit(f[4]) and f[4] == 0.0 and f[3] == -5e-324


def test_bool_table_places_every_combination():
    t = R.bool_table()
    idx = R.bool_combo_index()
    (p, pm), (q, qm) = t.cols["p"], t.cols["q"]
    seen = [(None if not pm[i] else bool(p[i]), None if not qm[i] else bool(q[i])) for i in range(t.n)]
    assert seen == [R.COMBOS[i] for i in idx] and len(set(R.COMBOS)) == 9
    rows = np.arange(t.n)
    last_tile = rows >= (t.n // R.TILE) * R.TILE
    word_edge = np.isin(rows % 64, (62, 63, 0, 1)) & (rows >= 62)
    for c in range(9):
        at = idx == c
        assert (at & (rows % 2 == 0)).any() and (at & (rows % 2 == 1)).any() and (at & word_edge).any() and (at & last_tile).any(), R.COMBOS[c]
    assert t.n - (t.n // R.TILE) * R.TILE < R.TILE


def test_load_table_holds_every_extreme_of_every_dtype():
    t = R.load_table()
    masks = []
    for name, dt in R.LOAD_DTYPES.items():
        v, m = t.cols[name]
        assert v.dtype == dt and not m.all()
        masks.append(m)
        present = set(v[m].tolist())
        if dt is np.bool_:
            assert present == {True, False}
        elif dt is np.float64:
            assert {np.finfo(dt).max, -np.finfo(dt).max, -1.0, 0.0} <= present and np.signbit(v[m & (v == 0)]).any()
        else:
            info = np.iinfo(dt)
            assert {info.min, info.max, 0, -1 if info.min < 0 else info.max} <= present
            if info.min == 0:
                assert (info.max >> 1) + 1 in present                       # the top bit alone: what a wrong sign extension turns negative
        for n in t.sizes()[1:]:                                             # every truncation from 127 rows on still shows each value valid
            assert set(v[:n][m[:n]].tolist()) == present, (name, n)
    assert len({tuple(m.tolist()) for m in masks}) == len(masks)            # the nulls do not line up
    i8, u32 = t.cols["i8"][0], t.cols["u32"][0]
    assert len({(int(x), int(y)) for x, y in zip(i8, u32)}) == 16           # nor do the values


# ---- the device restatement against the reference ---------------------------------------------------------------------------------------------------------------
def interpreted(pe, case, cols):
    """the compiled program through tests/program_eval.py, put back in row order: {label: (values, valid)} as expr_rows.observe gives them"""
    prog = R.query(pl, frame_like(cols), case.exprs).debug_program()
    got = pe.evaluate(prog, cols)
    rows = got["row"][0]
    order = np.argsort(rows, kind="stable")
    assert np.array_equal(rows[order], np.arange(len(rows))) and len(rows) == len(cols["row"][0])
    col = lambda name: (got[name][0][order], np.ones(len(rows), bool) if got[name][1] is None else got[name][1][order])
    res = {}
    for label, x in case.exprs:
        if x.ty == "b":
            (s, _), (c, _) = col(label + ".sum"), col(label + ".count")
            res[label] = (s == 1, c == 1)
        else:
            res[label] = col(label)
    return res


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_numpy_restatement_of_the_device_code_agrees_with_the_reference(pe, name):
    case = R.CASES[name]
    for n in (case.table.n, R.TILE + 1):
        cols = case.table.head(n)
        R.compare(interpreted(pe, case, cols), R.reference(case.exprs, cols), (name, n))


def test_reference_spot_values():
    """the reference itself at the rows the tables are built around, against answers worked out by hand"""
    a, b = R.col("a", "i"), R.col("b", "i")
    row = lambda x, y: {"a": x, "b": y}
    MIN, MAX = R.I64_MIN, R.I64_MAX
    assert R.arith("//", a, b).ev(row(MIN, -1)) == MIN and R.arith("%", a, b).ev(row(MIN, -1)) == 0          # wrapping_div(MIN, -1) = MIN
    assert R.arith("//", a, b).ev(row(7, 0)) is None and R.arith("%", a, b).ev(row(7, 0)) is None
    assert R.arith("//", a, b).ev(row(-7, 2)) == -4 and R.arith("%", a, b).ev(row(-7, 2)) == 1 and R.arith("%", a, b).ev(row(7, -2)) == -1
    assert R.arith("//", a, b).ev(row(2 ** 31 + 1, 2 ** 31 - 1)) == 1 and R.arith("%", a, b).ev(row(2 ** 31 + 1, 2 ** 31 - 1)) == 2
    assert R.arith("*", a, b).ev(row(MAX, 2)) == -2 and R.arith("+", a, b).ev(row(MAX, 1)) == MIN and R.arith("-", a, b).ev(row(MIN, 1)) == MAX
    assert R.arith("%", a, R.lit(-3, "i")).ev(row(7, 0)) == -2 and R.arith("//", a, R.lit(7, "i")).ev(row(-1, 0)) == -1
    assert R.cast(a, "Float64").ev(row(2 ** 53 + 1, 0)) == 2.0 ** 53 and R.cast(a, "Float64").ev(row(MAX, 0)) == 2.0 ** 63
    ua, ub = R.col("a", "u"), R.col("b", "u")
    assert R.arith("-", ua, ub).ev(row(0, 1)) == 2 ** 64 - 1 and R.arith("//", ua, ub).ev(row(2 ** 64 - 1, 2 ** 63)) == 1 and R.cmp("<", ua, ub).ev(row(2 ** 63 - 1, 2 ** 63)) is True
    assert R.cast(ua, "Float64").ev(row(2 ** 64 - 1, 0)) == 2.0 ** 64
    fa, fb = R.col("a", "f"), R.col("b", "f")
    nan, frow = np.float64("nan"), lambda x, y: {"a": np.float64(x), "b": np.float64(y)}
    assert R.cmp("==", fa, fb).ev(frow(nan, nan)) is True and R.cmp(">", fa, fb).ev(frow(nan, np.inf)) is True and R.cmp("<", fa, fb).ev(frow(nan, 1.0)) is False
    assert R.cmp("==", fa, fb).ev(frow(-0.0, 0.0)) is True and R.cmp("<", fa, fb).ev(frow(-0.0, 0.0)) is False and R.cmp(">=", fa, fb).ev(frow(1.0, nan)) is False
    assert np.isinf(R.arith("*", fa, fb).ev(frow(1.5e300, 1.5e300))) and R.arith("*", fa, fb).ev(frow(5e-324, 0.1)) == 0.0
    assert np.signbit(R.arith("*", fa, fb).ev(frow(-5e-324, 0.1))) and R.arith("/", fa, R.lit(4.0, "f")).ev(frow(5e-324, 0)) == 0.0
    p, q = R.col("p", "b"), R.col("q", "b")
    prow = lambda x, y: {"p": x, "q": y}
    assert R.logic("&", p, q).ev(prow(False, None)) is False and R.logic("&", p, q).ev(prow(True, None)) is None
    assert R.logic("|", p, q).ev(prow(True, None)) is True and R.logic("|", p, q).ev(prow(False, None)) is None and R.logic("^", p, q).ev(prow(True, None)) is None
    assert R.fill_null(p, True).ev(prow(None, None)) is True and R.is_null(p).ev(prow(None, True)) is True and R.not_(p).ev(prow(None, True)) is None


# ---- input order of the ten-input programs ----------------------------------------------------------------------------------------------------------------------
def test_ten_input_programs_reach_both_load_paths_with_every_dtype():
    narrow = {program_eval.I8, program_eval.I16, program_eval.I32, program_eval.U8, program_eval.U16, program_eval.U32}
    below, beyond = set(), []
    for name, (order, mins) in R.LOAD_PROGRAMS.items():
        prog = program_of(R.CASES[name])
        ins = prog["inputs"]
        assert [i["name"] for i in ins] == ["row"] + order and len(ins) == 10, (name, ins)
        assert [op[0] for op in prog["ops"][:10]] == [program_eval.OP_LOAD] * 10 and [op[2] for op in prog["ops"][:10]] == list(range(10))
        below |= {i["dtype"] for i in ins[:PREFETCHED]}
        beyond.append(ins[PREFETCHED:])
        for late in ins[PREFETCHED:]:            # what goes through load_input is looked at on its own, not only inside the total, in a program of this order
            assert any("min_" + late["name"] in dict(R.CASES[other].exprs) for other, (o, _) in R.LOAD_PROGRAMS.items() if o == order), (name, late)
    assert below == {program_eval.BOOL, program_eval.I8, program_eval.I16, program_eval.I32, program_eval.I64, program_eval.U8, program_eval.U16, program_eval.U32,
                     program_eval.U64, program_eval.F64}
    assert all(len(late) == 2 and all(i["dtype"] in narrow and i["nullable"] for i in late) for late in beyond)
    assert {i["name"] for late in beyond for i in late} == {"u16", "i8", "i32", "u32"}
    # every column has a min of its own in a program where it sits below index 8
    for k in R.LOAD_DTYPES:
        assert any("min_" + k in dict(R.CASES[n].exprs) and (["row"] + o).index(k) < PREFETCHED for n, (o, _) in R.LOAD_PROGRAMS.items() if k in o), k


# ---- the random trees the device test runs ----------------------------------------------------------------------------------------------------------------------
def test_which_random_trees_fuse():
    """tests/test_gpu_program_ops.py holds the list of seeds whose query is one fused program; it is computed here"""
    from tests.test_gpu_program_ops import FUSING_SEEDS, TREE_SEEDS
    fuse = []
    for seed in TREE_SEEDS:
        cols, pred, ftree, itree = expr_trees.tree_case(seed)
        try:
            expr_trees.tree_query(frame_like(cols).lazy(), pred, ftree, itree).debug_program()
            fuse.append(seed)
        except pl.UnsupportedError:
            pass
    assert fuse == FUSING_SEEDS and len(fuse) >= 30 and set(range(40)) <= set(TREE_SEEDS)


def test_a_select_that_aggregates_a_bare_literal_is_not_fused():
    """select(lit(k).sum()) is the aggregate of a one-row literal (the per-node evaluator and the reference: sum k, count 1); a fused program would repeat k on every
    row.  Inside a larger tree a literal is broadcast against its column as before, and a group_by is unchanged."""
    cols, _, _, _ = expr_trees.tree_case(0)
    lf = frame_like(cols).lazy()
    for agg in (pl.lit(2.75).sum(), pl.lit(-5, dtype=pl.Int64).count(), (pl.lit(2) * pl.lit(3)).max()):
        with pytest.raises(pl.UnsupportedError, match="aggregate of a literal is a scalar"):
            lf.filter(pl.col("a") > 0).select(pl.len().alias("n"), agg.alias("v")).debug_program()
    lf.select((pl.col("x") * 2.0 + 1.0).sum().alias("v")).debug_program()
    lf.group_by("b").agg(pl.lit(1).sum().alias("ones")).debug_program()
