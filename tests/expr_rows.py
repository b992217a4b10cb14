"""Edge tables, a row-by-row reference and the observation harness of the fused-program opcode tests (tests/test_gpu_program_ops.py on the device,
tests/test_expr_rows_cpu.py without one).

The fused scan runs a register program per row (fused_device.hpp exec_op / load_input / prefetch_inputs / store_prefetched).  Here every opcode that
ordinary queries are made of meets the values at which such code goes wrong, and every row's result is looked at on its own:

  * TABLES: deterministic columns (no RNG) whose layout against the 128-row scan tile is part of the test -- which tiles qualify for the 32-bit divide,
    where a single wide lane sits, which rows of a validity word hold which Boolean combination;
  * an expression is an X: the mirror-API expression and, next to it, its value for one row in plain Python -- integers as Python ints reduced mod 2^64,
    floor rules from Python's // and %, int -> f64 as float(int), f64 arithmetic as numpy float64, the float total order written out, three-valued validity
    (None is null).  Nothing here reads tests/program_eval.py: that module restates the device code, this one the meaning of the expressions;
  * observe(): one group per row.  group_by("row") with the row id as the key turns the scan's aggregate cells into a per-row read-out: min() of a numeric
    expression is the row's value and is null exactly when the value is null, sum() / count() of a Boolean give its value and its validity;
  * CASES: the queries of the GPU file, a few expressions packed into each program (the run-time compiler builds a kernel per program shape).
"""
import functools
import operator
import os
import re

import numpy as np

TILE = 128                       # fused::kTileRows
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M64 = 1 << 64


# ================================================================================================================ tables
class Table:
    """cols: {name: (values, valid bool array or None)}; the first column is the row id."""

    def __init__(self, name, cols):
        self.name, self.cols = name, cols
        self.n = len(cols["row"][0])
        for v, m in cols.values():
            v.setflags(write=False)
            if m is not None:
                m.setflags(write=False)

    def head(self, n):
        return {k: (v[:n], None if m is None else m[:n]) for k, (v, m) in self.cols.items()}

    def sizes(self):
        """full length, one short of it, one row, and one tile give or take a row"""
        return sorted({1, TILE - 1, TILE, TILE + 1, self.n - 1, self.n})


NARROW = [0, 1, 2, 3, 7, 65536, 2 ** 31 - 2, 2 ** 31 - 1]                # every pair qualifies for the 32-bit divide; 0 is among the divisors
E_I64 = [I64_MIN, I64_MIN + 1, -2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1, -7, -2, -1, 0, 1, 2, 7, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32, 2 ** 53 + 1, I64_MAX - 1, I64_MAX]
E_U64 = [0, 1, 2, 7, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2, 2 ** 64 - 1]
NAN_BITS, NAN_PAYLOAD_BITS = 0x7ff8000000000000, 0xfff8000000000123
E_F64_BITS = [np.float64(x).view(np.uint64).item() for x in (-np.inf, -1.5e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 0.1, 1.0, 3.0, 2.0 ** 53 + 2, 1.5e300, np.inf)] + [NAN_BITS, NAN_PAYLOAD_BITS]
WIDE_A_ROW, WIDE_B_ROW = 61, 90                                             # the two rows of tile 1 that differ from tile 0: a = -1, b = 2^31
CROSS0 = 2 * TILE                                                           # first row of the i64 cross product


def _cross_validity(n_cross):
    """a is null on every 5th row of a cross product, b on every 7th, counted so that INT64_MIN // -1 (row 7 of E_I64 x E_I64) is under neither"""
    k = np.arange(n_cross)
    return k % 5 != 4, k % 7 != 6


def _row_ids(n):
    return np.arange(n, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def i64_table(null_heads=False):
    """Tile 0: narrow pairs only.  Tile 1: tile 0 again with one wide a and one wide b.  Then E x E.
    null_heads: tiles 0 and 1 carry nulls, and they sit on wide values -- tile 0 holds wide garbage under three nulls (row 0: INT64_MIN // -1), the two wide rows
    of tile 1 are the null ones -- so both tiles take the 64-bit divide although every VALID lane is narrow."""
    head = [(NARROW[i % 8], NARROW[(i // 8) % 8]) for i in range(TILE)]
    tile1 = list(head)
    tile1[WIDE_A_ROW] = (-1, head[WIDE_A_ROW][1])
    tile1[WIDE_B_ROW] = (head[WIDE_B_ROW][0], 2 ** 31)
    cross = [(x, y) for x in E_I64 for y in E_I64]
    pairs = head + tile1 + cross
    a, b = np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)
    va, vb = np.ones(len(pairs), bool), np.ones(len(pairs), bool)
    va[CROSS0:], vb[CROSS0:] = _cross_validity(len(cross))
    if null_heads:
        a[0], b[0] = I64_MIN, -1
        va[0] = vb[0] = False
        a[77], va[77] = -5, False
        b[100], vb[100] = 2 ** 40, False
        va[TILE + WIDE_A_ROW] = False
        vb[TILE + WIDE_B_ROW] = False
    return Table("i64_null_heads" if null_heads else "i64", {"row": (_row_ids(len(pairs)), None), "a": (a, va), "b": (b, vb)})


def _cross_table(name, values):
    cross = [(x, y) for x in values for y in values]
    a, b = np.array([p[0] for p in cross], np.uint64), np.array([p[1] for p in cross], np.uint64)
    va, vb = _cross_validity(len(cross))
    return name, a, b, va, vb


@functools.lru_cache(maxsize=None)
def u64_table():
    name, a, b, va, vb = _cross_table("u64", E_U64)
    return Table(name, {"row": (_row_ids(len(a)), None), "a": (a, va), "b": (b, vb)})


@functools.lru_cache(maxsize=None)
def f64_table():
    name, a, b, va, vb = _cross_table("f64", E_F64_BITS)
    return Table(name, {"row": (_row_ids(len(a)), None), "a": (a.view(np.float64), va), "b": (b.view(np.float64), vb)})


COMBOS = [(p, q) for p in (True, False, None) for q in (True, False, None)]
WORD_EDGE_ROWS = [62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193]   # rows 62..65 of three validity words
BOOL_ROWS = 2 * TILE + 3 * len(COMBOS)                                      # odd; the last tile holds every combination three times


def bool_combo_index(n=BOOL_ROWS):
    """Row -> index into COMBOS: the nine in turn (nine is odd, so each meets even and odd rows), and each of them once more on the rows around a word edge."""
    idx = np.arange(n) % len(COMBOS)
    for j, r in enumerate(WORD_EDGE_ROWS):
        idx[r] = j % len(COMBOS)
    return idx


@functools.lru_cache(maxsize=None)
def bool_table():
    idx = bool_combo_index()
    def column(k):
        return np.array([COMBOS[i][k] is True for i in idx]), np.array([COMBOS[i][k] is not None for i in idx])
    return Table("bool", {"row": (_row_ids(len(idx)), None), "p": column(0), "q": column(1)})


def _int_edges(dt):
    info = np.iinfo(dt)
    if info.min < 0:
        return [info.min, info.max, -1, 0]
    return [0, info.max, (info.max >> 1) + 1, info.max >> 1]                # minimum, maximum = all ones, the top bit alone, everything below it


LOAD_DTYPES = {"flag": np.bool_, "i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64,
               "f64": np.float64}
LOAD_ROWS = 2 * TILE + 45                                                   # odd, partial last tile


@functools.lru_cache(maxsize=None)
def load_table():
    """One nullable column per dtype; column j repeats each of its edge values j + 1 times, so the columns drift against each other, and is null on rows of its own."""
    n = LOAD_ROWS
    i = np.arange(n)
    cols = {"row": (_row_ids(n), None)}
    for j, (name, dt) in enumerate(LOAD_DTYPES.items()):
        if dt is np.bool_:
            vals = [False, True, True, False]
        elif dt is np.float64:
            vals = [-np.finfo(np.float64).max, np.finfo(np.float64).max, -1.0, 0.0, -0.0]
        else:
            vals = _int_edges(dt)
        v = np.array(vals, dtype=dt)[(i // (j + 1)) % len(vals)]
        cols[name] = (v, (i + 3 * j) % (11 + j) != 0)
    return Table("loads", cols)


# ================================================================================================================ expressions with a per-row meaning
class X:
    """ty: 'i' (Int64), 'u' (UInt64), 'f' (Float64), 'b' (Boolean).  build(pl) -> the mirror-API expression.  ev(row) -> the value for one row {column: python value
    or None}: a Python int (already wrapped), a numpy float64, a bool, or None for null."""

    def __init__(self, ty, build, ev, text, lit=None):
        self.ty, self.build, self.ev, self.text, self.lit = ty, build, ev, text, lit

    def __repr__(self):
        return self.text


def wrap(x, ty):
    x %= M64
    return x - M64 if ty == "i" and x >= 1 << 63 else x


def col(name, ty):
    return X(ty, lambda pl: pl.col(name), lambda r: r[name], name)


def lit(v, ty, dtype=None):
    """dtype None: a plain Python literal (takes the column's class), else pl.lit(v, dtype=pl.<dtype>)"""
    val = np.float64(v) if ty == "f" else v
    return X(ty, lambda pl: v if dtype is None else pl.lit(v, dtype=getattr(pl, dtype)), lambda r: val, repr(v), lit=val)


def _strict(fn):
    """nulls propagate"""
    def ev2(x, y):
        def ev(r):
            p, q = x.ev(r), y.ev(r)
            return None if p is None or q is None else fn(p, q)
        return ev
    return ev2


def _to_f(p):
    return np.float64(float(p))            # Python's int -> float is correctly rounded (round half to even), like v_cvt_f64 of a 64-bit integer


_PY = {"+": operator.add, "-": operator.sub, "*": operator.mul, "/": operator.truediv, "//": operator.floordiv, "%": operator.mod,
       "==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge, "&": operator.and_, "|": operator.or_, "^": operator.xor}


def _build2(sym, x, y):
    return lambda pl: _PY[sym](x.build(pl), y.build(pl))


def arith(sym, x, y):
    """+ - * wrap at 64 bits; // and % floor (Python's rules), divisor 0 -> null, x // -1 = -x wrapped; / is f64 division, and division by a literal is
    multiplication by its reciprocal (the reference folds col / lit into col * (1 / lit))."""
    ty = x.ty
    text = f"({x} {sym} {y})"
    if sym == "/":
        conv = _to_f if ty in "iu" else (lambda p: p)
        if y.lit is not None:
            recip = np.float64(1.0) / np.float64(float(y.lit))
            fn = lambda p, q: conv(p) * recip
        else:
            fn = lambda p, q: conv(p) / conv(q)
        def ev_f(p, q):
            with np.errstate(all="ignore"):
                return fn(p, q)
        return X("f", _build2(sym, x, y), _strict(ev_f)(x, y), text)
    if ty == "f":
        def ev_f(p, q):
            with np.errstate(all="ignore"):
                return _PY[sym](p, q)
        return X("f", _build2(sym, x, y), _strict(ev_f)(x, y), text)
    if sym in ("//", "%"):
        fn = lambda p, q: None if q == 0 else wrap(_PY[sym](p, q), ty)
    else:
        fn = lambda p, q: wrap(_PY[sym](p, q), ty)
    return X(ty, _build2(sym, x, y), _strict(fn)(x, y), text)


def total_order(sym, p, q):
    """The float order of the reference: NaN equals NaN and is the greatest value; -0.0 equals 0.0."""
    pn, qn = bool(np.isnan(p)), bool(np.isnan(q))
    eq = (pn and qn) or (not pn and not qn and bool(p == q))
    lt = not eq and not pn and (qn or bool(p < q))
    return {"==": eq, "!=": not eq, "<": lt, "<=": lt or eq, ">": not (lt or eq), ">=": not lt}[sym]


def cmp(sym, x, y):
    fn = (lambda p, q: total_order(sym, p, q)) if x.ty == "f" else (lambda p, q: bool(_PY[sym](p, q)))
    return X("b", _build2(sym, x, y), _strict(fn)(x, y), f"({x} {sym} {y})")


def logic(sym, x, y):
    """Kleene: false & null = false, true | null = true; xor propagates nulls."""
    def ev(r):
        p, q = x.ev(r), y.ev(r)
        if sym == "&":
            return False if p is False or q is False else None if p is None or q is None else True
        if sym == "|":
            return True if p is True or q is True else None if p is None or q is None else False
        return None if p is None or q is None else p != q
    return X("b", _build2(sym, x, y), ev, f"({x} {sym} {y})")


def not_(x):
    return X("b", lambda pl: ~x.build(pl), lambda r: None if x.ev(r) is None else not x.ev(r), f"~{x}")


def is_null(x):
    return X("b", lambda pl: x.build(pl).is_null(), lambda r: x.ev(r) is None, f"{x}.is_null()")


def is_not_null(x):
    return X("b", lambda pl: x.build(pl).is_not_null(), lambda r: x.ev(r) is not None, f"{x}.is_not_null()")


def fill_null(x, v):
    val = np.float64(v) if x.ty == "f" else v
    return X(x.ty, lambda pl: x.build(pl).fill_null(v), lambda r: val if x.ev(r) is None else x.ev(r), f"{x}.fill_null({v!r})")


def cast(x, dtype):
    """Int64 / UInt64 of a narrower column of the same signedness keeps the value; Float64 of an integer rounds to nearest even; Float64 of a float is itself."""
    ty = {"Int64": "i", "UInt64": "u", "Float64": "f"}[dtype]
    if ty == "f":
        ev = lambda r: None if x.ev(r) is None else (x.ev(r) if x.ty == "f" else _to_f(x.ev(r)))
    else:
        assert x.ty == ty
        ev = x.ev
    return X(ty, lambda pl: x.build(pl).cast(getattr(pl, dtype)), ev, f"{x}.cast({dtype})")


def flag01(x):
    """when(flag).then(1).otherwise(0): a null flag takes the otherwise branch"""
    return X("i", lambda pl: pl.when(x.build(pl)).then(1).otherwise(0), lambda r: 1 if x.ev(r) is True else 0, f"when({x}).then(1).otherwise(0)")


def _py(v):
    if isinstance(v, np.bool_):
        return bool(v)
    if isinstance(v, np.integer):
        return int(v)
    return v                               # numpy float64 stays (its NaN bits with it)


def rows_of(cols):
    """{name: (values, valid)} -> one {name: python value or None} per row"""
    n = len(cols["row"][0])
    return [{k: (None if m is not None and not m[i] else _py(v[i])) for k, (v, m) in cols.items()} for i in range(n)]


NP_OF = {"i": np.int64, "u": np.uint64, "f": np.float64, "b": np.bool_}


def reference(exprs, cols):
    """{label: (values, valid)} of [(label, X)] over the rows of cols; a null row's value is 0"""
    rows = rows_of(cols)
    out = {}
    for label, x in exprs:
        vals = [x.ev(r) for r in rows]
        valid = np.array([v is not None for v in vals], bool)
        out[label] = (np.array([0 if v is None else v for v in vals], dtype=NP_OF[x.ty]), valid)
    return out


# ================================================================================================================ the queries
class Case:
    """One fused program: exprs [(label, X)] over `table`, observed per row.  ops: the opcodes (names of fused.hpp) the program must contain."""

    def __init__(self, name, table, exprs, ops):
        self.name, self.table, self.exprs, self.ops = name, table, exprs, ops


def _int_cases(ty, table, name, mod_lit):
    a, b = col("a", ty), col("b", ty)
    sfx = "I" if ty == "i" else "U"
    ints = [("add", arith("+", a, b)), ("sub", arith("-", a, b)), ("mul", arith("*", a, b)), ("fdiv", arith("//", a, b)), ("mod", arith("%", a, b))]
    lits = [("fdiv7", arith("//", a, lit(7, ty))), (f"mod{mod_lit}", arith("%", a, lit(mod_lit, ty)))]      # a program of their own: a 64-bit division is ~100 instructions
                                                                                                           # per row and path, and the run-time compiler's time goes with them
    flts = [("truediv", arith("/", a, b)), ("quarter", arith("/", a, lit(4, ty))), ("as_f64", cast(a, "Float64"))]
    conv = "OP_I2F" if ty == "i" else "OP_U2F"
    return [Case(f"{name}_ints", table, ints, ["OP_ADD_I", "OP_SUB_I", "OP_MUL_I", "OP_FDIV_" + sfx, "OP_MOD_" + sfx]),
            Case(f"{name}_int_literals", table, lits, ["OP_CONST", "OP_FDIV_" + sfx, "OP_MOD_" + sfx]),
            Case(f"{name}_floats", table, flts, [conv, "OP_DIV_F", "OP_MUL_F"])]


def _six(x, y, prefix=""):
    return [(prefix + n, cmp(s, x, y)) for n, s in (("eq", "=="), ("ne", "!="), ("lt", "<"), ("le", "<="), ("gt", ">"), ("ge", ">="))]


def _cases():
    cs = {}
    def add(*cases):
        for c in cases:
            cs[c.name] = c
    add(*_int_cases("i", i64_table(False), "i64", -3), *_int_cases("i", i64_table(True), "i64_null_heads", -3), *_int_cases("u", u64_table(), "u64", 3))
    fa, fb = col("a", "f"), col("b", "f")
    add(Case("f64_binary", f64_table(), [("add", arith("+", fa, fb)), ("sub", arith("-", fa, fb)), ("mul", arith("*", fa, fb)), ("div", arith("/", fa, fb))],
             ["OP_ADD_F", "OP_SUB_F", "OP_MUL_F", "OP_DIV_F"]),
        Case("f64_literals", f64_table(), [("quarter", arith("/", fa, lit(4.0, "f"))), ("affine", arith("+", arith("*", fa, lit(2.0, "f")), lit(1.0, "f"))), ("filled", fill_null(fa, 2.5))],
             ["OP_MUL_F", "OP_ADD_F", "OP_IFNULL"]))
    # comparisons: the six operators are one program
    ia, ib, ua, ub = col("a", "i"), col("b", "i"), col("a", "u"), col("b", "u")
    add(Case("cmp_i64", i64_table(True), _six(ia, ib), ["OP_CMP_I"]),
        Case("cmp_i64_lit", i64_table(True), _six(ia, lit(2 ** 31, "i")), ["OP_CMP_I"]),
        Case("cmp_u64", u64_table(), _six(ua, ub), ["OP_CMP_U"]),
        Case("cmp_u64_lit", u64_table(), _six(ua, lit(2 ** 63, "u", "UInt64")), ["OP_CMP_U"]),
        Case("cmp_f64", f64_table(), _six(fa, fb), ["OP_CMP_F"]),
        Case("cmp_f64_nan", f64_table(), _six(fa, lit(float("nan"), "f")), ["OP_CMP_F"]),
        Case("cmp_f64_negzero", f64_table(), _six(fa, lit(-0.0, "f")), ["OP_CMP_F"]))
    p, q = col("p", "b"), col("q", "b")
    add(Case("kleene_binary", bool_table(), [("and", logic("&", p, q)), ("or", logic("|", p, q)), ("xor", logic("^", p, q)), ("not", not_(p))], ["OP_AND", "OP_OR", "OP_XOR", "OP_NOT"]),
        Case("kleene_nulls", bool_table(), [("is_null", is_null(p)), ("is_not_null", is_not_null(p)), ("filled", fill_null(p, True)),
                                             ("mix", logic("|", logic("&", p, not_(q)), logic("^", q, fill_null(p, False))))], ["OP_IFNULL", "OP_AND", "OP_OR", "OP_XOR", "OP_NOT"]))
    add(*_load_cases(), *_narrow_cmp_cases())
    return cs


# ---- the ten-input programs -----------------------------------------------------------------------------------------------------------------------------------
# The row id is input 0; the compiler numbers the other inputs in the order the first aggregate names them.  The generic interpreter loads inputs 0..7 through
# prefetch_inputs / store_prefetched and inputs 8 and 9 through load_input: across the two orders every dtype sits below index 8, and 8 and 9 are narrow nullable
# columns in both.  A program has 16 aggregate cells -- the total takes 3, a min 2 (3 for f64) -- so the second order is observed by two programs.
LOAD_ORDER_A = ["flag", "i64", "u64", "f64", "i32", "u32", "i16", "u16", "i8"]           # leaves u8 out; inputs 8, 9 = u16, i8
LOAD_ORDER_B = ["u8", "i8", "u16", "f64", "u64", "i64", "flag", "i32", "u32"]            # leaves i16 out; inputs 8, 9 = i32, u32
LOAD_PROGRAMS = {"loads_a": (LOAD_ORDER_A, ["u16", "i8", "i16", "i32", "u32", "flag"]),
                 "loads_b1": (LOAD_ORDER_B, ["i32", "u32", "u8", "f64", "i8"]),
                 "loads_b2": (LOAD_ORDER_B, ["i64", "u64", "u16", "flag"])}
LOAD_TY = {"flag": "b", "i8": "i", "i16": "i", "i32": "i", "i64": "i", "u8": "u", "u16": "u", "u32": "u", "u64": "u", "f64": "f"}


def _load_column(name):
    c = col(name, LOAD_TY[name])
    return flag01(c) if name == "flag" else c


def _load_cases():
    out = []
    for name, (order, mins) in LOAD_PROGRAMS.items():
        terms = [cast(_load_column(k), "Float64") for k in order]
        total = terms[0]
        for t in terms[1:]:
            total = arith("+", total, t)
        exprs = [("total", total)]
        for k in mins:       # widened by a cast where the result dtype would otherwise be the narrow one: the cast is lossless and costs no op
            c = _load_column(k)
            exprs.append(("min_" + k, c if k in ("i64", "u64", "f64") else cast(c, "UInt64" if LOAD_TY[k] == "u" else "Int64")))
        out.append(Case(name, load_table(), exprs, ["OP_SELECT", "OP_I2F", "OP_U2F", "OP_ADD_F"]))
    return out


NARROW_LITS = {"i8": ("Int8", -128), "i16": ("Int16", -32768), "i32": ("Int32", -2 ** 31), "u8": ("UInt8", 255), "u16": ("UInt16", 65535), "u32": ("UInt32", 2 ** 32 - 1)}


def _narrow_cmp_cases():
    """a narrow column against a literal of its own dtype: fused, the load widens and the compare is a 64-bit one"""
    return [Case(f"cmp_{k}_lit", load_table(), _six(col(k, LOAD_TY[k]), lit(v, LOAD_TY[k], dt)), ["OP_CMP_I"]) for k, (dt, v) in NARROW_LITS.items()]


CASES = _cases()

# Predicates observed a second time through the filter-to-frame pipeline (filter(e).collect() and filter(~e).collect()): (case, label).  Every one of them runs in
# the generic interpreter and per node; FILTER_JIT names the ones that also get a run-time compiled kernel (a predicate and its negation are a kernel each).
FILTER_PREDICATES = [(c, l) for c in ("cmp_i64", "cmp_i64_lit", "cmp_u64", "cmp_u64_lit", "cmp_f64", "cmp_f64_nan", "cmp_f64_negzero") for l in ("eq", "ne", "lt", "le", "gt", "ge")]
FILTER_JIT = [("cmp_i64", "le"), ("cmp_u64_lit", "gt"), ("cmp_f64", "lt"), ("cmp_f64_nan", "eq")]

# ---- what does not fuse, by name ------------------------------------------------------------------------------------------------------------------------------
# The compiler sends arithmetic on dtypes narrower than 64 bits (it wraps at the column's width) and float // and % to the per-node kernels on purpose.
# (label, table, column dtype or None for the f64 table, operator)
NON_FUSABLE = [(f"{k}_{n}", k, s) for k in ("i8", "i16", "i32", "u8", "u16", "u32") for n, s in (("add", "+"), ("sub", "-"), ("mul", "*"))] + [("f64_fdiv", None, "//"), ("f64_mod", None, "%")]
NARROW_PARTNER = {"i8": 127, "i16": 32767, "i32": 2 ** 31 - 1, "u8": 255, "u16": 65535, "u32": 2 ** 32 - 1}      # the literal operand: the dtype's maximum


def non_fusable_query(pl, frame, label):
    """(query, column name, result numpy dtype or None) of a NON_FUSABLE entry over `frame` (the load table, or the f64 table)"""
    _, k, s = next(e for e in NON_FUSABLE if e[0] == label)
    if k is None:
        e = _PY[s](pl.col("a"), pl.col("b"))
    else:
        e = _PY[s](pl.col(k), pl.lit(NARROW_PARTNER[k], dtype=getattr(pl, NARROW_LITS[k][0])))
    return frame.lazy().group_by("row").agg(e.min().alias("v"))


# ================================================================================================================ placeholders, frames, observation
def aggregates(pl, exprs):
    """numeric: min (the row's value; null exactly when it is null).  Boolean: sum (1 = true) and count (1 = valid)."""
    out = []
    for label, x in exprs:
        e = x.build(pl)
        out += [e.sum().alias(label + ".sum"), e.count().alias(label + ".count")] if x.ty == "b" else [e.min().alias(label)]
    return out


def query(pl, frame, exprs):
    return frame.lazy().group_by("row").agg(*aggregates(pl, exprs))


class DeviceTable:
    """A table uploaded once; frame(n) is its first n rows as views of the same buffers (values and bitmaps), so a column is nullable at every length -- the
    program, and with it the compiled kernel, is the same for every n."""

    def __init__(self, pl, table):
        self.pl, self.table = pl, table
        self.full = {k: pl.Series(k, v, validity=m) for k, (v, m) in table.cols.items()}

    def frame(self, n):
        pl = self.pl
        cols = []
        for k, s in self.full.items():
            vp, mp = s.device_ptrs()
            cols.append(pl.Series.from_device(k, s.dtype, vp, n, mp, keepalive=s))
        return pl.DataFrame(cols)


MODES = ("generic", "jit", "per_node")


def configured_min_rows():
    """the run-time compiler's threshold as the library starts with it (csrc/jit.cpp enabled(); it has a setter and no getter), as tests/test_gpu_scan_tiles.py reads it"""
    if os.environ.get("PLX_JIT", "1").startswith("0"):
        return -1
    return int(os.environ.get("PLX_JIT_MIN_ROWS", 1 << 22))
PER_NODE_INPUTS = 8          # a per-node group_by takes its materialised aggregate sources as columns of a scan of at most 10 inputs: the key and 8 of them at a time


def per_node_plan(plan):
    """No expression ran inside a fused program: no fused filter or whole-frame aggregate, and a group-by only over inputs the per-node kernels materialised
    (its scan then holds nothing but the loads of those columns: ops == inputs)."""
    if "FusedFilter{" in plan or "FusedFilterAgg{" in plan or "fused_join" in plan:
        return False
    if "FusedFilterGroupBy{" not in plan:
        return True
    ins, ops = (int(x) for x in re.search(r"inputs=(\d+), ops=(\d+)", plan).groups())
    return "GroupBy{materialised inputs" in plan and ins == ops


def collect(pl, lf, mode, want="Fused"):
    """lf.collect() on one of the three routes; the fused ones must say so in the plan (a query that fell back to the per-node kernels fails here)."""
    F = pl._ffi
    if mode == "per_node":
        out = lf.collect(no_fusion=True)
        assert per_node_plan(pl.last_plan()), pl.last_plan()
        return out
    try:
        F.jit_set_min_rows(-1 if mode == "generic" else 0)
        out = lf.collect()
    finally:
        F.jit_set_min_rows(configured_min_rows())
    plan = pl.last_plan()
    assert want in plan and f"fused_scan[{mode}]" in plan and "materialised inputs" not in plan and "not fused" not in plan, (mode, plan)
    return out


def observe(pl, frame, exprs, mode):
    """{label: (values, valid)} per row, in row order, of [(label, X)]"""
    cost = lambda es: sum(2 if x.ty == "b" else 1 for _, x in es)
    if mode == "per_node" and cost(exprs) > PER_NODE_INPUTS:
        res, part = {}, []
        for e in exprs:
            if cost(part + [e]) > PER_NODE_INPUTS:
                res.update(observe(pl, frame, part, mode))
                part = []
            part.append(e)
        res.update(observe(pl, frame, part, mode))
        return res
    out = collect(pl, query(pl, frame, exprs), mode)
    got = dict(zip(out.columns, out._download_all()))
    rows, rows_valid = got["row"]
    order = np.argsort(rows, kind="stable")
    assert rows_valid is None and np.array_equal(rows[order], np.arange(frame.height)), (mode, len(rows), frame.height)      # one group per row, none lost
    def column(name):
        v, m = got[name]
        return v[order], (np.ones(len(v), bool) if m is None else m[order])
    res = {}
    for label, x in exprs:
        if x.ty == "b":
            (s, sm), (c, cm) = column(label + ".sum"), column(label + ".count")
            assert sm.all() and cm.all() and (c <= 1).all() and (s <= c).all(), (mode, label)
            res[label] = (s == 1, c == 1)
        else:
            res[label] = column(label)
    return res


def observe_filter(pl, frame, x, mode):
    """(rows where x is valid and true, rows where it is valid and false) through filter(x) / filter(~x) -> frame"""
    kept = []
    for e in (x.build(pl), ~x.build(pl)):
        out = collect(pl, frame.lazy().filter(e), mode, want="FusedFilter{")
        v, m = out["row"]._download()
        assert m is None
        kept.append(np.asarray(v, np.int64))
    return kept


def compare(got, want, where):
    """validity exact; integers and Booleans exact; f64 as bit patterns (the sign of zero counts), a NaN for a NaN whatever its payload"""
    for label, (wv, wm) in want.items():
        gv, gm = got[label]
        assert len(gv) == len(wv), (where, label, len(gv), len(wv))
        bad = np.nonzero(gm != wm)[0]
        assert len(bad) == 0, (where, label, "validity", bad[:8].tolist(), gm[bad[:8]].tolist())
        if wv.dtype == np.float64:
            gv = np.ascontiguousarray(gv, dtype=np.float64)
            assert got[label][0].dtype == np.float64, (where, label, got[label][0].dtype)
            nan = np.isnan(wv)
            same = np.where(nan, np.isnan(gv), gv.view(np.uint64) == np.ascontiguousarray(wv).view(np.uint64))
        else:
            assert gv.dtype.kind == wv.dtype.kind and gv.dtype.itemsize == wv.dtype.itemsize, (where, label, gv.dtype, wv.dtype)
            same = gv == wv
        bad = np.nonzero(wm & ~same)[0]
        assert len(bad) == 0, (where, label, "rows", bad[:8].tolist(), "got", gv[bad[:8]].tolist(), "want", wv[bad[:8]].tolist())
