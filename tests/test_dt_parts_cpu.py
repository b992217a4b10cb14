"""The dt namespace without a GPU: the reference of every check validates itself (tests/dt_parts_ref.py against numpy's datetime64 casts and pyarrow.compute); the
arithmetic of csrc/temporal.hpp through its host entry (plx_temporal_part_host), bit for bit over the corpus, and as a stand-alone program under
-fsanitize=undefined,address against a calendar walked day by day; the mirror API and its lowering (dtype and name table, TypeErrors, kind 13 with the part in `op`
and the unit in `lit`, an unchanged plx_aexpr); the fused programs the C++ compiler emits for queries that contain the op, interpreted row by row
(tests/program_eval_datepart.py adds OP_DATEPART to tests/program_eval.py); the late-materialisation split; the packed key plan of date parts; the run-time compiled
kernel's source; the per-node kernels' registers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import dt_parts_ref as R
from tests import program_eval
from tests import program_eval_datepart as ped
from tests.test_program_eval_cpu import by_key, close, frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars_amd", "csrc")
c = pl.col
DT = {"date": pl.Date, "ms": pl.Datetime("ms"), "us": pl.Datetime, "ns": pl.Datetime("ns")}
OUT_DT = {"year": pl.Int32, "ordinal_day": pl.Int16, "date": pl.Date}      # every other part: Int8


@pytest.fixture
def pe(monkeypatch):
    """program_eval whose run_rows knows OP_DATEPART (and OP_SELECT / OP_DICT below it)."""
    monkeypatch.setattr(program_eval, "run_rows", ped.run_rows)
    return program_eval


# ---- the reference, the host entry, the stand-alone program ---------------------------------------------------------------------------
def test_reference_agrees_with_numpy_and_pyarrow():
    R.self_check()
    # the corpus holds what the issue lists
    d = set(R.corpus("date")[0].tolist())
    assert {0, 1, -1, 58, 59, 60, -719468, -719467, -719469, 146096, 146097, 146098, -146096, -146097, -146098, -719162, 2932896, -(1 << 31), (1 << 31) - 1} <= d
    for y in (1900, 2000, 2100):
        assert {R.days_from_civil(y, 3, 1), R.days_from_civil(y, 3, 1) - 1} <= d
    for unit in ("ms", "us", "ns"):
        t, tpd = set(R.corpus(unit)[0].tolist()), R.TICKS_PER_DAY[unit]
        assert {R.I64_MIN + 1, R.I64_MAX, -1, 0, tpd - 1, 59 * tpd - 1, 59 * tpd, 60 * tpd - 1} <= t
    v, valid = R.corpus("us", nullable=True)
    assert 0.25 < 1 - valid.mean() < 0.45 and not valid[0]


def host_part(values, unit, part):
    v = np.ascontiguousarray(values)
    out = np.full(len(v), -99, dtype=R.out_dtype(part))
    F.check(F.lib().plx_temporal_part_host(v.ctypes.data, R.UNITS.index(unit), R.PARTS.index(part), len(v), out.ctypes.data))
    return out


@pytest.mark.parametrize("unit", R.UNITS)
def test_host_entry_matches_the_reference_bit_for_bit(unit):
    v = R.corpus(unit)[0]
    assert v.dtype == (np.int32 if unit == "date" else np.int64)
    for part in R.PARTS:
        if not R.parts_of(unit, part):
            out = np.zeros(len(v), np.int32)
            assert F.lib().plx_temporal_part_host(v.ctypes.data, R.UNITS.index(unit), R.PARTS.index(part), len(v), out.ctypes.data) != 0
            assert "Datetime only" in F.lib().plx_last_error().decode()
            continue
        got, want = host_part(v, unit, part), R.part(v, unit, part)
        assert got.dtype == want.dtype and np.array_equal(got, want), (unit, part, v[got != want][:5], got[got != want][:5], want[got != want][:5])
    assert F.lib().plx_temporal_part_host(v.ctypes.data, 4, 0, len(v), v.ctypes.data) != 0 and F.lib().plx_temporal_part_host(v.ctypes.data, 0, 10, len(v), v.ctypes.data) != 0
    assert F.lib().plx_temporal_part_host(None, 0, 0, 0, None) == 0


def test_the_arithmetic_under_sanitizers_against_a_walked_calendar(tmp_path):
    """tests/emu/temporal_main.cpp: temporal::part (the body the kernels and plx_temporal_part_host share) as a stand-alone program built with
    -fsanitize=undefined,address -- a signed overflow aborts it -- over the corpus, 1e6 strided values per unit and every day of the years 1..4000, against plain
    counters stepped day by day."""
    exe, path = str(tmp_path / "temporal_main"), str(tmp_path / "corpus.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "temporal_main.cpp")], check=True)
    R.write_corpus_file(path)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    m = re.search(r"checked=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 50_000_000, r.stdout


# ---- the mirror API and its lowering ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    """A few thousand rows: half drawn from the corpus (boundary values, whole dtype range), half ordinary dates of 1992..2003; a third of d / t null."""
    rng = np.random.default_rng(30)
    n = 3001
    def draw(unit):
        corp = R.corpus(unit)[0]
        tpd = R.TICKS_PER_DAY[unit]
        usual = rng.integers(8035 * tpd, 12418 * tpd, n)
        return np.where(rng.random(n) < 0.5, corp[rng.integers(0, len(corp), n)], usual).astype(corp.dtype)
    cols = {"d": (draw("date"), rng.random(n) >= 1 / 3), "t": (draw("us"), rng.random(n) >= 1 / 3), "tn": (draw("ns"), None), "tm": (draw("ms"), None),
            "d2": (rng.integers(8035, 10592, n).astype(np.int32), None),      # 1992-01-01 .. 1998-12-31, no nulls
            "x": (rng.normal(size=n), None), "v": (rng.integers(-50, 50, n).astype(np.int64), rng.random(n) < 0.8), "flag": (rng.random(n) < 0.5, rng.random(n) < 0.75),
            "k": (rng.integers(0, 5, n).astype(np.int64), None)}
    dtypes = {"d": pl.Date, "t": pl.Datetime, "tn": pl.Datetime("ns"), "tm": pl.Datetime("ms"), "d2": pl.Date}
    return cols, frame_like(cols, dtypes), dtypes


def full(cols, name):
    v, m = cols[name]
    return v, np.ones(len(v), bool) if m is None else m


def lowered(df, expr):
    low, root, schema = df.lazy().select(expr)._lower()
    return low, low.aexprs[low.irs[root]["exprs"][0]], schema


def test_dtype_and_output_name_table(data):
    _, df, _ = data
    for col, unit in (("d", "date"), ("tm", "ms"), ("t", "us"), ("tn", "ns")):
        for i, part in enumerate(R.PARTS):
            expr = getattr(c(col).dt, part)()
            assert repr(expr) == f"col({col!r}).dt.{part}()"
            if not R.parts_of(unit, part):
                with pytest.raises(TypeError, match="needs a Datetime column, got Date"):
                    lowered(df, expr)
                continue
            low, top, schema = lowered(df, expr)
            assert list(schema.items()) == [(col, OUT_DT.get(part, pl.Int8))], (col, part, schema)      # named like the column, as the reference
            assert top["kind"] == F.AE_TEMPORAL == 13 and top["op"] == i and top["lit"] == R.UNITS.index(unit) and low.aexprs[top["lhs"]]["kind"] == F.AE_COLUMN
    low, top, schema = lowered(df, c("t").dt.date().dt.year().alias("y"))      # the date of a Datetime is a Date: its parts are a Date's
    inner = low.aexprs[low.aexprs[top["lhs"]]["lhs"]]
    assert schema == {"y": pl.Int32} and low.aexprs[top["lhs"]]["lit"] == F.UNIT_DATE and inner["lit"] == F.UNIT_US and inner["op"] == F.PART_DATE
    assert lowered(df, (c("d").dt.month() == 12))[2] == {"d": pl.Boolean}


def test_type_errors(data):
    _, df, _ = data
    for bad in (c("v").dt.year(), c("x").dt.month(), c("flag").dt.day(), pl.lit(3).dt.year(), c("d").dt.year().dt.month()):
        with pytest.raises(TypeError, match="needs a Date or Datetime column"):
            lowered(df, bad)
    for part in R.DATETIME_ONLY:
        with pytest.raises(TypeError, match="needs a Datetime column, got Date"):
            lowered(df, getattr(c("d").dt, part)())
    with pytest.raises(TypeError, match="needs a Date or Datetime column"):
        df.lazy().group_by(c("k").dt.weekday()).agg(pl.len())._lower()


def test_the_node_crosses_the_abi_with_the_unit_in_the_literal_slot(data, tmp_path):
    _, df, _ = data
    low, root, _ = df.lazy().select(c("tn").dt.hour(), c("d").dt.year().alias("y"), (c("k") + 1).alias("p"))._lower()
    ir, n_ir, ae, n_ae, keep = low.to_c()
    seen = 0
    for i, d in enumerate(low.aexprs):
        if d["kind"] == F.AE_TEMPORAL:
            seen += 1
            assert ae[i].kind == 13 and ae[i].op == d["op"] and ae[i].lit.u == d["lit"] and ae[i].lhs == d["lhs"] and ae[i].cond == -1
    assert seen == 2
    # the layout of plx_aexpr is what it was: `cond` is still the trailing field and the struct has not grown
    assert F.AExpr._fields_[-1][0] == "cond" and C.sizeof(F.AExpr) == 48 and F.AExpr.lit.offset == 24 and F.AExpr.name.offset == 32 and F.AExpr.cond.offset == 40
    src = tmp_path / "temporal.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AE_TEMPORAL == 13 && PLX_AE_BITMAP_LOOKUP == 12, "plx_aexpr_kind numbering");
_Static_assert(sizeof(plx_aexpr) == 48 && offsetof(plx_aexpr, cond) == offsetof(plx_aexpr, name) + sizeof(char*), "plx_aexpr did not grow; cond is its trailing field");
_Static_assert(PLX_UNIT_DATE == 0 && PLX_UNIT_NS == 3 && PLX_PART_YEAR == 0 && PLX_PART_DATE == 9, "unit / part numbering");
int (*p1)(plx_column, int, int, plx_column*) = plx_temporal_part;
int (*p2)(const void*, int, int, int64_t, void*) = plx_temporal_part_host;
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "temporal.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the importer checks the node before anything needs a device
    buf = C.create_string_buffer(1 << 12)
    for field, value, msg in (("lit", 4, "date part"), ("op", 10, "date part"), ("lit", F.UNIT_DATE, "Int32 expression")):
        low, root, _ = df.lazy().select(c("tn").dt.hour().cast(pl.Int64).sum())._lower()
        node = [d for d in low.aexprs if d["kind"] == F.AE_TEMPORAL][0]
        node[field] = value
        if msg == "Int32 expression":
            node["op"] = F.PART_YEAR
        ir, n_ir, ae, n_ae, keep = low.to_c()
        assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) != 0
        assert msg in F.lib().plx_last_error().decode(), F.lib().plx_last_error().decode()
    for name in ("_polars_plugin_plx_dt_part", "_polars_plugin_field_plx_dt_part"):
        assert hasattr(F.lib(), name)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "plx_dt_part" in f.read()


# ---- the fused programs, row by row ------------------------------------------------------------------------------------------------------
def n_dateparts(prog):
    return sum(op[0] == ped.OP_DATEPART for op in prog["ops"])


def test_filter_on_year_and_a_part_as_aggregate_source(data, pe):
    cols, df, _ = data
    q = (df.lazy().filter((c("d").dt.year() == 2000) | (c("t").dt.month() == 12))
         .select(c("d").dt.day().cast(pl.Int64).sum().alias("s"), c("t").dt.ordinal_day().max().alias("mx"), c("tn").dt.hour().sum().alias("h"),
                 c("tm").dt.weekday().min().alias("wd"), c("t").dt.second().count().alias("cnt"), pl.len().alias("n")))
    prog = q.debug_program()
    assert n_dateparts(prog) == 7
    for op in prog["ops"]:
        if op[0] == ped.OP_DATEPART:
            assert op[2] == op[3] and int(op[5]) == 0          # one source slot, no immediate
    got = pe.evaluate(prog, cols)
    (d, dm), (t, tm_), (tn, _), (tms, _) = (full(cols, nm) for nm in ("d", "t", "tn", "tm"))
    a, b = (R.part(d, "date", "year") == 2000, dm), (R.part(t, "us", "month") == 12, tm_)
    keep = (a[0] & a[1]) | (b[0] & b[1])                      # Kleene or: true wherever one side is valid and true
    assert 50 < keep.sum() < len(d) - 50
    assert got["s"][0][0] == int(R.part(d, "date", "day")[keep & dm].astype(np.int64).sum()) and got["mx"][0][0] == int(R.part(t, "us", "ordinal_day")[keep & tm_].max())
    assert got["h"][0][0] == int(R.part(tn, "ns", "hour")[keep].astype(np.int64).sum()) and got["wd"][0][0] == int(R.part(tms, "ms", "weekday")[keep].min())
    assert got["cnt"][0][0] == int((keep & tm_).sum()) and got["n"][0][0] == int(keep.sum())
    assert pe.split_matches(prog, cols)


def group_reference(keys, valids, keep, aggs):
    """{key tuple (None = null): {name: value}} over the rows of `keep`; aggs: {name: fn(row mask) -> value}"""
    want = {}
    tuples = [tuple(int(k[i]) if m[i] else None for k, m in zip(keys, valids)) for i in np.nonzero(keep)[0]]
    for key in set(tuples):
        rows = keep.copy()
        for k, m, kv in zip(keys, valids, key):
            rows &= ~m if kv is None else (m & (k == kv))
        want[key] = {name: fn(rows) for name, fn in aggs.items()}
    return want


@pytest.mark.parametrize("col,unit", [("d", "date"), ("t", "us")])
def test_group_by_month_and_by_year_month(data, pe, col, unit):
    cols, df, _ = data
    (v, vm), (x, _), (k, km) = full(cols, "v"), full(cols, "x"), full(cols, col)
    aggs = [c("x").sum().alias("s"), c("v").sum().alias("vs"), c("v").min().alias("mn"), pl.len().alias("n")]
    ref = {"s": lambda r: float(x[r].sum()), "vs": lambda r: int(v[r & vm].sum()), "mn": lambda r: int(v[r & vm].min()) if (r & vm).any() else None, "n": lambda r: int(r.sum())}
    keep = np.ones(len(k), bool)
    month, year = R.part(k, unit, "month"), R.part(k, unit, "year")
    # month alone
    prog = df.lazy().group_by(c(col).dt.month().alias("m")).agg(*aggs).debug_program()
    assert n_dateparts(prog) == 1 and prog["key_plan"]["packed"] == 1
    got, want = by_key(pe.evaluate(prog, cols), ["m"]), group_reference([month], [km], keep, ref)
    assert set(got) == set(want) and len(want) == 13                  # twelve months and the nulls
    for key, w in want.items():
        assert all(close(got[key][nm], w[nm]) for nm in w), (key, got[key], w)
    # (year, month) under a filter on the same column
    prog = df.lazy().filter(c(col).dt.weekday() <= 5).group_by(c(col).dt.year().alias("y"), c(col).dt.month().alias("m")).agg(*aggs).debug_program()
    assert n_dateparts(prog) == 3
    keep = km & (R.part(k, unit, "weekday") <= 5)
    got, want = by_key(pe.evaluate(prog, cols), ["y", "m"]), group_reference([year, month], [km, km], keep, ref)
    assert set(got) == set(want) and len(want) > 60
    for key, w in want.items():
        assert all(close(got[key][nm], w[nm]) for nm in w), (key, got[key], w)
    assert pe.split_matches(prog, cols)


def test_a_part_inside_when_then(data, pe):
    cols, df, _ = data
    n = len(cols["x"][0])
    q = df.lazy().group_by("k").agg(pl.when(c("d").dt.weekday() >= 6).then(c("x")).otherwise(0.0).sum().alias("weekend"),
                                    pl.when(c("flag")).then(c("t").dt.quarter().cast(pl.Int64)).otherwise(0).sum().alias("q"),
                                    pl.when(c("t").dt.minute() < 30).then(c("d").dt.day()).max().alias("mx"))
    prog = q.debug_program()
    assert n_dateparts(prog) == 4
    got = by_key(pe.evaluate(prog, cols), ["k"])
    (d, dm), (t, tm_), (x, _), (flag, fm), (k, _) = (full(cols, nm) for nm in ("d", "t", "x", "flag", "k"))
    wk = (R.part(d, "date", "weekday") >= 6) & dm             # a null predicate row takes the otherwise
    fl = flag & fm
    half = (R.part(t, "us", "minute") < 30) & tm_
    for kv in range(5):
        rows = k == kv
        g = got[(kv,)]
        assert close(g["weekend"], float(x[rows & wk].sum()))
        assert g["q"] == int(R.part(t, "us", "quarter")[rows & fl & tm_].astype(np.int64).sum())
        assert g["mx"] == int(R.part(d, "date", "day")[rows & half & dm].max())


def test_a_part_under_the_probe_side_predicate_of_a_join_pipeline(data, pe):
    rng = np.random.default_rng(33)
    nb, npr = 800, 6000
    bcols = {"k": (rng.permutation(2000)[:nb].astype(np.int64), None), "attr": (rng.integers(0, 6, nb).astype(np.int64), None)}
    corp = R.corpus("date")[0]
    pd_ = np.where(rng.random(npr) < 0.3, corp[rng.integers(0, len(corp), npr)], rng.integers(10957, 11688, npr)).astype(np.int32)      # many rows in 2000 and 2001
    pcols = {"k": (rng.integers(0, 2000, npr).astype(np.int64), None), "d": (pd_, rng.random(npr) < 0.8), "x": (rng.normal(size=npr), None)}
    P = frame_like(pcols, {"d": pl.Date}).lazy().filter(c("d").dt.year() == 2000)
    prog = P.join(frame_like(bcols).lazy(), on="k").group_by("k", "attr").agg(c("x").sum().alias("s"), c("d").dt.month().max().alias("mm"), pl.len().alias("n")).debug_program()
    assert prog["kind"] == "join_group_by" and n_dateparts(prog["probe"]) == 2
    pp = prog["probe"]
    year_pc = [i for i, op in enumerate(pp["ops"]) if op[0] == ped.OP_DATEPART and (op[4] & 15) == F.PART_YEAR]
    month_pc = [i for i, op in enumerate(pp["ops"]) if op[0] == ped.OP_DATEPART and (op[4] & 15) == F.PART_MONTH]
    assert len(year_pc) == 1 and (pp["early_mask"] >> year_pc[0]) & 1 and len(month_pc) == 1 and not (pp["early_mask"] >> month_pc[0]) & 1      # the predicate's part early, the aggregate's late
    assert pe.split_matches(pp, pcols)
    got = by_key(pe.evaluate_join(prog, bcols, pcols), ["k", "attr"])
    attr_of = dict(zip(bcols["k"][0].tolist(), bcols["attr"][0].tolist()))
    (d, dm), (x, _), (k, _) = (full(pcols, nm) for nm in ("d", "x", "k"))
    keep = dm & (R.part(d, "date", "year") == 2000) & np.isin(k, bcols["k"][0])
    month = R.part(d, "date", "month")
    assert keep.sum() > 200 and len(got) == len(set(k[keep].tolist()))
    for kv in set(k[keep].tolist()):
        rows, g = keep & (k == kv), got[(kv, attr_of[kv])]
        assert g["n"] == int(rows.sum()) and close(g["s"], float(x[rows].sum())) and g["mm"] == int(month[rows].max())


def test_split_keeps_the_op_early_only_where_the_predicate_or_the_key_needs_it(data, pe):
    cols, df, _ = data
    early = lambda prog, pc: (prog["early_mask"] >> pc) & 1
    pcs = lambda prog, part: [i for i, op in enumerate(prog["ops"]) if op[0] == ped.OP_DATEPART and (op[4] & 15) == part]
    # predicate: early; aggregate source: late
    prog = df.lazy().filter(c("d").dt.year() == 2000).select(c("t").dt.day().sum().alias("s"), pl.len().alias("n")).debug_program()
    (y,), (dd,) = pcs(prog, F.PART_YEAR), pcs(prog, F.PART_DAY)
    assert prog["any_late"] == 1 and early(prog, y) and not early(prog, dd) and pe.split_matches(prog, cols)
    # key: early; the same column's other part, an aggregate source: late
    prog = df.lazy().filter(c("k") < 4).group_by(c("d").dt.month().alias("m")).agg(c("d").dt.day().max().alias("mx")).debug_program()
    (m,), (dd,) = pcs(prog, F.PART_MONTH), pcs(prog, F.PART_DAY)
    assert early(prog, m) and not early(prog, dd) and pe.split_matches(prog, cols)
    # the one op feeds both: early, and emitted once
    prog = df.lazy().filter(c("d").dt.month() > 6).select(c("d").dt.month().max().alias("mx")).debug_program()
    (m,) = pcs(prog, F.PART_MONTH)
    assert early(prog, m) and pe.split_matches(prog, cols)


def bits(part):
    return bin(int(part["mask"])).count("1")


def test_key_plan_packs_date_parts(data):
    cols, df, dtypes = data
    # d2: 1992-01-01 .. 1998-12-31 without nulls -> 7 years: 3 bits, then the month: 4 bits
    kp = df.lazy().group_by(c("d2").dt.year().alias("y"), c("d2").dt.month().alias("m")).agg(pl.len()).debug_program()["key_plan"]
    y, m = kp["parts"]
    d2 = cols["d2"][0]
    assert kp["packed"] == 1 and kp["wide"] == 0 and (bits(y), y["shift"], int(y["min"])) == (3, 0, int(R.part(d2, "date", "year").min())) and (bits(m), m["shift"], int(m["min"])) == (4, 3, 1)
    assert y["dtype"] == F.I32 and m["dtype"] == F.I8 and int(y["null_code"]) == (1 << 64) - 1
    kp = df.lazy().group_by(c("d2").dt.month()).agg(pl.len()).debug_program()["key_plan"]
    assert kp["packed"] == 1 and [bits(p) for p in kp["parts"]] == [4]
    # static ranges need nothing from the column: a column nobody has statistics of, every part but year / date
    bare = frame_like(cols, dtypes, stats=False)
    for part, nbits in (("month", 4), ("day", 5), ("quarter", 2), ("weekday", 3), ("ordinal_day", 9), ("hour", 5), ("minute", 6), ("second", 6)):
        kp = bare.lazy().group_by(getattr(c("tn").dt, part)()).agg(pl.len()).debug_program()["key_plan"]
        assert kp["packed"] == 1 and [bits(p) for p in kp["parts"]] == [nbits], (part, kp)
    # a nullable operand: one more code for the null
    kp = df.lazy().group_by(c("t").dt.quarter().alias("q"), c("t").dt.weekday().alias("w")).agg(pl.len()).debug_program()["key_plan"]
    q, w = kp["parts"]
    assert kp["packed"] == 1 and (bits(q), int(q["null_code"])) == (3, 4) and (bits(w), int(w["null_code"]), w["shift"]) == (3, 7, 3)
    # date() of a Datetime is monotone like the year
    t = cols["t"][0][cols["t"][1]]
    kp = df.lazy().group_by(c("t").dt.date()).agg(pl.len()).debug_program()["key_plan"]
    lo, hi = int(R.part(np.array([t.min()]), "us", "date")[0]), int(R.part(np.array([t.max()]), "us", "date")[0])
    assert kp["packed"] == 1 and int(kp["parts"][0]["min"]) == lo and bits(kp["parts"][0]) == int(hi - lo + 2 - 1).bit_length() and kp["parts"][0]["dtype"] == F.I32
    # no range for the year of a column without statistics, or of an expression: a raw 64-bit key
    for lf in (bare.lazy().group_by(c("d2").dt.year()), df.lazy().group_by(c("t").dt.date().dt.year())):
        kp = lf.agg(pl.len()).debug_program()["key_plan"]
        assert kp["packed"] == 0 and int(kp["parts"][0]["mask"]) == (1 << 64) - 1


def test_the_run_time_compiled_kernel_builds(data):
    _, df, _ = data
    (df.lazy().filter(c("d").dt.year() == 2000).group_by(c("t").dt.year().alias("y"), c("t").dt.month().alias("m"))
     .agg(c("tn").dt.hour().sum().alias("h"), c("tm").dt.ordinal_day().max().alias("o"), c("x").sum().alias("s"))).jit_selftest()


def test_queries_lower(data):
    from polars_amd import datagen, queries
    li = datagen.lineitem_host(2000, seed=5)
    names = ("l_shipdate", "l_extendedprice", "l_discount", "l_quantity")
    df = frame_like({k: (li[k], None) for k in names}, datagen.logical_dtypes(pl))
    prog = queries.revenue_by_ship_month(df.lazy()).debug_program()
    assert [p["name"] for p in prog["key_plan"]["parts"]] == ["year", "month"] and prog["key_plan"]["packed"] == 1 and n_dateparts(prog) == 2
    prog = queries.q6_year(df.lazy(), 1994).debug_program()
    assert n_dateparts(prog) == 1 and prog["kind"] == "select"
    low, _, _ = queries.q6_year(df.lazy(), 1994)._lower()
    assert low.notes == ["col('l_shipdate').dt.year() [Datetime[us]]"]          # what pl.last_plan() / explain() print next to the engine's plan after a collect


# ---- the per-node kernels ------------------------------------------------------------------------------------------------------------------
def test_per_node_kernels_use_no_scratch_and_spill_nothing():
    """kernels_temporal.hip compiled with -Rpass-analysis=kernel-resource-usage (no GPU needed): one kernel per (unit, part), none with scratch or spilled registers."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-munsafe-fp-atomics",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernels_temporal.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900).stderr
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(": ", 1)[1]
            res[cur] = {}
        elif cur and ": " in t:
            k, v = t.split(": ", 1)
            res[cur][k.strip()] = v.strip()
    kernels = {name: r for name, r in res.items() if "temporal_part_kernel" in name}
    assert len(kernels) == 6 + 3 * 10, sorted(kernels)          # a Date has six parts, each Datetime unit ten
    for name, r in kernels.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r)                  # (nothing here needs many: full occupancy for a kernel that streams)
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "kernels_temporal" in re.search(r"^KERNELS = (.*)$", f.read(), re.M).group(1).split()
