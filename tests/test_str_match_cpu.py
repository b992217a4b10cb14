"""String predicates without a GPU: the decision function of str.starts_with / ends_with / contains (polars_amd/csrc/strmatch.hpp) through its host twin
plx_strview_match_host against Python's bytes.startswith / endswith / in (cross-checked with pyarrow.compute) over the corpus of tests/str_match_corpus.py, its
error cases, the mirror API (Expr.str), the lowering to PLX_AE_BITMAP_LOOKUP on placeholder frames, the fused programs the C++ compiler emits for plans that hold a
string predicate (interpreted row by row: tests/program_eval.py) against numpy, and the same decision function under AddressSanitizer as a stand-alone program."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests import program_eval
from tests import program_eval_select as pes
from tests import str_match_corpus as K
from tests.test_program_eval_cpu import by_key, close, frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = pl.col
ERR_INVALID = 1


@pytest.fixture(scope="module")
def corpus():
    views, data = K.views_of(K.STRINGS)
    assert len(data) > 0 and any(int(v[0]) & 0xFFFFFFFF > 12 for v in views)
    refs = {(kind, p): K.reference(kind, K.STRINGS, p) for kind in K.KINDS for p in K.PATTERNS}        # computed once, shared, never changed
    return views, data, refs


@pytest.fixture
def pe(monkeypatch):
    """program_eval whose run_rows knows OP_SELECT (when/then/otherwise)."""
    monkeypatch.setattr(program_eval, "run_rows", pes.run_rows)
    return program_eval


# ---- the decision function through its host twin --------------------------------------------------------------------------------------
def test_python_reference_agrees_with_pyarrow(corpus):
    _, _, refs = corpus
    for (kind, p), want in refs.items():
        assert K.arrow_reference(kind, K.STRINGS, p) == want, (K.KINDS[kind], p)
    # the properties the kernel is built around, stated on the reference itself
    assert refs[(F.STR_CONTAINS, "c\0")][K.STRINGS.index("abc")] is False and refs[(F.STR_ENDS_WITH, "c\0")][K.STRINGS.index("abc")] is False
    assert refs[(F.STR_CONTAINS, "\0")][K.STRINGS.index("ab\0cd")] is True and refs[(F.STR_ENDS_WITH, "\0")][K.STRINGS.index("abc\0")] is True
    assert all(v is True for v, s in zip(refs[(F.STR_STARTS_WITH, "")], K.STRINGS) if s is not None)
    assert refs[(F.STR_STARTS_WITH, "PROMO")].count(True) >= 4 and refs[(F.STR_STARTS_WITH, "PROM")].count(True) > refs[(F.STR_STARTS_WITH, "PROMO")].count(True)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_host_twin_matches_the_reference(corpus, n):
    views, data, refs = corpus
    v = K.tile_views(views, n)
    for (kind, p), ref in refs.items():
        st, got, valid, (wb, wv) = K.host_match(v, data, kind, p)
        assert st == 0, F.lib().plx_last_error()
        want, want_valid = K.split(K.tile(ref, n))
        assert np.array_equal(got, want) and np.array_equal(valid, want_valid), (K.KINDS[kind], p, n)
        if n % 64:      # the bits past n in the last word are zero
            assert int(wb[-1]) >> (n % 64) == 0 and int(wv[-1]) >> (n % 64) == 0


def test_host_twin_error_cases(corpus):
    views, data, refs = corpus
    lib = F.lib()
    long_rows = [i for i, s in enumerate(K.STRINGS) if s is not None and len(s.encode()) > 12]
    longs = views[long_rows]
    # a view whose offset + len passes the pool
    bad = longs.copy()
    bad[1, 1] = (int(bad[1, 1]) & 0xFFFFFFFF) | ((len(data) - 3) << 32)
    st, got, _, _ = K.host_match(bad, data, F.STR_ENDS_WITH, "tail")
    assert st == ERR_INVALID and "points outside its buffer" in lib.plx_last_error().decode()
    far = longs.copy()
    far[0, 1] = (int(far[0, 1]) & 0xFFFFFFFF) | (0xFFFFFFF0 << 32)
    assert K.host_match(far, data, F.STR_CONTAINS, "PROMO")[0] == ERR_INVALID
    other_buffer = longs.copy()
    other_buffer[0, 1] = int(other_buffer[0, 1]) | 1                       # buffer index 1: there is one buffer
    assert K.host_match(other_buffer, data, F.STR_CONTAINS, "PROMO")[0] == ERR_INVALID
    huge = longs.copy()
    huge[0, 0] = (int(huge[0, 0]) & ~0xFFFFFFFF) | 0x7FFFFFFF              # a length far beyond the pool
    assert K.host_match(huge, data, F.STR_ENDS_WITH, "x")[0] == ERR_INVALID
    # long strings need the pool ...
    for kind, p in ((F.STR_ENDS_WITH, "x"), (F.STR_CONTAINS, "PROMO"), (F.STR_STARTS_WITH, "PROMO")):
        st, _, _, _ = K.host_match(longs, data, kind, p, data_none=True)
        assert st == ERR_INVALID and "needs the data buffer" in lib.plx_last_error().decode(), (kind, p)
    # ... but not for starts_with of at most four bytes: the prefix is in the view
    for p in ("", "P", "PRO", "PROM", "STAN", "zero", "hél"):
        st, got, valid, _ = K.host_match(longs, data, F.STR_STARTS_WITH, p, data_none=True)
        want, _ = K.split([refs[(F.STR_STARTS_WITH, p)][i] if (F.STR_STARTS_WITH, p) in refs else K.reference(F.STR_STARTS_WITH, [K.STRINGS[i]], p)[0] for i in long_rows])
        assert st == 0 and np.array_equal(got, want) and valid.all(), p
    # and a five-byte prefix whose first four bytes already differ never reaches the pool either
    st, got, _, _ = K.host_match(longs, data, F.STR_STARTS_WITH, "QROMO", data_none=True)
    assert st == 0 and not got.any()
    # inline strings never need it
    inline = views[[i for i, s in enumerate(K.STRINGS) if s is None or len(s.encode()) <= 12]]
    for kind in K.KINDS:
        assert K.host_match(inline, data, kind, "abc", data_none=True)[0] == 0
    # the pattern limit is 64 bytes and the message names it
    assert K.host_match(views, data, F.STR_CONTAINS, "y" * 64)[0] == 0
    assert K.host_match(views, data, F.STR_CONTAINS, "y" * 65)[0] == F.ERR_UNSUPPORTED and "64 bytes" in lib.plx_last_error().decode()
    assert K.host_match(views, data, 3, "y")[0] == ERR_INVALID


def test_the_decision_function_under_address_sanitizer(corpus, tmp_path):
    """tests/emu/strmatch_main.cpp: match_view / match_views_host (the body the kernel and plx_strview_match_host share) as a stand-alone program built with
    -fsanitize=address,undefined, over the corpus and over views that point outside the pool -- views and pool sit in heap blocks of exactly their size."""
    views, data, refs = corpus
    exe = str(tmp_path / "strmatch_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "strmatch_main.cpp")], check=True)

    def write(path, v, cases):
        n, words = len(v), (len(v) + 63) // 64
        with open(path, "wb") as f:
            f.write(struct.pack("<QQQ", n, len(data), len(cases)) + np.ascontiguousarray(v).tobytes() + data)
            for kind, p, no_data, flags, want in cases:
                pb = K.as_bytes(p)
                bits, valid = K.split(want)
                pack = lambda b: np.packbits(np.concatenate([b, np.zeros(words * 64 - n, bool)]), bitorder="little").tobytes()
                f.write(struct.pack("<iIII", kind, len(pb), int(no_data), flags) + pb + pack(bits) + pack(valid))

    n = 129
    good = str(tmp_path / "good.bin")
    write(good, K.tile_views(views, n), [(kind, p, False, 0, K.tile(ref, n)) for (kind, p), ref in refs.items()])
    # out-of-range views: every long view moved so that its last byte lies just past the pool, or far away; without the pool.  Such rows answer false and raise a flag
    long_rows = [i for i, s in enumerate(K.STRINGS) if s is not None and len(s.encode()) > 12]
    past = views.copy()
    for i in long_rows:
        past[i, 1] = (int(past[i, 1]) & 0xFFFFFFFF) | ((len(data) - (int(past[i, 0]) & 0xFFFFFFFF) + 1) << 32)
    far = views.copy()
    for i in long_rows:
        far[i, 1] = (int(far[i, 1]) & 0xFFFFFFFF) | (0xFFFFFF00 << 32)
    inline_only = lambda ref: [v if (s is None or len(s.encode()) <= 12) else False for v, s in zip(ref, K.STRINGS)]
    bad = str(tmp_path / "bad.bin")
    for j, v in enumerate((past, far)):
        cases = [(kind, p, False, 1, inline_only(refs[(kind, p)])) for kind in (F.STR_ENDS_WITH, F.STR_CONTAINS) for p in ("a", "rld", "PROMO PL", " and a forty-byte ta")]
        cases += [(kind, "PROMO PL", True, 2, inline_only(refs[(kind, "PROMO PL")])) for kind in K.KINDS]
        cases += [(F.STR_STARTS_WITH, "PROM", True, 0, refs[(F.STR_STARTS_WITH, "PROM")])]          # decided from the prefix: no flag, the full answer
        write(bad + str(j), v, cases)
    for path in (good, bad + "0", bad + "1"):
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "bad=0" in r.stdout, (path, r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---- the mirror API ---------------------------------------------------------------------------------------------------------------------
def test_expr_str_namespace_and_errors():
    e = c("s").str.starts_with("PROMO")
    assert isinstance(e, pl.Expr) and e.kind == "str_match" and e.op == F.STR_STARTS_WITH and e.value == "PROMO" and e.lhs.kind == "col"
    assert repr(e) == "col('s').str.starts_with('PROMO')"
    assert repr(c("s").str.ends_with("x")) == "col('s').str.ends_with('x')" and repr(c("s").str.contains(b"a\0")) == "col('s').str.contains(b'a\\x00')"
    assert repr(~e) == "~col('s').str.starts_with('PROMO')"
    both = e & (c("x") > 0)
    assert both.kind == "binary" and both.op == F.OP_AND and both.lhs is e
    w = pl.when(e).then(c("x")).otherwise(0)
    assert w.kind == "ternary" and w.cond is e and repr(w) == "when(col('s').str.starts_with('PROMO')).then(col('x')).otherwise(lit(0))"
    assert c("s").str.contains("a", literal=True).op == F.STR_CONTAINS
    with pytest.raises(TypeError, match="regular expressions are not on this path"):
        c("s").str.contains("a.*", literal=False)
    for bad in (c("t"), c("t") + "x", 3, None):
        with pytest.raises(TypeError, match="literal"):
            c("s").str.starts_with(bad)
        with pytest.raises(TypeError, match="literal"):
            c("s").str.contains(bad)
    from polars_amd import io
    assert io.expr_columns(pl.when(c("s").str.ends_with("x")).then(c("a")).otherwise(c("b"))) == {"s", "a", "b"}


# ---- lowering and the fused programs, on placeholder frames ------------------------------------------------------------------------------
CATS = ["PROMO BURNISHED TIN", "STANDARD PLATED STEEL", "PROMO ANODIZED COPPER", "ECONOMY PROMO", "SMALL BRUSHED BRASS", "PROMO", "LARGE PROM", "MEDIUM POLISHED NICKEL PROMO"]


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(41)
    n = 2001
    cols = {"t": (rng.integers(0, len(CATS), n).astype(np.uint8), rng.random(n) < 0.8), "u": (rng.integers(0, len(CATS), n).astype(np.uint32), None),
            "k": (rng.integers(0, 4, n).astype(np.int64), None), "x": (rng.normal(size=n), rng.random(n) < 0.85), "y": (rng.integers(-9, 9, n).astype(np.int64), None)}
    df = frame_like(cols, {"t": pl.Categorical(CATS, pl.UInt8), "u": pl.Categorical(CATS, pl.UInt32)})
    return cols, df


def pred_of(cols, name, kind, pattern):
    """(values, validity) of the predicate per row, from the host strings: the reference of every plan check."""
    codes, valid = cols[name]
    ref = K.reference(kind, [CATS[i] for i in codes], pattern)
    v = np.array(ref, dtype=bool)
    return v, np.ones(len(v), bool) if valid is None else valid


def test_lowering_pushes_a_bitmap_lookup_over_the_codes(data, tmp_path):
    cols, df = data
    lf = df.lazy().filter(c("t").str.starts_with("PROMO")).select(c("x").sum())
    low, root, schema = lf._lower()
    looks = [d for d in low.aexprs if d["kind"] == F.AE_BITMAP_LOOKUP]
    assert F.AE_BITMAP_LOOKUP == 12 and len(looks) == 1
    look = looks[0]
    assert low.aexprs[look["lhs"]]["kind"] == F.AE_COLUMN and low.aexprs[look["lhs"]]["name"] == "t" and look["lut"] is low.lut_columns[0]
    assert np.array_equal(low.luts[0], [s.startswith("PROMO") for s in CATS]) and low.luts[0].dtype == bool
    assert low.notes == [f"str.starts_with('PROMO') over {len(CATS)} categories [host]"]
    # the bitmap's column handle crosses the ABI in the node's literal slot, and stays alive with the arenas
    ir, n_ir, ae, n_ae, keep = low.to_c()
    i = low.aexprs.index(look)
    assert ae[i].kind == 12 and ae[i].lit.u == look["lut"]._h != 0 and any(k is look["lut"] for k in keep)
    dt, n, nulls = C.c_int32(), C.c_int64(), C.c_int64()
    F.check(F.lib().plx_column_info(ae[i].lit.u, C.byref(dt), C.byref(n), C.byref(nulls)))
    assert (dt.value, n.value) == (F.BOOL, len(CATS))
    # dtype: Boolean wherever it is used; anything but a Categorical operand is refused in the style of the string comparisons
    assert df.lazy().select(c("t").str.contains("O").alias("p")).collect_schema() == {"p": pl.Boolean}
    for bad in (c("k"), c("x"), c("t") == "PROMO", pl.lit(3)):
        with pytest.raises(TypeError, match="needs a dictionary-encoded \\(Categorical\\) column"):
            df.lazy().filter(bad.str.starts_with("P"))._lower()
    with pytest.raises(F.UnsupportedError, match="64 bytes"):
        df.lazy().filter(c("t").str.contains("z" * 65))._lower()
    # the importer checks the node before it needs a device
    buf = C.create_string_buffer(1 << 12)
    ae[i].lit.u = df["x"]._h                                            # a Float64 column is no lookup bitmap
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) != 0 and "must be a Boolean column" in F.lib().plx_last_error().decode()
    ae[i].lit.u = 0
    assert F.lib().plx_debug_program_json(ir, n_ir, ae, n_ae, root, buf, len(buf)) != 0
    # the header: the kind's number, the pattern limit, and a layout that did not move
    src = tmp_path / "lookup.c"
    src.write_text(r'''
#include <stddef.h>
#include "polars_amd.h"
_Static_assert(PLX_AE_BITMAP_LOOKUP == 12 && PLX_AE_TERNARY == 11, "plx_aexpr_kind numbering");
_Static_assert(PLX_STR_STARTS_WITH == 0 && PLX_STR_ENDS_WITH == 1 && PLX_STR_CONTAINS == 2 && PLX_STR_MATCH_MAX_PATTERN >= 64, "plx_str_match_kind");
_Static_assert(offsetof(plx_aexpr, lit) == 24 && sizeof(((plx_aexpr*)0)->lit) == sizeof(plx_column), "the lookup bitmap's handle fits the literal slot");
int main(void) { return 0; }
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "lookup.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def bit_lookups(prog):
    return [op for op in prog["ops"] if op[0] == program_eval.OP_BITLOOKUP]


def test_filter_group_by_program(data):
    cols, df = data
    for name, kind, p in (("t", F.STR_STARTS_WITH, "PROMO"), ("u", F.STR_ENDS_WITH, "PROMO"), ("t", F.STR_CONTAINS, "PLATED"), ("t", F.STR_CONTAINS, "no such")):
        pred = getattr(c(name).str, K.KINDS[kind])(p)
        lf = df.lazy().filter(pred).group_by("k").agg(c("x").sum().alias("s"), pl.len().alias("n"), c("y").max().alias("m"))
        fus, _, why, _ = lf.describe_fusion()
        assert fus, why
        low, _, _ = lf._lower()
        prog = lf.debug_program()
        looks = bit_lookups(prog)
        assert len(looks) == 1 and looks[0][4] == 0 and looks[0][5] == "0"          # lookup bitmap 0, no key offset
        got = by_key(program_eval.evaluate(prog, cols, luts={0: low.luts[0]}), ["k"])
        pv, pm = pred_of(cols, name, kind, p)
        keep = pv & pm
        xv, xm = cols["x"]
        ks = sorted(set(cols["k"][0][keep].tolist()))
        assert sorted(k for (k,) in got) == ks, (name, p)
        for k in ks:
            sel = keep & (cols["k"][0] == k)
            assert got[(k,)]["n"] == int(sel.sum()) and close(got[(k,)]["s"], float(xv[sel & xm].sum())) and got[(k,)]["m"] == int(cols["y"][0][sel].max())
        assert program_eval.split_matches(prog, cols, {0: low.luts[0]})


def test_conditional_sum_program(data, pe):
    cols, df = data
    xv, xm = cols["x"]
    for name, kind, p in (("t", F.STR_STARTS_WITH, "PROMO"), ("u", F.STR_CONTAINS, "PROM"), ("t", F.STR_ENDS_WITH, "L")):
        pred = getattr(c(name).str, K.KINDS[kind])(p)
        lf = df.lazy().select(pl.when(pred).then(c("x")).otherwise(0.0).sum().alias("s"), pl.when(~pred).then(1).otherwise(0).sum().alias("n_not"), c("x").sum().alias("all"))
        fus, _, why, _ = lf.describe_fusion()
        assert fus, why                                                # one scan: the conditional aggregates and the plain one
        low, _, _ = lf._lower()
        assert len(low.luts) == 1                                      # pred and ~pred share one bitmap
        prog = lf.debug_program()
        assert len(bit_lookups(prog)) >= 1
        got = pe.evaluate(prog, cols, luts={i: l for i, l in enumerate(low.luts)})
        pv, pm = pred_of(cols, name, kind, p)
        t = pv & pm
        assert close(got["s"][0][0].item(), float(xv[t & xm].sum())) and close(got["all"][0][0].item(), float(xv[xm].sum()))
        assert got["n_not"][0][0].item() == int((~pv & pm).sum())       # ~null is null: a null row takes the otherwise branch


def test_boolean_group_key_program(data):
    cols, df = data
    xv, xm = cols["x"]
    for name, kind, p in (("t", F.STR_STARTS_WITH, "PROMO"), ("u", F.STR_CONTAINS, "BR")):
        pred = getattr(c(name).str, K.KINDS[kind])(p)
        lf = df.lazy().group_by(pred.alias("p")).agg(pl.len().alias("n"), c("x").sum().alias("s"))
        fus, _, why, _ = lf.describe_fusion()
        assert fus, why
        low, _, _ = lf._lower()
        got = by_key(program_eval.evaluate(lf.debug_program(), cols, luts={0: low.luts[0]}), ["p"])
        pv, pm = pred_of(cols, name, kind, p)
        want = {}
        for key, sel in ((True, pv & pm), (False, ~pv & pm), (None, ~pm)):
            if sel.any():
                want[(key,)] = (int(sel.sum()), float(xv[sel & xm].sum()))
        assert set(got) == set(want), (got.keys(), want.keys())
        for key, (n, s) in want.items():
            assert got[key]["n"] == n and close(got[key]["s"], s)


def test_a_third_bitmap_declines_fusion_with_a_reason(data):
    cols, df = data
    two = c("t").str.starts_with("PROMO") | c("u").str.ends_with("PROMO")
    assert df.lazy().filter(two).select(c("x").sum()).describe_fusion()[0]
    same = c("t").str.starts_with("PROMO")
    three = two & c("t").str.contains("TIN")
    fus, _, why, _ = df.lazy().filter(three).select(c("x").sum()).describe_fusion()
    assert not fus and "more than 2 lookup bitmaps" in why and "kMaxLuts" in why
    lf = df.lazy().filter(three).group_by("k").agg(pl.len())
    assert not lf.describe_fusion()[0]
    with pytest.raises(F.UnsupportedError, match="lookup bitmaps"):
        lf.debug_program()
    del same


def test_fused_join_pipelines_number_their_bitmaps(monkeypatch):
    """A string predicate on the build side and on the probe side of the fused join -> group-by: the count / build programs, the probe program and -- on a left join --
    the unmatched program, whose own membership bitmap takes index 0 so that the predicate's bitmap is number 1 there.  Interpreted against pandas merge -> groupby."""
    from tests.test_program_eval_cpu import _pandas_join_groupby
    rng = np.random.default_rng(77)
    nb, npr = 3_000, 25_000
    promo = [i for i, s in enumerate(CATS) if s.startswith("PROMO")]
    has_o = [i for i, s in enumerate(CATS) if "OMO" in s]
    bcols = {"k": (rng.integers(100, 1600, nb).astype(np.int64), None), "attr": (rng.integers(0, 4, nb).astype(np.int64), None), "flag": (rng.integers(0, 100, nb).astype(np.int64), None),
             "t": (rng.integers(0, len(CATS), nb).astype(np.uint8), rng.random(nb) < 0.9)}
    pcols = {"k": (rng.integers(0, 2500, npr).astype(np.int64), rng.random(npr) < 0.96), "v": (rng.integers(-50, 50, npr).astype(np.int64), None),
             "u": (rng.integers(0, len(CATS), npr).astype(np.uint32), rng.random(npr) < 0.9)}
    cat = {"t": pl.Categorical(CATS, pl.UInt8), "u": pl.Categorical(CATS, pl.UInt32)}
    aggs = (c("v").sum().alias("s"), pl.len().alias("n"))
    lookups = lambda p: [op[4] for op in p["ops"] if op[0] == program_eval.OP_BITLOOKUP]
    # build side, inner join
    lf = frame_like(pcols, cat).lazy().filter(c("v") > -45).join(frame_like(bcols, cat).lazy().filter(c("t").str.starts_with("PROMO")), on="k").group_by("k", "attr").agg(*aggs)
    fus, _, why, _ = lf.describe_fusion()
    assert fus, why
    low, _, _ = lf._lower()
    prog = lf.debug_program()
    assert prog["kind"] == "join_group_by" and prog["build_side"] == "right" and lookups(prog["build"]) == [0] and lookups(prog["count"]) == [0] and lookups(prog["probe"]) == []
    monkeypatch.setattr(program_eval, "build_luts", lambda prog, filter_cols: {0: low.luts[0]})
    got = by_key(program_eval.evaluate_join(prog, bcols, pcols), ["k", "attr"])
    want = _pandas_join_groupby(bcols, pcols, "inner", ["k", "attr"], bpred=lambda f: f["t"].isin(promo).fillna(False).astype(bool), ppred=lambda f: f["v"] > -45)
    assert got == want and len(want) > 300
    # probe side, left join: the unmatched program numbers its membership bitmap 0 and the predicate's 1
    lf = (frame_like(pcols, cat).lazy().filter(c("u").str.contains("OMO")).join(frame_like(bcols, cat).lazy().filter(c("flag") < 60), on="k", how="left").group_by("k", "attr").agg(*aggs))
    fus, _, why, _ = lf.describe_fusion()
    assert fus, why
    low, _, _ = lf._lower()
    prog = lf.debug_program()
    assert prog["how"] == "left" and lookups(prog["probe"]) == [0] and lookups(prog["build"]) == [] and prog["unmatched"]["lut"] == 0
    assert sorted(lookups(prog["unmatched"]["program"])) == [0, 1]
    # one dict serves all programs of the pipeline: the probe program reads the predicate's bitmap as number 0, the unmatched program as number 1.  evaluate_join
    # copies the dict for the unmatched program and THEN stores that program's membership bitmap under un["lut"] == 0 (asserted above), so the entry 0 given here
    # is replaced there and never read as a membership bitmap.
    monkeypatch.setattr(program_eval, "build_luts", lambda prog, filter_cols: {0: low.luts[0], 1: low.luts[0]})
    got = by_key(program_eval.evaluate_join(prog, bcols, pcols), ["k", "attr"])
    want = _pandas_join_groupby(bcols, pcols, "left", ["k", "attr"], bpred=lambda f: f["flag"] < 60, ppred=lambda f: f["u"].isin(has_o).fillna(False).astype(bool))
    assert got == want and len(want) > 1000 and any(k[1] is None for k in want)
