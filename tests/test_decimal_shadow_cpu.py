"""Decimal shadows of f64 columns without a GPU (csrc/decimal.hpp, csrc/encoded_inputs.hpp): the chooser and the decode through their host twins in the C ABI; the
program the compiler emits over a placeholder column that declares decimal32, interpreted row by row in numpy (tests/program_eval_decimal.py adds OP_DEC10, the
three-FMA constant-divisor division, to tests/program_eval.py) against the plain program over the decoded values (which are bit-identical, so every result is); the ahead-of-time shapes; the stand-alone sanitizer build of the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import datagen
from polars_amd import queries as Q
from tests import program_eval
from tests import program_eval_decimal as ped
from tests.test_encoded_inputs_cpu import AFFINE, DICT, SHAPE_Q1, SHAPE_Q1_ENCODED, declare, encoded_lineitem
from tests.test_program_eval_cpu import by_key, frame_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIMAL = 3
SHAPE_Q1_ENCODED_PRICE = 16
OP_CONST, OP_ADD_I, OP_DEC10 = 2, 7, ped.OP_DEC10       # fused.hpp OpCode


@pytest.fixture
def pe(monkeypatch):
    monkeypatch.setattr(program_eval, "run_rows", ped.run_rows)
    return program_eval


# ---- the chooser ---------------------------------------------------------------------------------------------------------------------------
def choose(values, valid=None):
    v = np.ascontiguousarray(values, dtype=np.float64)
    bits = None if valid is None else np.packbits(np.asarray(valid, bool), bitorder="little")
    ok, e, base = C.c_int32(), C.c_int32(), C.c_int64()
    F.check(F.lib().plx_encoding_choose_decimal(v.ctypes.data, None if bits is None else bits.ctypes.data, len(v), C.byref(ok), C.byref(e), C.byref(base)))
    return (e.value, base.value) if ok.value else None


def test_chooser_picks_the_smallest_exponent_and_the_base():
    assert choose([1.0, 250.0, 0.0]) == (0, 0)
    assert choose([1.5, 250.0]) == (1, 0)
    assert choose([1.25, 3.5, 100.0]) == (2, 0)
    assert choose([0.001, 7.0]) == (3, 0)
    assert choose([1e-9, 0.5]) == (9, 0)
    assert choose([0.0, 4294967295.0]) == (0, 0)                      # the whole code range, base 0
    assert choose([0.0, 42949672.95]) == (2, 0)
    assert choose([1.0, 4294967296.0]) == (0, 1)                      # past 2^32: the minimum becomes the base
    assert choose([-12.5, 3.0]) == (1, -125)                          # negative values: base = min
    assert choose([-0.01, 0.0]) == (2, -1)
    assert choose([2.0**53 - 1]) == (0, 2**53 - 1)
    assert choose([-(2.0**53) + 1, -(2.0**53) + 4294967296.0]) == (0, -(2**53) + 1)


def test_chooser_rejects():
    assert choose([0.0, 4294967296.0]) is None                        # a span of 2^32
    assert choose([-1.0, 4294967295.0]) is None
    assert choose([1e-10]) is None                                    # the exponent would have to be 10
    assert choose([1.5, float("nan")]) is None
    assert choose([1.5, float("inf")]) is None and choose([float("-inf")]) is None
    assert choose([1.5, -0.0]) is None                                # would decode to +0.0
    assert choose([2.0**53]) is None and choose([-(2.0**53)]) is None  # |k| >= 2^53
    assert choose([0.1 + 0.2]) is None and choose([0.3]) == (1, 0)    # 0.30000000000000004 is no decimal of nine digits; 0.3 is one
    assert choose([]) is None
    rng = np.random.default_rng(1)
    assert choose(900 + 1e5 * rng.random(1000)) is None               # arbitrary doubles


def test_chooser_ignores_null_rows_that_hold_garbage():
    v = np.array([1.25, np.nan, 2.5, -0.0, np.inf, 0.1 + 0.2, 1e300, 7.0])
    valid = np.array([1, 0, 1, 0, 0, 0, 0, 1], bool)
    assert choose(v) is None and choose(v, valid) == (2, 0)
    assert choose(v, np.zeros(8, bool)) is None                       # no valid row at all


# ---- the decode ----------------------------------------------------------------------------------------------------------------------------
def decode(base, e, codes):
    codes = np.ascontiguousarray(codes, dtype=np.uint32)
    out = np.empty(len(codes), np.float64)
    F.check(F.lib().plx_encoding_decimal_decode(base, e, codes.ctypes.data, len(codes), out.ctypes.data))
    return out


def test_decode_is_the_division_bit_for_bit():
    """The decode is the three-FMA form of the division by a constant; it must give what the IEEE division gives.  The evaluator's own div10 (exact rational
    arithmetic, rounded once per step) is held against both on a slice."""
    rng = np.random.default_rng(2)
    differs = 0
    for e in range(10):
        for base in (0, -123456789012, 2**52):
            codes = np.concatenate([rng.integers(0, 2**32, 50_000, dtype=np.uint64).astype(np.uint32), np.array([0, 1, 2**32 - 1], np.uint32)])
            k = base + codes.astype(np.int64)
            want = k.astype(np.float64) / 10.0**e
            assert np.array_equal(decode(base, e, codes).view(np.uint64), want.view(np.uint64)), (e, base)
            assert np.array_equal(ped.div10(k[:300].astype(np.float64), e).view(np.uint64), want[:300].view(np.uint64)), (e, base)
            if e:
                differs += int((want != k.astype(np.float64) * 10.0**-e).sum())
    assert differs > 1000      # the multiplication by 10^-e is another function: the decode has to divide


def test_host_encoder_round_trips_and_flags_mismatches():
    v = np.array([12.34, 0.0, 42949672.95, 42949672.96, -0.01, np.nan, -0.0, 0.1 + 0.2])
    codes, ok = np.zeros(len(v), np.uint32), np.zeros(len(v), np.uint8)
    F.check(F.lib().plx_encoding_decimal_encode(v.ctypes.data, len(v), 0, 2, codes.ctypes.data, ok.ctypes.data))
    assert ok.tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and codes[:3].tolist() == [1234, 0, 2**32 - 1]
    assert np.array_equal(decode(0, 2, codes[:3]).view(np.uint64), v[:3].view(np.uint64))


# ---- the rewritten program -------------------------------------------------------------------------------------------------------------------
def price_lineitem(n=5003, seed=3):
    """encoded_lineitem plus l_extendedprice as decimal32 (base 0, exponent 2)"""
    cols, codes, dicts, df = encoded_lineitem(n, seed)
    price = cols["l_extendedprice"][0]
    assert choose(price) == (2, 0)
    k = np.rint(price * 100.0).astype(np.int64)
    assert np.array_equal(decode(0, 2, k).view(np.uint64), price.view(np.uint64))
    codes["l_extendedprice"] = (k.astype(np.uint32), None)
    declare(df["l_extendedprice"], DECIMAL, 4, 0, 2)
    return cols, codes, dicts, df


def test_q1_program_over_the_decimal_price_equals_the_plain_program(pe):
    cols, codes, dicts, df = price_lineitem()
    plain = Q.q1(frame_like(cols, datagen.logical_dtypes(pl)).lazy()).debug_program()
    prog = Q.q1(df.lazy()).debug_program()
    assert prog["encoded"] == "encoded{l_shipdate:affine16,l_quantity:affine8,l_extendedprice:decimal32,l_discount:dict8,l_tax:dict8}"
    assert [i["dtype"] for i in prog["inputs"]] == [pe.U16, pe.U8, pe.U8, pe.U8, pe.U32, pe.U8, pe.U8]
    assert len(plain["ops"]) == 18 and len(prog["ops"]) == 27
    dec = [op for op in prog["ops"] if op[0] == OP_DEC10]
    assert len(dec) == 1 and dec[0][1] == dec[0][2] and dec[0][4] == 2      # base 0: the load and one op in place on its slot, the exponent in c
    prog["dicts"] = dicts
    se, pass_e = pe.run_rows(prog, codes)
    sp, pass_p = pe.run_rows(plain, cols)
    assert np.array_equal(pass_e, pass_p) and pe.live_out_slots(prog) == pe.live_out_slots(plain)
    for s in pe.live_out_slots(plain):
        assert np.array_equal(se[s][0], sp[s][0]) and np.array_equal(se[s][1], sp[s][1]), s
    keys = ["l_returnflag", "l_linestatus"]
    assert by_key(pe.evaluate(prog, codes), keys) == by_key(pe.evaluate(plain, cols), keys)


def test_select_program_with_a_nullable_decimal_input_equals_the_plain_program(pe):
    """The register-sink form; a nullable decimal column with a base (its null rows carry code 0 and hold garbage in the plain column), and one without."""
    rng = np.random.default_rng(4)
    n = 4001
    valid = rng.random(n) < 0.7
    kx = rng.integers(-5_000_000, 5_000_000, n)
    x = kx / 1000.0
    x[~valid] = np.where(rng.random(int((~valid).sum())) < 0.5, np.nan, 0.1 + 0.2)
    ky = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.int64)
    y = ky.astype(np.float64)
    cols = {"x": (x, valid), "y": (y, None), "p": (rng.integers(0, 100, n).astype(np.int64), None)}
    assert choose(x, valid) == (3, int(kx[valid].min())) and choose(y) == (0, 0)
    base = int(kx[valid].min())
    codes = {"x": (np.where(valid, kx - base, 0).astype(np.uint32), valid), "y": (ky.astype(np.uint32), None), "p": cols["p"]}
    assert np.array_equal(decode(base, 3, codes["x"][0])[valid].view(np.uint64), x[valid].view(np.uint64))
    df = frame_like(cols)
    declare(df["x"], DECIMAL, 4, base, 3)
    declare(df["y"], DECIMAL, 4, 0, 0)

    def q(frame):
        c = pl.col
        return frame.lazy().filter((c("p") < 70) & (c("x") > -2000.0)).select(c("x").sum().alias("sx"), c("x").min().alias("mx"), c("x").count().alias("cx"), (c("x") * c("y")).sum().alias("sxy"),
                                                                            c("y").max().alias("my"))
    plain, prog = q(frame_like(cols)).debug_program(), q(df).debug_program()
    assert prog["encoded"] == "encoded{x:decimal32,y:decimal32}", prog["encoded"]
    kinds = [op[0] for op in prog["ops"]]
    assert kinds.count(OP_DEC10) == 2 and sorted(op[4] for op in prog["ops"] if op[0] == OP_DEC10) == [0, 3]
    assert len(prog["ops"]) == len(plain["ops"]) + 3 + 1 and kinds.count(OP_ADD_I) == [op[0] for op in plain["ops"]].count(OP_ADD_I) + 1      # x: const, add, dec10; y: dec10
    got, want = pe.evaluate(prog, codes), pe.evaluate(plain, cols)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k][0]).view(np.uint64) if np.asarray(got[k][0]).dtype == np.float64 else got[k][0],
                              np.asarray(want[k][0]).view(np.uint64) if np.asarray(want[k][0]).dtype == np.float64 else want[k][0]) and (got[k][1] is None) == (want[k][1] is None), k


def test_static_shapes():
    cols, _, _, df5 = price_lineitem(n=1 << 12)
    ok, sid, why, _ = Q.q1(df5.lazy()).describe_fusion()
    assert ok and sid == SHAPE_Q1_ENCODED_PRICE, (ok, sid, why)
    _, _, _, df4 = encoded_lineitem(n=1 << 12)
    ok, sid, why, _ = Q.q1(df4.lazy()).describe_fusion()
    assert ok and sid == SHAPE_Q1_ENCODED, (ok, sid, why)
    ok, sid, why, _ = Q.q1(frame_like(cols, datagen.logical_dtypes(pl)).lazy()).describe_fusion()
    assert ok and sid == SHAPE_Q1, (ok, sid, why)


def test_placeholder_encoding_checks_its_arguments():
    df = frame_like({"x": (np.zeros(8), None), "i": (np.zeros(8, np.int64), None)})
    lib = F.lib()
    assert lib.plx_column_placeholder_encoding(df["x"]._h, DECIMAL, 4, -5, 9) == 0
    assert lib.plx_column_placeholder_encoding(df["x"]._h, DECIMAL, 4, 0, 10) != 0      # exponent 0..9
    assert lib.plx_column_placeholder_encoding(df["x"]._h, DECIMAL, 2, 0, 2) != 0       # width 4 only
    assert lib.plx_column_placeholder_encoding(df["i"]._h, DECIMAL, 4, 0, 2) != 0       # f64 only
    assert lib.plx_column_placeholder_encoding(df["x"]._h, AFFINE, 4, 0, 1) != 0 and lib.plx_column_placeholder_encoding(df["x"]._h, DICT, 1, 0, 0) != 0      # kinds 1 and 2 keep their checks


def test_a_program_too_long_for_the_decode_runs_plain():
    """32 ops is the limit: a program of 32 ops has no room for the one op of a base-0 decode; a shorter one takes it."""
    rng = np.random.default_rng(5)
    cols = {"x": (np.round(rng.random(64) * 100, 2), None)}

    def q(frame, terms, square):      # 1 + 2 * terms ops, one more with the square
        e = pl.col("x")
        for i in range(terms):
            e = e + float(i + 1)
        return frame.lazy().select((e * e if square else e).sum().alias("s"))
    lengths = {}
    for terms, square in ((13, False), (14, True), (15, False), (15, True)):
        df = frame_like(cols)
        declare(df["x"], DECIMAL, 4, 0, 2)
        plain, prog = q(frame_like(cols), terms, square).debug_program(), q(df, terms, square).debug_program()
        lengths[len(plain["ops"])] = "encoded" in prog
        assert len(prog["ops"]) == len(plain["ops"]) + (1 if "encoded" in prog else 0) <= 32
    assert 31 in lengths and 32 in lengths and all(took == (n + 1 <= 32) for n, took in lengths.items()), lengths


def test_min_rows_setter_and_getter():
    before = F.encoded_decimal_min_rows()
    try:
        F.encoded_set_decimal_min_rows(0)
        assert F.encoded_decimal_min_rows() == 0
        F.encoded_set_decimal_min_rows(12345)
        assert F.encoded_decimal_min_rows() == 12345
    finally:
        F.encoded_set_decimal_min_rows(before)
    assert before == int(os.environ.get("PLX_ENCODED_DECIMAL_MIN_ROWS", 1 << 22))


# ---- the header alone, under the sanitizers ----------------------------------------------------------------------------------------------------
def test_the_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/emu/decimal_main.cpp: chooser, per-row encoder and decode over the edge values, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "decimal_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "decimal_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
