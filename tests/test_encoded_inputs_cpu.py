"""Encoded shadows without a GPU: the program the compiler emits over encoded inputs (placeholder columns that declare their encoding), interpreted row by row in
numpy (tests/program_eval_dict.py adds OP_DICT to tests/program_eval.py), against the plain program over the decoded values; the ahead-of-time shape of the encoded
Q1; the affine chooser."""
import ctypes as C

import numpy as np
import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import datagen
from polars_amd import queries as Q
from tests import program_eval
from tests import program_eval_dict as ped
from tests.test_program_eval_cpu import by_key, frame_like

AFFINE, DICT = 1, 2
SHAPE_Q1, SHAPE_Q1_ENCODED = 3, 15


@pytest.fixture
def pe(monkeypatch):
    monkeypatch.setattr(program_eval, "run_rows", ped.run_rows)
    return program_eval


def declare(series, kind, width, base=0, stride=1):
    F.check(F.lib().plx_column_placeholder_encoding(series._h, kind, width, base, stride))


def encoded_lineitem(n=5003, seed=3):
    """-> (plain columns, the same columns as codes, dictionaries, the placeholder frame that declares the encodings)"""
    li = datagen.lineitem_host(n, seed=seed)
    cols = {k: (li[k], None) for k in datagen.LINEITEM_Q1_COLS}
    df = frame_like(cols, datagen.logical_dtypes(pl))
    ship, qty = li["l_shipdate"], li["l_quantity"]
    base, stride = int(ship.min()), datagen.DAY_US
    codes = dict(cols)
    codes["l_shipdate"] = (((ship - base) // stride).astype(np.uint16), None)
    codes["l_quantity"] = ((qty - int(qty.min())).astype(np.uint8), None)
    dicts = []
    for name in ("l_discount", "l_tax"):
        d, inv = np.unique(li[name].view(np.uint64), return_inverse=True)
        dicts.append(np.concatenate([d, np.zeros(256 - len(d), np.uint64)]))
        codes[name] = (inv.astype(np.uint8), None)
    declare(df["l_shipdate"], AFFINE, 2, base, stride)
    declare(df["l_quantity"], AFFINE, 1, int(qty.min()), 1)
    declare(df["l_discount"], DICT, 1)
    declare(df["l_tax"], DICT, 1)
    return cols, codes, dicts, df


def test_encoded_q1_program_equals_the_plain_program_on_decoded_inputs(pe):
    cols, codes, dicts, df = encoded_lineitem()
    plain = Q.q1(frame_like(cols, datagen.logical_dtypes(pl)).lazy()).debug_program()
    prog = Q.q1(df.lazy()).debug_program()
    assert prog["encoded"] == "encoded{l_shipdate:affine16,l_quantity:affine8,l_discount:dict8,l_tax:dict8}" and "encoded" not in plain
    assert [i["name"] for i in prog["inputs"]] == [i["name"] for i in plain["inputs"]]
    assert [i["dtype"] for i in prog["inputs"]] == [pe.U16, pe.U8, pe.U8, pe.U8, pe.F64, pe.U8, pe.U8]
    assert sum(op[0] == ped.OP_DICT for op in prog["ops"]) == 2 and len(prog["ops"]) == len(plain["ops"]) + 8
    prog["dicts"] = dicts
    # row by row: the predicate, the key and every aggregate source hold the same bits
    se, pass_e = pe.run_rows(prog, codes)
    sp, pass_p = pe.run_rows(plain, cols)
    assert np.array_equal(pass_e, pass_p) and pe.live_out_slots(prog) == pe.live_out_slots(plain)
    for s in pe.live_out_slots(plain):
        assert np.array_equal(se[s][0], sp[s][0]) and np.array_equal(se[s][1], sp[s][1]), s
    # and the query result is the same, bit for bit
    keys = ["l_returnflag", "l_linestatus"]
    assert by_key(pe.evaluate(prog, codes), keys) == by_key(pe.evaluate(plain, cols), keys)


def test_encoded_select_program_with_nulls_equals_the_plain_program(pe):
    """The register-sink form, a nullable encoded column (its null rows carry code 0), a stride without a base and a base without a stride."""
    rng = np.random.default_rng(4)
    n = 4001
    valid = rng.random(n) < 0.7
    a = 12 * rng.integers(0, 3000, n).astype(np.int64)
    b = -77 + rng.integers(0, 200, n).astype(np.int64)
    x = rng.integers(0, 5, n) / 8.0
    cols = {"a": (a, valid), "b": (b, None), "x": (x, valid)}
    df = frame_like(cols)
    d, inv = np.unique(x.view(np.uint64), return_inverse=True)
    codes = {"a": (np.where(valid, a // 12, 0).astype(np.uint16), valid), "b": ((b + 77).astype(np.uint8), None), "x": (np.where(valid, inv, 0).astype(np.uint8), valid)}
    declare(df["a"], AFFINE, 2, 0, 12)
    declare(df["b"], AFFINE, 1, -77, 1)
    declare(df["x"], DICT, 1)

    def q(frame):
        c = pl.col
        return frame.lazy().filter((c("a") > 6000) | (c("b") < 0)).select(c("a").sum().alias("sa"), c("a").max().alias("ma"), c("b").min().alias("mb"), (c("x") * 2.0).sum().alias("sx"), c("x").count().alias("cx"))
    plain, prog = q(frame_like(cols)).debug_program(), q(df).debug_program()
    assert prog["encoded"] == "encoded{a:affine16,b:affine8,x:dict8}"
    prog["dicts"] = [np.concatenate([d, np.zeros(256 - len(d), np.uint64)])]
    got, want = pe.evaluate(prog, codes), pe.evaluate(plain, cols)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k][0], want[k][0]) and (got[k][1] is None) == (want[k][1] is None), k


def test_q1_over_encoded_placeholders_hits_the_static_shape():
    cols, _, _, df = encoded_lineitem(n=1 << 12)
    ok, sid, why, _ = Q.q1(df.lazy()).describe_fusion()
    assert ok and sid == SHAPE_Q1_ENCODED, (ok, sid, why)
    ok, sid, why, _ = Q.q1(frame_like(cols, datagen.logical_dtypes(pl)).lazy()).describe_fusion()
    assert ok and sid == SHAPE_Q1, (ok, sid, why)


def choose(mn, mx, g=0):
    ok, width, needs = C.c_int32(), C.c_int32(), C.c_int32()
    base, stride = C.c_int64(), C.c_uint64()
    F.check(F.lib().plx_encoding_choose_affine(mn, mx, g, C.byref(ok), C.byref(width), C.byref(base), C.byref(stride), C.byref(needs)))
    return (bool(ok.value), width.value, base.value, stride.value) if ok.value else None, bool(needs.value)


def test_affine_chooser():
    i64 = np.iinfo(np.int64)
    assert choose(5, 5) == ((True, 1, 5, 1), False)                              # a constant column: gcd 0, zero codes
    assert choose(-3, -3 + 255) == ((True, 1, -3, 1), False)
    assert choose(-3, -3 + 256) == ((True, 2, -3, 1), False)
    assert choose(10, 10 + 65535) == ((True, 2, 10, 1), False)
    assert choose(10, 10 + 65536) == (None, True)                                 # needs the gcd pass; without one it does not encode
    assert choose(10, 10 + 65536, 1) == (None, True)
    assert choose(10, 10 + 65536, 2) == ((True, 2, 10, 2), True)
    day = 86_400_000_000
    assert choose(8036 * day, 8036 * day + 2645 * day, day) == ((True, 2, 8036 * day, day), True)
    assert choose(0, 255 * day, day) == ((True, 1, 0, day), True)
    assert choose(0, 256 * day, day) == ((True, 2, 0, day), True)
    assert choose(0, 65535 * day, day) == ((True, 2, 0, day), True)
    assert choose(0, 65536 * day, day) == (None, True)
    assert choose(0, 65535 * day, 0) == (None, True)                              # gcd 0 past the one-pass span: nothing to divide by
    assert choose(int(i64.min), int(i64.max), 1) == (None, False)                 # a span of 2^64 - 1
    assert choose(0, (1 << 62) - 1, (1 << 62) - 1) == ((True, 1, 0, (1 << 62) - 1), True)
    assert choose(0, 1 << 62, 1 << 62) == (None, False)                           # the span limit itself
    assert choose(int(i64.min), int(i64.min) + 255) == ((True, 1, int(i64.min), 1), False)
    assert choose(int(i64.max) - 65535, int(i64.max)) == ((True, 2, int(i64.max) - 65535, 1), False)
    assert choose(7, 3) == (None, False)                                          # max below min
