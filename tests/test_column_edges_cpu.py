"""Pins the tables and references of tests/column_edges.py without a GPU: the cast references against the oracle's long-double restatement (orc_cast) on
every row of every table, the float32 rounding helper against numpy, the reduce references on cases small enough to check by hand, and the shape of the
tables (which edges they hold)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import column_edges as E


def orc_cast(orc, a, to):
    ev = np.zeros(len(a), dtype=E.NP[to]); okb = np.zeros((len(a) + 7) // 8 + 8, dtype=np.uint8)
    rc = orc.lib().orc_cast(orc.DT_OF[a.dtype], orc.DT_OF[np.dtype(E.NP[to])], a.ctypes.data_as(C.c_void_p), C.c_int64(len(a)), ev.ctypes.data_as(C.c_void_p), okb.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return ev, orc.unpack(okb, len(a))


@pytest.mark.parametrize("frm", E.DTYPES)
def test_cast_references_agree_with_the_oracle_on_every_row(orc, frm):
    a = E.cast_table(frm)
    for to in E.DTYPES:
        want, ok = E.cast_reference(a, to)
        got, got_ok = orc_cast(orc, a, to)
        assert np.array_equal(ok, got_ok), (frm, to, a[ok != got_ok][:8])
        assert E.same_values(got[ok], want[ok]), (frm, to, a[ok][got[ok] != want[ok]][:8])
        assert not want[~ok].any()


def test_int_to_f32_rounds_like_numpy():
    vals = set()
    for k in range(23, 65):
        for d in range(-3, 4):
            vals.add((1 << k) + d)
            vals.add((1 << k) + (1 << (k - 24)) + d if k >= 24 else 0)      # the tie between two neighbours, and around it
            vals.add((1 << k) + 3 * (1 << (k - 24)) + d if k >= 24 else 0)
    rng = np.random.default_rng(5)
    vals |= set(int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, 2000, dtype=np.int64))
    signed = [v for v in vals if -2 ** 63 <= v < 2 ** 63] + [-v for v in vals if 0 < v <= 2 ** 63]
    unsigned = [v for v in vals if 0 <= v < 2 ** 64]
    for xs, dt in ((signed, np.int64), (unsigned, np.uint64)):
        a = np.array(xs, dtype=dt)
        want = a.astype(np.float32)
        got = np.array([E.int_to_f32(int(x)) for x in a], dtype=np.float32)
        assert E.same_values(got, want), a[got != want][:8]
    assert E.int_to_f32(2 ** 24 + 1) == 2 ** 24 and E.int_to_f32(2 ** 24 + 3) == 2 ** 24 + 4 and E.int_to_f32(2 ** 64 - 1) == 2.0 ** 64 and E.int_to_f32(-(2 ** 24) - 3) == -(2 ** 24) - 4


def test_the_cast_tables_hold_the_edges():
    f32, f64 = E.cast_table("f32"), E.cast_table("f64")
    for t in (f32, f64):
        assert len(t) > 128 and len(t) % 2 == 1
        for v in (2.0 ** 31, 2.0 ** 63, 2.0 ** 64, 256.0, -0.5, -1.0, -129.0, 65536.0):
            assert v in t, v
        assert np.isnan(t).sum() >= 2 and np.inf in t and -np.inf in t and np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all()
    assert np.nextafter(np.float32(256.0), np.float32(0)) in f32 and 2147483647.0 in f64 and 4294967295.0 in f64
    assert np.nextafter(2147483648.0, 0.0) in f64 and np.nextafter(-1.0, 0.0) in f64 and np.nextafter(np.float32(-1.0), np.float32(0)) in f32
    # f64 -> f32: ties, overflow, denormal results
    with np.errstate(over="ignore"):
        r = f64.astype(np.float32)
    assert np.isinf(r[np.isfinite(f64)]).any() and ((r != 0) & (np.abs(r) < np.finfo(np.float32).tiny)).any() and ((r == 0) & (f64 != 0)).any()
    assert E.cast_reference(np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]), "f32")[0].tolist() == [1.0, 1.0 + 2.0 ** -22]
    i64, u64, i8 = E.cast_table("i64"), E.cast_table("u64"), E.cast_table("i8")
    for v in (-2 ** 63, 2 ** 63 - 1, -129, -128, 127, 128, 255, 256, 2 ** 31, -2 ** 31 - 1, 2 ** 32, 2 ** 24 + 1, -(2 ** 53) - 3):
        assert v in [int(x) for x in i64], v
    assert 2 ** 64 - 1 in [int(x) for x in u64] and 2 ** 63 in [int(x) for x in u64] and sorted(set(int(x) for x in i8)) == [-128, -1, 0, 1, 127]


def test_cast_reference_by_hand():
    v, ok = E.cast_reference(np.array([255.5, 256.0, -0.5, -1.0, np.nan, np.inf, -0.0], dtype=np.float64), "u8")
    assert ok.tolist() == [True, False, True, False, False, False, True] and v.tolist() == [255, 0, 0, 0, 0, 0, 0]
    v, ok = E.cast_reference(np.array([2.0 ** 63, np.nextafter(2.0 ** 63, 0), -2.0 ** 63, np.nextafter(-2.0 ** 63, -np.inf)]), "i64")
    assert ok.tolist() == [False, True, True, False] and v.tolist() == [0, 2 ** 63 - 1024, -2 ** 63, 0]
    v, ok = E.cast_reference(np.array([-1, 0, 2 ** 32 - 1, 2 ** 32], dtype=np.int64), "u32")
    assert ok.tolist() == [False, True, True, False] and v.tolist() == [0, 0, 2 ** 32 - 1, 0]
    v, ok = E.cast_reference(np.array([2 ** 53 + 1, 2 ** 53 + 3, 2 ** 63 - 1], dtype=np.int64), "f64")
    assert ok.all() and v.tolist() == [2.0 ** 53, 2.0 ** 53 + 4, 2.0 ** 63]


def test_reduce_reference_by_hand():
    nan, inf = math.nan, math.inf
    r = E.reduce_reference(np.array([nan, 1.0, -3.0, nan]))
    assert r["count"] == 4 and r["min"] == -3.0 and r["max"] == 1.0 and math.isnan(r["sum"]) and math.isnan(r["mean"])
    r = E.reduce_reference(np.array([nan, 1.0, -3.0, nan]), np.array([False, True, True, False]))
    assert (r["count"], r["sum"], r["mean"], r["min"], r["max"]) == (2, -2.0, -1.0, -3.0, 1.0)
    r = E.reduce_reference(np.array([nan, nan], dtype=np.float32))
    assert math.isnan(r["min"]) and math.isnan(r["max"]) and math.isnan(r["mean"])
    r = E.reduce_reference(np.array([1.0, 2.0]), np.zeros(2, bool))
    assert r["count"] == 0 and r["min"] is None and r["max"] is None and r["mean"] is None
    assert math.isnan(E.reduce_reference(np.array([inf, -inf, 1.0]))["sum"]) and E.reduce_reference(np.array([inf, 1.0]))["sum"] == inf
    r = E.reduce_reference(np.array([2 ** 31 - 1, 1, 5], dtype=np.int32))
    assert (r["sum"], r["min"], r["max"], r["mean"]) == (-2 ** 31 + 5, 1, 2 ** 31 - 1, Fraction(2 ** 31 + 5, 3))
    assert E.reduce_reference(np.array([2 ** 32 - 1, 2], dtype=np.uint32))["sum"] == 1
    assert E.reduce_reference(np.array([127, 127], dtype=np.int8))["sum"] == 254 and E.reduce_reference(np.array([255, 255], dtype=np.uint8))["sum"] == 510
    r = E.reduce_reference(np.array([2 ** 64 - 1, 2 ** 63 + 1, 3], dtype=np.uint64))
    assert (r["sum"], r["max"], r["min"]) == ((2 ** 64 - 1 + 2 ** 63 + 1 + 3) % 2 ** 64, 2 ** 64 - 1, 3)
    r = E.reduce_reference(np.array([-2 ** 63, 2 ** 63 - 1, -2 ** 63], dtype=np.int64))
    assert (r["sum"], r["min"], r["max"]) == (2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1)


def test_reduce_shapes_and_validity_patterns():
    for dt in E.DTYPES:
        v, n = E.vec(dt), E.reduce_rows(dt)
        assert n % (64 * v) == 3 and n // (64 * v) == 81 and n <= 100_000 and all(0 <= r < n for r in E.lone_rows(dt)) and len(set(E.lone_rows(dt))) == (8 if v == 2 else 9)
        w = E.walk_validity(n)
        words = np.add.reduceat(w.astype(np.int64), np.arange(0, n, 64))
        assert words[:-1].tolist() == [1] * (len(words) - 1) and w[0] and w[64 + 7] and w[128 + 14] and w[64 * 10 + 6]
        assert set(np.flatnonzero(w) % 64) == set(range(64))                      # every bit position of a word, so every lane and every in-pack shift
        a = E.walk_values(dt, n)
        assert a.min() >= 1 and E.word_validity(n)[:64].all() and not E.word_validity(n)[64:128].any()
    assert E.wrap(2 ** 31, "i32") == -2 ** 31 and E.wrap(-1, "u64") == 2 ** 64 - 1 and E.wrap(5, "i64") == 5


def test_bool_operands_hold_every_pair_at_both_ends():
    for n in E.BOOL_LENGTHS:
        (a, av), (b, bv) = E.bool_operands(n)
        pairs = lambda s: {(None if not av[i] else bool(a[i]), None if not bv[i] else bool(b[i])) for i in range(*s.indices(n))}
        if n >= 9:
            assert pairs(slice(0, 9)) == set(E.COMBOS) and pairs(slice(n - 9, n)) == set(E.COMBOS)
        if n % 64 >= 9 or n % 64 == 0:
            assert pairs(slice((n - 1) // 64 * 64, n)) == set(E.COMBOS)
        assert a[~av].all() and not b[~bv].any()
    t, f = np.array([True]), np.array([False])
    assert E.kleene("and", f, t, t, f) == (f, t) and E.kleene("and", t, t, t, f)[1] == f and E.kleene("or", t, t, f, f)[1] == t and E.kleene("or", f, t, f, f)[1] == f
    assert E.kleene("xor", t, t, f, f)[1] == f
    assert [bool(E.bool_cmp_reference(op, f, t)[0]) for op in range(6)] == [False, True, True, True, False, False]


def test_concat_offsets_and_filter_frames():
    off = E.concat_offsets()
    assert len(E.CONCAT_LENGTHS) >= 8 and E.CONCAT_LENGTHS[0] == 0 and E.CONCAT_LENGTHS[-1] == 0 and set(E.CONCAT_LENGTHS) <= {0, 1, 31, 63, 64, 65, 200}
    assert {0, 1, 31, 63, 33} <= {o % 64 for o, n in zip(off, E.CONCAT_LENGTHS) if n}
    assert off[1] // 64 == off[2] // 64 == off[3] // 64 and E.CONCAT_LENGTHS[1] + E.CONCAT_LENGTHS[2] < 64      # three chunks meet in output word 0
    assert any(E.concat_chunk(k, 5)["a"][1] is None for k in range(3)) and any(E.concat_chunk(k, 5)["a"][1] is not None for k in range(3))
    widths = sorted(np.dtype(E.NP[d]).itemsize for d in E.DENSE_COLUMNS if d != "bool")
    assert widths == [1] * 3 + [2] * 3 + [4] * 4 + [8] * 4 and E.DENSE_COLUMNS.count("bool") == 1 and len(E.SPARSE_COLUMNS) == 9
    for c, dt in enumerate(E.DENSE_COLUMNS):
        x = E.stamped(dt, c, 20_011)
        if dt in ("i64", "u64"):
            assert int(x[20_010]) == 20_010 * E.PRIMES[c] + c
        if E.is_float(dt):
            assert np.array_equal(x, x.astype(np.int64).astype(x.dtype))
    for dt in E.DTYPES:
        x = E.window_values(dt, 300)
        assert (x != 0).all() and ((x < 0).any() == (dt[0] != "u"))
