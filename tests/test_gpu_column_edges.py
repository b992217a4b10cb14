"""The column kernels behind the C ABI -- plx_cast, plx_reduce, plx_cmp on Booleans, plx_bitmap_binop / plx_bitmap_not, plx_if_then_else, fill_null, plx_filter,
plx_gather, plx_frame_concat and the compaction behind FusedFilter{} -- row by row at the edges random data does not reach: values next to a target type's range,
a lone ordered value among NaNs or nulls in every lane / wave / workgroup position, validity bits at every position of a word, bitmap pad bits, concatenation at
every bit offset, frames wider than one compaction launch, and borrowed buffers that start off a 16-byte boundary.

The tables and references are tests/column_edges.py (pinned without a GPU by tests/test_column_edges_cpu.py).  Comparisons are exact -- validity bit for bit,
integers and Booleans equal, floats as bit patterns with a NaN for a NaN -- except the two places that name a margin."""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import column_edges as E
from tests import expr_rows as R

pytestmark = pytest.mark.gpu
RTOL = 1e-6          # the project's margin for float aggregates (BASELINE north_star), used for the mean of i64 values only


def dtype_of(pl, dt):
    return pl.Boolean if dt == "bool" else getattr(pl, E.PLDT[dt])


def S(pl, name, arr, dt, valid=None):
    return pl.Series(name, arr, dtype=dtype_of(pl, dt), validity=valid)


def dl(s):
    v, ok = s._download()
    return v, (np.ones(len(v), bool) if ok is None else ok)


def raw_words(pl, s, which):
    """the 64-bit words of a column's values bitmap (0) or validity bitmap (1) as they lie in device memory, pad bits included"""
    ptr = s.device_ptrs()[which]
    assert ptr, "no such buffer"
    return pl.Series.from_device("w", pl.UInt64, ptr, (len(s) + 63) // 64, keepalive=s).to_numpy()


def pad_bits_clear(pl, s):
    n = len(s)
    if n % 64 == 0:
        return True
    pad = ~np.uint64((1 << (n % 64)) - 1)
    ok = not (raw_words(pl, s, 0)[-1] & pad)
    if s.device_ptrs()[1]:
        ok = ok and not (raw_words(pl, s, 1)[-1] & pad)
    return bool(ok)


def check(s, want_v, want_ok, what):
    """values on the valid rows, validity bit for bit, null_count"""
    v, ok = dl(s)
    assert len(v) == len(want_v), what
    assert np.array_equal(ok, want_ok), (what, np.flatnonzero(ok != want_ok)[:8])
    assert s.null_count() == int((~want_ok).sum()), what
    g, w = v[want_ok], np.asarray(want_v)[want_ok]
    if not E.same_values(g, w):
        bad = [i for i in range(min(len(g), len(w))) if not E.same_values(g[i:i + 1], w[i:i + 1])][:8]
        raise AssertionError((what, g.dtype, w.dtype, np.flatnonzero(want_ok)[bad].tolist(), g[bad].tolist(), w[bad].tolist()))


# ================================================================================================================== 1. casts
@functools.lru_cache(maxsize=None)
def cast_want(frm, to):
    return E.cast_reference(E.cast_table(frm), to)


@pytest.mark.parametrize("frm", E.DTYPES)
def test_cast_at_every_target_range_edge(pl, frm):
    """cast_kernel's cast_one<F, T> for every (from, to): floats next to each integer target's lo - 1, lo, hi, hi + 1 (2^31 and 2^63 as f32 and f64, 2^64, 255.x / 256.0,
    -0.5 / -1.0 into unsigned targets), integers at each target's bounds, i64 / u64 -> f32 / f64 at ties and above 2^63, f64 -> f32 ties / overflow / denormals.
    Output validity is input validity AND "representable"."""
    a = E.cast_table(frm)
    for n in E.CUTS + [len(a)]:
        for valid in (None, E.every_third_null(n)):
            s = S(pl, "a", a[:n], frm, valid)
            in_ok = np.ones(n, bool) if valid is None else valid
            for to in E.DTYPES:
                want_v, want_ok = cast_want(frm, to)
                out = s.cast(dtype_of(pl, to))
                assert out._query_dtype().np_dtype == E.NP[to]
                check(out, want_v[:n], want_ok[:n] & in_ok, (frm, to, n, valid is not None))


@pytest.mark.parametrize("n", E.BOOL_LENGTHS)
def test_cast_from_boolean_to_every_dtype(pl, n):
    (a, av), _ = E.bool_operands(n)
    for valid in (None, av):
        s = S(pl, "b", a, "bool", valid)
        for to in E.DTYPES:
            check(s.cast(dtype_of(pl, to)), a.astype(E.NP[to]), np.ones(n, bool) if valid is None else valid, (to, n, valid is not None))


# ============================================================================================================= 2. reductions
def reductions(s):
    return {k: getattr(s, k)() for k in ("sum", "mean", "min", "max", "count")}


@pytest.mark.parametrize("dt", E.FLOATS)
def test_a_lone_ordered_value_survives_every_merge(pl, dt):
    """Acc::merge joins an accumulator that has seen no ordered value with one that has, in the wave tree, across the waves of a workgroup and in the finish kernel: every
    row is NaN (then: null) except one, placed in the first lane's first and last element, the second lane, the last lane of the first run, the second run, the
    middle, and the row tail."""
    n, x = E.reduce_rows(dt), -2.5
    for row in E.lone_rows(dt):
        a = np.full(n, np.nan, dtype=E.NP[dt])
        a[row] = x
        r = reductions(S(pl, "a", a, dt))
        assert r["min"] == x and r["max"] == x and r["count"] == n and math.isnan(r["mean"]) and math.isnan(r["sum"]), (dt, row, "NaN", r)
        valid = np.zeros(n, bool)
        valid[row] = True
        r = reductions(S(pl, "a", a, dt, valid))
        assert r == {"sum": x, "mean": x, "min": x, "max": x, "count": 1}, (dt, row, "null", r)
    for lo_row, hi_row in ((0, n - 1), (n - 1, 0), (E.vec(dt), n - 4)):       # two survivors at opposite ends
        a = np.full(n, np.nan, dtype=E.NP[dt])
        a[lo_row], a[hi_row] = -7.0, 3.0
        r = reductions(S(pl, "a", a, dt))
        assert r["min"] == -7.0 and r["max"] == 3.0 and math.isnan(r["mean"]), (dt, lo_row, hi_row, r)
        valid = np.zeros(n, bool)
        valid[[lo_row, hi_row]] = True
        r = reductions(S(pl, "a", a, dt, valid))
        assert r == {"sum": -4.0, "mean": -2.0, "min": -7.0, "max": 3.0, "count": 2}, (dt, lo_row, hi_row, r)


@pytest.mark.parametrize("dt", E.FLOATS)
def test_float_reductions_without_an_ordered_value_and_with_infinities(pl, dt):
    n = E.reduce_rows(dt)
    a = np.full(n, np.nan, dtype=E.NP[dt])
    r = reductions(S(pl, "a", a, dt))
    assert math.isnan(r["min"]) and math.isnan(r["max"]) and math.isnan(r["mean"]) and r["count"] == n, r
    r = reductions(S(pl, "a", a, dt, np.zeros(n, bool)))
    assert r["min"] is None and r["max"] is None and r["mean"] is None and r["count"] == 0 and r["sum"] == 0.0, r
    a = np.ones(n, dtype=E.NP[dt])
    a[1], a[n - 2] = np.inf, -np.inf
    r = reductions(S(pl, "a", a, dt))
    assert math.isnan(r["sum"]) and math.isnan(r["mean"]) and r["min"] == -math.inf and r["max"] == math.inf, r
    # a column of +0.0 and -0.0 only: which zero comes out depends on the order of the merges, which neither the kernel's contract nor the reference fixes
    # (-0.0 < +0.0 is false either way), so the sign is not compared
    a = np.zeros(n, dtype=E.NP[dt])
    a[::3] = -0.0
    r = reductions(S(pl, "a", a, dt))
    assert r["min"] == 0.0 and r["max"] == 0.0 and r["sum"] == 0.0 and r["mean"] == 0.0, r


@pytest.mark.parametrize("dt", E.FLOATS)
def test_float_sums_of_integer_valued_data_are_exact(pl, dt):
    """sum |x| stays below 2^53 (f64) / 2^24 (f32): every partial sum is an integer the accumulator holds exactly, so the sum is the same in any order and
    equals math.fsum; the mean is that sum divided once."""
    n = E.reduce_rows(dt)
    rng = np.random.default_rng(7)
    a = rng.integers(-(1 << 20), 1 << 20, n).astype(np.float64) if dt == "f64" else rng.integers(-100, 101, n).astype(np.float32)
    assert np.abs(a.astype(np.float64)).sum() < (2 ** 53 if dt == "f64" else 2 ** 24)
    for valid in (None, E.every_third_null(n), E.walk_validity(n)):
        want = E.reduce_reference(a, valid)
        r = reductions(S(pl, "a", a, dt, valid))
        mean = want["sum"] / want["count"]
        assert r["sum"] == want["sum"] and r["mean"] == (mean if dt == "f64" else float(np.float32(mean))), (dt, r, want)
        assert r["min"] == want["min"] and r["max"] == want["max"] and r["count"] == want["count"], (dt, r, want)


@pytest.mark.parametrize("dt", E.DTYPES)
def test_validity_bits_at_every_position_of_a_word(pl, dt):
    """reduce_kernel's vector path reads valid[base >> 6] >> (base & 63) per lane: one valid row per 64-row word, at bit (7 w) % 64 of word w -- a shift that is off by
    any amount picks another row or none, and every value is distinct and positive.  Then whole words valid, alternating with whole words null."""
    n = E.reduce_rows(dt)
    a = E.walk_values(dt, n)
    for valid in (E.walk_validity(n), E.word_validity(n)):
        want = E.reduce_reference(a, valid)
        r = reductions(S(pl, "a", a, dt, valid))
        mean = float(want["mean"]) if not E.is_float(dt) else want["sum"] / want["count"]      # (the integer sums here stay far below 2^53: one rounding, in the division)
        if dt == "f32":      # the kernel sums f32 columns in f64 -- exact here -- and rounds the result to f32 once
            want["sum"] = float(np.float32(want["sum"]))
        for k in ("sum", "min", "max", "count"):
            assert r[k] == want[k], (dt, k, r, want)
        assert r["mean"] == (float(np.float32(mean)) if dt == "f32" else mean), (dt, r, want)


def test_integer_reductions_at_the_extremes(pl):
    """i64 / u64 columns holding their extremes, a u64 maximum above 2^63, i32 / u32 sums that wrap at the width the sum is returned in"""
    for dt in ("i64", "u64", "i32", "u32"):
        n = E.reduce_rows(dt)
        lo, hi = E.int_range(dt)
        a = np.zeros(n, dtype=E.NP[dt])
        a[::5], a[1::5], a[2::5] = hi, lo, hi - 3
        a[n - 1] = hi
        for valid in (None, E.every_third_null(n)):
            want = E.reduce_reference(a, valid)
            r = reductions(S(pl, "a", a, dt, valid))
            for k in ("sum", "min", "max", "count"):
                assert r[k] == want[k], (dt, k, r[k], want[k])
    a = np.full(E.reduce_rows("u64"), 5, dtype=np.uint64)
    a[77] = 2 ** 63 + 12345
    assert S(pl, "a", a, "u64").max() == 2 ** 63 + 12345 and S(pl, "a", a, "u64").min() == 5
    for dt, x in (("i32", 2 ** 31 - 1), ("u32", 2 ** 32 - 1), ("i32", -2 ** 31)):
        a = np.full(E.reduce_rows(dt), x, dtype=E.NP[dt])
        assert S(pl, "a", a, dt).sum() == E.wrap(x * len(a), dt) != x * len(a), dt


def test_mean_of_int64_values_near_2_pow_62(pl):
    """The mean of these is not exact -- the kernel adds (double)x per row -- so it is held to the exact mean (a Fraction) within the project's 1e-6 relative."""
    n = E.reduce_rows("i64")
    i = np.arange(n, dtype=np.int64)
    for sign in (1, -1):
        a = sign * ((1 << 62) - 1 - 3 * i)
        for valid in (None, E.every_third_null(n)):
            want = E.reduce_reference(a, valid)["mean"]
            got = S(pl, "a", a, "i64", valid).mean()
            print("mean i64 near 2^62:", sign, got, float(want), float(abs(Fraction(got) - want) / abs(want)))
            assert abs(Fraction(got) - want) <= Fraction(RTOL) * abs(want), (sign, got, float(want))


# ======================================================================================================== 3. Boolean columns
NULL_MODES = ["none", "left", "both"]


def bool_pair(pl, n, mode):
    (a, av), (b, bv) = E.bool_operands(n)
    if mode == "none":
        av, bv = np.ones(n, bool), np.ones(n, bool)
    elif mode == "left":
        bv = np.ones(n, bool)
    sa = S(pl, "a", a, "bool", None if av.all() else av)
    sb = S(pl, "b", b, "bool", None if bv.all() else bv)
    return (sa, a, av), (sb, b, bv)


@pytest.mark.parametrize("n", E.BOOL_LENGTHS)
def test_boolean_comparisons_and_logic_at_word_edges(pl, n):
    """ops::cmp on Boolean operands (six operators composed from bitmap_op, two of them in place on their own output), &, |, ^ (Kleene) and ~, against numpy on uint8"""
    for mode in NULL_MODES:
        (sa, a, av), (sb, b, bv) = bool_pair(pl, n, mode)
        for op in range(6):
            out = sa.cmp(op, sb)
            check(out, E.bool_cmp_reference(op, a, b), av & bv, ("cmp", op, n, mode))
            assert pad_bits_clear(pl, out), ("cmp", op, n, mode)
        for name, fn in (("and", lambda x, y: x & y), ("or", lambda x, y: x | y), ("xor", lambda x, y: x ^ y)):
            out = fn(sa, sb)
            want_v, want_ok = E.kleene(name, a, av, b, bv)
            check(out, want_v, want_ok, (name, n, mode))
            assert pad_bits_clear(pl, out), (name, n, mode)
        out = ~sa
        check(out, ~a, av, ("not", n, mode))
        assert pad_bits_clear(pl, out), ("not", n, mode)


def fill_null_bool(pl, s, v):
    out = pl.DataFrame([s.rename("x")]).lazy().with_columns(pl.col("x").fill_null(v).alias("y")).collect()
    return out["y"]


@pytest.mark.parametrize("n", E.BOOL_LENGTHS)
def test_boolean_fill_null_select_aggregates_cast_filter_gather(pl, n):
    """fill_null_bool_kernel, select_bool_kernel with column, literal and null-literal sides, bitmap_popcount behind sum / mean, and the results filtered and gathered"""
    F = pl._ffi
    mv, mm = E.third_bool(n)
    idx = np.arange(n, dtype=np.uint32)[::-1].copy()
    for mode in NULL_MODES:
        (sa, a, av), (sb, b, bv) = bool_pair(pl, n, mode)
        for v in (True, False):
            out = fill_null_bool(pl, sa, v)
            check(out, np.where(av, a, v), np.ones(n, bool), ("fill_null", v, n, mode))
            assert out.device_ptrs()[1] == 0 or out.null_count() == 0
            assert pad_bits_clear(pl, out), ("fill_null", v, n, mode)
        # sum / mean / count
        trues, cnt = int((a & av).sum()), int(av.sum())
        assert sa.sum() == trues and sa.count() == cnt and sa.mean() == (trues / cnt if cnt else None), (n, mode)
        # cast
        check(sa.cast(pl.Int8), a.astype(np.int8), av, ("i8", n, mode))
        check(sa.cast(pl.Float64), a.astype(np.float64), av, ("f64", n, mode))
        # when(mask).then(x).otherwise(y): columns, literals (length-1 columns) and a null literal
        t = mv & (mm if mode != "none" else True)
        mask = S(pl, "m", mv, "bool", mm if mode != "none" else None)
        lit = {"true": (S(pl, "l", np.array([True]), "bool"), np.ones(n, bool), np.ones(n, bool)),
               "false": (S(pl, "l", np.array([False]), "bool"), np.zeros(n, bool), np.ones(n, bool)),
               "null": (S(pl, "l", np.array([True]), "bool", np.zeros(1, bool)), np.ones(n, bool), np.zeros(n, bool))}
        sides = {"a": (sa, a, av), "b": (sb, b, bv), **lit}
        for x, y in (("a", "b"), ("a", "true"), ("false", "b"), ("true", "false"), ("a", "null"), ("null", "b"), ("null", "false")):
            (sx, xv, xm), (sy, yv, ym) = sides[x], sides[y]
            h = C.c_uint64()
            F.check(F.lib().plx_if_then_else(mask._h, sx._h, sy._h, C.byref(h)))
            out = pl.Series._from_handle("r", h.value, pl.Boolean)
            check(out, np.where(t, xv, yv), np.where(t, xm, ym), ("select", x, y, n, mode))
            assert pad_bits_clear(pl, out), ("select", x, y, n, mode)
        # filter and gather of a result
        eq = sa.eq(sb)
        want_v, want_ok = E.bool_cmp_reference(0, a, b), av & bv
        check(eq.filter(mask), want_v[t], want_ok[t], ("filter", n, mode))
        check(eq.gather(pl.Series("i", idx, dtype=pl.UInt32)), want_v[idx], want_ok[idx], ("gather", n, mode))


@pytest.mark.parametrize("n", [n for n in E.BOOL_LENGTHS if n % 64])
def test_pad_bits_do_not_leak_into_sums_or_concatenations(pl, n):
    """After ~x, fill_null(True) and x == y the bits beyond the last row are zero in the buffer, sum() counts the rows only, and the result concatenated in front of
    another chunk gives exactly its rows followed by the chunk's.  (popcount and the concatenation mask the tail of what they read, so it is the words read back that
    show a set pad bit.)  Found by this test: fill_null(True) on a Boolean column set every pad bit of the last word
    (fill_null_bool_kernel ors in ~validity without the tail mask every other word-wise kernel applies), e.g. n = 63, row 62 null -> bit 63 set."""
    (sa, a, av), (sb, b, bv) = bool_pair(pl, n, "both")
    tail_v, tail_m = E.third_bool(65)
    results = {"not": (~sa, ~a, av), "fill_null": (fill_null_bool(pl, sa, True), np.where(av, a, True), np.ones(n, bool)), "eq": (sa.eq(sb), E.bool_cmp_reference(0, a, b), av & bv),
               "not_plain": (~S(pl, "p", a, "bool"), ~a, np.ones(n, bool))}
    for name, (s, v, m) in results.items():
        assert pad_bits_clear(pl, s), (name, n, raw_words(pl, s, 0)[-1])
        assert s.sum() == int((v & m).sum()), (name, n)
        for tail_valid in (tail_m, None):
            out = pl.concat([pl.DataFrame([s.rename("x")]), pl.DataFrame([S(pl, "x", tail_v, "bool", tail_valid)])])["x"]
            check(out, np.concatenate([v, tail_v]), np.concatenate([m, tail_m if tail_valid is not None else np.ones(65, bool)]), (name, n, "concat"))
            assert pad_bits_clear(pl, out), (name, n, "concat")


# ========================================================================================================== 4. concatenation
def test_concat_at_every_bit_offset(pl):
    """ops::concat -> bitmap_blit_kernel: two atomicOr per word at an arbitrary bit offset, an all-ones stand-in for chunks without validity.  Twelve chunks whose running
    offset mod 64 is 0, 31, 32, 63, 0, 1, 32, 33, 41; three of them meet in output word 0; a zero-length chunk first and last."""
    chunks = [E.concat_chunk(k, n) for k, n in enumerate(E.CONCAT_LENGTHS)]
    dts = {"a": "i64", "u": "u8", "b": "bool"}
    frames = [pl.DataFrame([S(pl, name, v, dts[name], m) for name, (v, m) in ch.items()]) for ch in chunks]
    out = pl.concat(frames)
    assert out.height == sum(E.CONCAT_LENGTHS)
    for name in dts:
        want_v = np.concatenate([ch[name][0] for ch in chunks])
        want_ok = np.concatenate([np.ones(len(ch[name][0]), bool) if ch[name][1] is None else ch[name][1] for ch in chunks])
        check(out[name], want_v, want_ok, name)
        assert raw_pad_ok(pl, out[name]), name
    # chunks that all lack validity give a column without one
    plain = pl.concat([pl.DataFrame([S(pl, "b", ch["b"][0], "bool")]) for ch in chunks])["b"]
    check(plain, np.concatenate([ch["b"][0] for ch in chunks]), np.ones(out.height, bool), "plain")
    assert plain.device_ptrs()[1] == 0


def raw_pad_ok(pl, s):
    n = len(s)
    if n % 64 == 0 or not s.device_ptrs()[1]:
        return True
    return not (raw_words(pl, s, 1)[-1] & ~np.uint64((1 << (n % 64)) - 1))


# ================================================================================== 5. filter -> frame over many columns
def stamped_frame(pl, columns, n, nullable=()):
    host, cols = {}, []
    for c, dt in enumerate(columns):
        v = E.stamped(dt, c, n)
        m = ((np.arange(n) + c) % 5 != 0) if c in nullable else None
        host[f"c{c}"] = (v, m)
        cols.append(S(pl, f"c{c}", v, dt, m))
    return pl.DataFrame(cols), host


def check_filtered(out, host, keep, what):
    assert out.height == int(keep.sum()) and out.columns == list(host), what
    for name, (v, m) in host.items():
        check(out[name], v[keep], np.ones(int(keep.sum()), bool) if m is None else m[keep], (what, name))


@pytest.mark.parametrize("n", E.FILTER_LENGTHS)
def test_filter_to_frame_over_fifteen_columns(pl, n):
    """compact_by_ballots_kernel: 14 fixed-width columns (4 x 8 bytes, 4 x 4, 3 x 2, 3 x 1) in shuffled order are two launches of at most kCompactMaxCols (12) and
    groups of kCompactGroup (3) + 1 per width; a Boolean column and a nullable 8-byte column take the bitmap route beside them.  Every value names its row and its column."""
    df, host = stamped_frame(pl, E.DENSE_COLUMNS, n, nullable=(2,))
    key = host["c11"][0]
    last = int(key[n - 1])
    c = pl.col
    for what, pred, keep in (("only the last", c("c11") == last, key == last), ("all but the last", c("c11") != last, key != last),
                             ("every third", c("c11") % 3 == 2, key % 3 == 2)):
        out = df.lazy().filter(pred).collect()
        plan = pl.last_plan()
        assert "FusedFilter{" in plan, plan
        m = int(keep.sum())
        if 0 < m < n and m * 16 > n:
            assert "compaction of 14 columns in one pass (+2 bitmaps" in plan, plan
        check_filtered(out, host, keep, (n, what))


@pytest.mark.parametrize("n", E.FILTER_LENGTHS)
def test_sparse_filter_to_frame_over_nine_plain_columns(pl, n):
    """a selectivity under 1/16 over nine plain Int64 / Int32 columns: the kept row ids, then one gather_multi of kGatherMultiMax (8) columns and a single-column gather"""
    df, host = stamped_frame(pl, E.SPARSE_COLUMNS, n)
    key = host["c0"][0]
    last = int(key[n - 1])
    c = pl.col
    for what, pred, keep in (("only the last", c("c0") == last, key == last), ("all but the last", c("c0") != last, key != last),
                             ("one row in 17", c("c0") % 17 == 5, key % 17 == 5)):
        out = df.lazy().filter(pred).collect()
        plan = pl.last_plan()
        assert "FusedFilter{" in plan, plan
        m = int(keep.sum())
        if m < n and m * 16 <= n:
            assert "row ids -> gather x9" in plan, plan
        elif m < n:
            assert "compaction of 9 columns in one pass" in plan, plan
        check_filtered(out, host, keep, (n, what))
    if n >= 127:
        assert "row ids -> gather x9" in plan, plan      # the last predicate is sparse at every length from 127 on


# ============================================================================= 6. borrowed columns off a 16-byte boundary
class Window:
    """n rows of a library-owned buffer from row `skip` on, borrowed through Series.from_device: the column starts skip * itemsize bytes behind a 16-byte boundary"""

    def __init__(self, pl, dt, skip, n, valid=None, name="w", seed=0, values=None):
        self.dt, self.skip, self.n = dt, skip, n
        self.all = np.roll(E.window_values(dt, skip + n + 16), seed) if values is None else values(skip + n + 16).astype(E.NP[dt])
        self.base = S(pl, "base", self.all, dt)
        ptr = self.base.device_ptrs()[0]
        assert ptr % 16 == 0
        self.v = self.all[skip:skip + n]
        self.valid = valid
        self.bits = None
        vptr = 0
        if valid is not None:      # the window's own bits, uploaded on their own: whole 64-bit words at an 8-byte-aligned pointer
            words = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
            packed = np.packbits(valid, bitorder="little")
            words.view(np.uint8)[:len(packed)] = packed
            self.bits = pl.Series("bits", words, dtype=pl.UInt64)
            vptr = self.bits.device_ptrs()[0]
            assert vptr % 8 == 0
        itemsize = self.all.itemsize
        self.s = pl.Series.from_device(name, dtype_of(pl, dt), ptr + skip * itemsize, n, vptr, keepalive=(self.base, self.bits))
        assert skip * itemsize % 16 != 0 and self.s.device_ptrs()[0] % 16 == skip * itemsize % 16
        self.ok = np.ones(n, bool) if valid is None else valid

    def unchanged(self):
        return np.array_equal(self.base._download()[0], self.all)


def windows(dt):
    return [(skip, n) for skip in E.SKIPS[np.dtype(E.NP[dt]).itemsize] for n in E.borrowed_rows(dt)]


@pytest.mark.parametrize("dt", E.DTYPES)
def test_arithmetic_on_borrowed_columns_off_a_16_byte_boundary(pl, orc, dt):
    """arith_kernel loads 16 bytes per lane through load_pack; a borrowed Int64 column one row into a buffer is 8 bytes behind a 16-byte boundary.  All six operators,
    column-column with both sides borrowed and with one side owned, column-scalar in both orders; the reference is the oracle on the window's rows."""
    for skip, n in windows(dt):
        w, w2 = Window(pl, dt, skip, n), Window(pl, dt, skip, n, seed=5)
        owned = S(pl, "o", w2.v, dt)
        sc = w2.v[0].item()
        for op in range(6):
            ev, extra = orc.arith(op, w.v, w2.v)
            eok = np.ones(n, bool) if extra is None else extra
            check(w.s.arith(op, w2.s), ev, eok, (dt, skip, n, op, "both borrowed"))
            check(w.s.arith(op, owned), ev, eok, (dt, skip, n, op, "borrowed, owned"))
            ev, extra = orc.arith(op, w2.v, w.v)
            check(owned.arith(op, w.s), ev, np.ones(n, bool) if extra is None else extra, (dt, skip, n, op, "owned, borrowed"))
            ev, extra = orc.arith(op, w.v, sc, mode=1)
            check(w.s.arith(op, sc), ev, np.ones(n, bool) if extra is None else extra, (dt, skip, n, op, "column, scalar"))
            ev, extra = orc.arith(op, sc, w.v, mode=2)
            check(w.s.arith(op, sc, scalar_on_left=True), ev, np.ones(n, bool) if extra is None else extra, (dt, skip, n, op, "scalar, column"))
        assert w.unchanged() and w2.unchanged()


@pytest.mark.parametrize("dt", E.DTYPES)
def test_reductions_on_borrowed_columns_off_a_16_byte_boundary(pl, dt):
    """reduce_kernel and var_kernel (16-byte load_pack per lane), with and without a validity bitmap of the window's own"""
    for skip, n in windows(dt):
        for valid in (None, E.every_third_null(n)):
            if valid is not None and valid.all():
                continue
            w = Window(pl, dt, skip, n, valid)
            want = E.reduce_reference(w.v, valid)
            r = reductions(w.s)
            for k in ("sum", "min", "max", "count"):
                assert r[k] == want[k], (dt, skip, n, k, r, want)      # (float columns hold small integers: exact)
            mean = None if want["mean"] is None else (float(want["mean"]) if dt != "f32" else float(np.float32(float(want["mean"]))))
            assert r["mean"] == mean, (dt, skip, n, r, want)
            rows = w.v[w.ok].astype(np.float64)
            var = w.s.var()
            if len(rows) < 2:
                assert var is None
            else:
                # small integers: the sums of d and d * d are exact; what is left is a few hundred roundings of 2^-53 in the merges (f32: the result's own rounding)
                assert math.isclose(var, float(np.float32(rows.var(ddof=1))) if dt == "f32" else rows.var(ddof=1), rel_tol=1e-6 if dt == "f32" else 1e-12), (dt, skip, n, var)
            assert w.unchanged()


@pytest.mark.parametrize("dt", E.DTYPES)
def test_per_node_operators_on_borrowed_columns_off_a_16_byte_boundary(pl, dt):
    """cmp, cast, filter, gather, fill_null and arg_sort through the same windows, against numpy on v[skip : skip + n]"""
    for skip, n in windows(dt):
        valid = E.every_third_null(n) if n > 2 else None
        w, wv = Window(pl, dt, skip, n), Window(pl, dt, skip, n, valid)
        pivot = w.v[n // 2].item()
        owned = S(pl, "o", np.roll(w.v, 1), dt)
        for op, fn in E.BOOL_CMP.items():
            check(w.s.cmp(op, pivot), fn(w.v, w.v[n // 2]), np.ones(n, bool), (dt, skip, n, "cmp scalar", op))
            check(wv.s.cmp(op, owned), fn(w.v, np.roll(w.v, 1)), wv.ok, (dt, skip, n, "cmp column", op))
        for to in ("f64", "i8", "u64", "f32"):
            want_v, want_ok = E.cast_reference(w.v, to)
            check(wv.s.cast(dtype_of(pl, to)), want_v, want_ok & wv.ok, (dt, skip, n, "cast", to))
        mv, mm = E.third_bool(n)
        t = mv & mm
        check(wv.s.filter(S(pl, "m", mv, "bool", mm)), w.v[t], wv.ok[t], (dt, skip, n, "filter"))
        idx = np.arange(n, dtype=np.uint32)[::-1].copy()
        check(wv.s.gather(pl.Series("i", idx, dtype=pl.UInt32)), w.v[idx], wv.ok[idx], (dt, skip, n, "gather"))
        lit = 7.0 if E.is_float(dt) else 7
        filled = pl.DataFrame([wv.s]).lazy().with_columns(pl.col("w").fill_null(lit).alias("y")).collect()["y"]
        check(filled, np.where(wv.ok, w.v, E.NP[dt](7)), np.ones(n, bool), (dt, skip, n, "fill_null"))
        order = w.s.arg_sort().to_numpy()
        assert np.array_equal(order, np.argsort(w.v, kind="stable")), (dt, skip, n, "arg_sort")
        assert w.unchanged() and wv.unchanged()


def borrowed_frame(pl, n):
    ws = {"a": Window(pl, "i64", 1, n, name="a"), "x": Window(pl, "f64", 1, n, E.every_third_null(n), name="x", seed=3), "i": Window(pl, "i32", 3, n, name="i", seed=1),
          "k": Window(pl, "i32", 1, n, name="k", values=lambda m: np.arange(m) % 5)}
    return pl.DataFrame([w.s for w in ws.values()]), ws


def test_queries_over_a_frame_of_borrowed_columns(pl):
    """the fused scans' two-row loads (fused_device.hpp load2 / prefetch_inputs: 16 bytes for an 8-byte column) and compact_load_col<8> over borrowed Int64 / Float64 /
    Int32 columns that start 8, 8, 12 and 4 bytes behind a 16-byte boundary: a filter + aggregate and a filter + group_by in the generic interpreter, the run-time
    compiled kernel and per node, and a filter -> frame dense enough for the compaction kernel"""
    n = 2 * 64 * 16 + 5
    df, ws = borrowed_frame(pl, n)
    a, x, xm, i, k = ws["a"].v, ws["x"].v, ws["x"].ok, ws["i"].v, ws["k"].v
    c = pl.col
    keep = (i > 0) & (a < 90)
    key = k
    for mode in R.MODES:
        out = R.collect(pl, df.lazy().filter((c("i") > 0) & (c("a") < 90)).select(c("a").sum().alias("sa"), c("x").sum().alias("sx"), c("x").count().alias("cx"), c("i").min().alias("mi")), mode).to_dict()
        assert out["sa"][0] == int(a[keep].sum()) and out["sx"][0] == float(x[keep & xm].sum()) and out["cx"][0] == int((keep & xm).sum()) and out["mi"][0] == int(i[keep].min()), (mode, out)
        g = R.collect(pl, df.lazy().filter(c("i") > 0).group_by("k").agg(c("a").sum().alias("sa"), c("x").sum().alias("sx"), pl.len().alias("n")), mode).sort_host("k")
        gk = sorted(set(key[i > 0].tolist()))
        assert g["k"] == gk, (mode, g)
        for j, kv in enumerate(gk):
            m = (i > 0) & (key == kv)
            assert g["sa"][j] == int(a[m].sum()) and g["sx"][j] == float(x[m & xm].sum()) and g["n"][j] == int(m.sum()), (mode, kv)
    out = df.lazy().filter(c("i") > 0).collect()
    plan = pl.last_plan()
    assert "FusedFilter{" in plan and "compaction of 4 columns" in plan, plan
    keep = i > 0
    check_filtered(out, {name: (w.v, w.valid) for name, w in ws.items()}, keep, "borrowed frame")
    assert all(w.unchanged() for w in ws.values())


def test_borrowed_pointers_below_the_documented_alignment_are_refused(pl):
    """plx_column_from_device: the values pointer is a multiple of the element width and the validity pointer a multiple of 8 (every kernel loads validity as uint64_t);
    anything else is PLX_ERR_INVALID before a kernel sees it"""
    base = pl.Series("base", np.arange(64, dtype=np.int64))
    bits = pl.Series("bits", np.full(4, 2 ** 64 - 1, dtype=np.uint64))
    ptr, vptr = base.device_ptrs()[0], bits.device_ptrs()[0]
    with pytest.raises(pl.PlxError) as e:
        pl.Series.from_device("v", pl.Int64, ptr + 4, 8, keepalive=base)
    assert e.value.code == 1 and "multiple of 8" in str(e.value)
    with pytest.raises(pl.PlxError) as e:
        pl.Series.from_device("v", pl.Int64, ptr + 8, 8, vptr + 4, keepalive=(base, bits))
    assert e.value.code == 1 and "validity" in str(e.value)
    with pytest.raises(pl.PlxError):
        pl.Series.from_device("v", pl.Int16, ptr + 1, 8, keepalive=base)
    ok = pl.Series.from_device("v", pl.Int64, ptr + 8, 8, vptr + 8, keepalive=(base, bits))      # 8 bytes off a 16-byte boundary on both: accepted
    assert ok.to_list() == list(range(1, 9)) and ok.null_count() == 0
