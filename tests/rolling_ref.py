"""numpy reference of shift / diff and rolling_sum / rolling_mean / rolling_min / rolling_max, plain and over partitions (TEST INFRASTRUCTURE).

Everything is a plain loop over the rows of a partition in row order (tests/cumulative_ref.py gives the partitions: a null key part is a value of its own,
NaN == NaN, -0 == +0).

shift(n, fill_value): row i of a partition takes its row i - n; where that row does not exist the result is null, or fill_value and valid.  The moved rows keep
their validity.  diff(n): x[i] - x[i - n] in the result dtype (UInt8 -> Int16, UInt16 -> Int32, UInt32 / UInt64 -> Int64, else unchanged; integers wrap), null where
either row is null or row i - n does not exist.

rolling_*(w, min_samples, center): the window of row i is the rows [i + h - w + 1, i + h] of its partition, h = 0 or (w - 1) // 2, clipped to the partition; null
where it holds fewer than min_samples non-null values, else the function of its non-null values.  rolling_sum: the cum_sum dtype (integers wrap; floats summed in
float64); rolling_mean: float64 sum / count (the result dtype is Float64, Float32 for a Float32 operand); rolling_min / rolling_max: np.fmin / np.fmax over the
valid values (a NaN is ignored unless every valid value is NaN).

self_check() runs hand-written vectors."""
import numpy as np

from tests import agg_edges as AE
from tests import cumulative_ref as CR

RTOL = AE.RTOL
OPS = ("rolling_sum", "rolling_mean", "rolling_min", "rolling_max")
DIFF_DTYPE = {np.dtype(np.uint8): np.int16, np.dtype(np.uint16): np.int32, np.dtype(np.uint32): np.int64, np.dtype(np.uint64): np.int64}


def result_dtype(op, dtype):
    dtype = np.dtype(dtype)
    if op == "rolling_sum":
        return CR.result_dtype("cum_sum", dtype)
    if op == "rolling_mean":
        return np.dtype(np.float32) if dtype == np.float32 else np.dtype(np.float64)
    if op == "diff":
        return np.dtype(DIFF_DTYPE.get(dtype, dtype))
    return dtype                                              # rolling_min / rolling_max / shift


def shift(x, valid=None, n=1, fill_value=None, keys=None):
    """-> (values, valid mask)"""
    x = np.asarray(x)
    rows = len(x)
    ok = np.ones(rows, bool) if valid is None else np.asarray(valid, bool)
    out = np.zeros(rows, x.dtype)
    out_ok = np.zeros(rows, bool)
    for p in CR.partitions(keys, rows):
        for j in range(len(p)):
            s = j - n
            if 0 <= s < len(p):
                out[p[j]], out_ok[p[j]] = x[p[s]], ok[p[s]]
            elif fill_value is not None:
                out[p[j]], out_ok[p[j]] = fill_value, True
    return out, out_ok


def diff(x, valid=None, n=1, keys=None):
    """-> (values in the result dtype, valid mask)"""
    x = np.asarray(x)
    rows = len(x)
    ok = np.ones(rows, bool) if valid is None else np.asarray(valid, bool)
    out_dt = result_dtype("diff", x.dtype)
    wide = x.astype(out_dt)                                   # (UInt64 -> Int64 wraps, as the device's conversion does)
    out = np.zeros(rows, out_dt)
    out_ok = np.zeros(rows, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in CR.partitions(keys, rows):
            for j in range(len(p)):
                s = j - n
                if 0 <= s < len(p) and ok[p[j]] and ok[p[s]]:
                    out[p[j]] = wide[p[j]] - wide[p[s]]       # numpy scalars of one dtype: integers wrap
                    out_ok[p[j]] = True
    return out, out_ok


_windows = {}


def _rolling_windows(op, x, ok, w, center, keys, ok_id):
    """every row's window with at least one valid value: (values, the window's sum of |x| or None, the window's count of valid values).  The last few results are
    remembered (the arrays are held, so their ids stay theirs): the checks of one frame differ in min_samples and in the route only"""
    memo_key = (op, id(x), ok_id, w, center) + tuple((id(v), id(m)) for v, m in (keys or []))
    if memo_key in _windows:
        return _windows[memo_key][0]
    rows = len(x)
    h = (w - 1) // 2 if center else 0
    isf = x.dtype.kind == "f"
    floaty = op == "rolling_mean" or (op == "rolling_sum" and isf)
    out_dt = np.dtype(np.float64) if floaty else result_dtype(op, x.dtype)
    out = np.zeros(rows, out_dt)
    scale = np.zeros(rows, np.float64) if floaty else None
    count = np.zeros(rows, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in CR.partitions(keys, rows):
            xv, okv = x[p], ok[p]
            for j in range(len(p)):
                lo, hi = max(j + h - w + 1, 0), min(j + h, len(p) - 1)
                v = xv[lo:hi + 1][okv[lo:hi + 1]]
                count[p[j]] = len(v)
                if not len(v):
                    continue
                if op in ("rolling_sum", "rolling_mean"):
                    if floaty:
                        v64 = v.astype(np.float64)
                        total = v64.sum()
                        out[p[j]] = total / len(v) if op == "rolling_mean" else total
                        scale[p[j]] = np.where(np.isfinite(v64), np.abs(v64), 0.0).sum()
                    else:
                        out[p[j]] = v.astype(out_dt).sum(dtype=out_dt)
                elif isf:
                    out[p[j]] = (np.fmin if op == "rolling_min" else np.fmax).reduce(v)
                else:
                    out[p[j]] = v.min() if op == "rolling_min" else v.max()
    if len(_windows) >= 64:
        _windows.clear()
    _windows[memo_key] = ((out, scale, count), (x, ok, keys))
    return out, scale, count


def rolling(op, x, valid=None, w=1, min_samples=None, center=False, keys=None):
    """-> (values: float64 for a float rolling_sum and for rolling_mean, else the result dtype; valid mask; the window's sum of |x| for those float results, else
    None; the window's count of valid values).  Pass the same array objects again and the windows are not walked again."""
    x = x if isinstance(x, np.ndarray) else np.asarray(x)
    m = w if min_samples is None else min_samples
    ok = np.ones(len(x), bool) if valid is None else (valid if isinstance(valid, np.ndarray) and valid.dtype == bool else np.asarray(valid, bool))
    out, scale, count = _rolling_windows(op, x, ok, w, center, keys, 0 if valid is None else id(ok))
    return out, count >= m, scale, count


def _same(g, w):
    if g.dtype.kind == "f":
        return (g == w) | (np.isnan(g) & np.isnan(w))
    return g == w


def check_shift(got, got_valid, x, valid=None, n=1, fill_value=None, keys=None, what=""):
    """shift is a copy: values exact (NaN for NaN, bit patterns of everything else through ==), validity bit for bit, the dtype the operand's"""
    x = np.asarray(x)
    want, want_ok = shift(x, valid, n, fill_value, keys)
    got = np.asarray(got)
    assert got.dtype == x.dtype and len(got) == len(want), (what, got.dtype, x.dtype, len(got), len(want))
    gv = np.ones(len(got), bool) if got_valid is None else np.asarray(got_valid, bool)
    assert np.array_equal(gv, want_ok), (what, "validity", np.flatnonzero(gv != want_ok)[:8])
    bad = ~_same(got[want_ok], want[want_ok])
    assert not bad.any(), (what, "rows", np.flatnonzero(want_ok)[bad][:8], got[want_ok][bad][:8], want[want_ok][bad][:8])


def check_diff(got, got_valid, x, valid=None, n=1, keys=None, what=""):
    """diff is one subtraction: exact for integers (wrapping) and for floats (one IEEE operation); validity bit for bit; the widened dtype"""
    x = np.asarray(x)
    want, want_ok = diff(x, valid, n, keys)
    got = np.asarray(got)
    assert got.dtype == want.dtype and len(got) == len(want), (what, got.dtype, want.dtype, len(got), len(want))
    gv = np.ones(len(got), bool) if got_valid is None else np.asarray(got_valid, bool)
    assert np.array_equal(gv, want_ok), (what, "validity", np.flatnonzero(gv != want_ok)[:8])
    bad = ~_same(got[want_ok], want[want_ok])
    assert not bad.any(), (what, "rows", np.flatnonzero(want_ok)[bad][:8], got[want_ok][bad][:8], want[want_ok][bad][:8])


def check_rolling(got, got_valid, op, x, valid=None, w=1, min_samples=None, center=False, keys=None, what=""):
    """One result column against the reference, every row in row order.  The result dtype; validity bit for bit; integer results and rolling_min / rolling_max
    exact (NaN for NaN; the sign of a zero is not compared); a float rolling_sum within RTOL * sum over the window of |x_j| of the float64 reference, rolling_mean
    within that bound divided by the count (a non-finite expectation matched in kind), plus one f32 ulp of the reference for a Float32 result -- the bound
    tests/cumulative_ref.py gives cum_sum: the scans add in another association than the loop, nothing more."""
    x = np.asarray(x)
    want, want_ok, scale, count = rolling(op, x, valid, w, min_samples, center, keys)
    got = np.asarray(got)
    assert len(got) == len(want), (what, len(got), len(want))
    assert got.dtype == result_dtype(op, x.dtype), (what, "dtype", got.dtype, result_dtype(op, x.dtype))
    gv = np.ones(len(got), bool) if got_valid is None else np.asarray(got_valid, bool)
    assert np.array_equal(gv, want_ok), (what, op, "validity", np.flatnonzero(gv != want_ok)[:8])
    sel = want_ok
    g, wv = got[sel], want[sel]
    if scale is None:
        bad = ~_same(g, wv)
        assert not bad.any(), (what, op, "rows", np.flatnonzero(sel)[bad][:8], g[bad][:8], wv[bad][:8])
        return
    g = g.astype(np.float64)
    fin = np.isfinite(wv)
    kind_ok = np.where(np.isnan(wv), np.isnan(g), g == wv)
    bound = RTOL * scale[sel]
    if op == "rolling_mean":
        bound = bound / np.maximum(count[sel], 1)
    if got.dtype == np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            bound = bound + np.where(fin, np.spacing(np.abs(wv).astype(np.float32)).astype(np.float64), 0.0)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(g) & (np.abs(g - wv) <= bound)
    bad = np.where(fin, ~close, ~kind_ok)
    assert not bad.any(), (what, op, "rows", np.flatnonzero(sel)[bad][:8], g[bad][:8], wv[bad][:8], bound[bad][:8])


def self_check():
    """hand-written vectors; -> how many were checked"""
    n = 0
    nan, inf = np.nan, np.inf

    def eq(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))
    x = np.array([1, 2, 3, 4, 5], np.int64)
    v, ok = shift(x, None, 2)
    assert ok.tolist() == [False, False, True, True, True] and eq(v[ok], [1, 2, 3]); n += 1
    v, ok = shift(x, None, -1, fill_value=9)
    assert ok.all() and eq(v, [2, 3, 4, 5, 9]); n += 1
    v, ok = shift(x, np.array([1, 0, 1, 1, 1], bool), 1)
    assert ok.tolist() == [False, True, False, True, True]; n += 1                                        # the moved rows keep their validity
    v, ok = shift(x, None, 7)
    assert not ok.any(); n += 1
    v, ok = shift(x, None, 1, None, [(np.array([7, 8, 7, 8, 7]), None)])
    assert ok.tolist() == [False, False, True, True, True] and eq(v[ok], [1, 2, 3]); n += 1
    v, ok = diff(np.array([5, 3, 10], np.uint8))
    assert v.dtype == np.int16 and ok.tolist() == [False, True, True] and eq(v[ok], [-2, 7]); n += 1
    v, ok = diff(np.array([0, 2 ** 64 - 1], np.uint64))
    assert v.dtype == np.int64 and eq(v[ok], [-1]); n += 1
    v, ok = diff(np.array([-2 ** 63, 2 ** 63 - 1], np.int64))
    assert eq(v[ok], [-1]); n += 1                                                                        # wraps
    v, ok = diff(np.array([1.0, nan, 4.0, 6.5]), np.array([1, 1, 0, 1], bool), 1)
    assert ok.tolist() == [False, True, False, False] and v[1] != v[1]; n += 1
    v, ok = diff(np.array([1, 5, 2, 9], np.int32), None, -1, [(np.array([0, 1, 0, 1]), None)])
    assert ok.tolist() == [True, True, False, False] and eq(v[ok], [-1, -4]); n += 1
    v, ok, _, _ = rolling("rolling_sum", x, None, 3)
    assert ok.tolist() == [False, False, True, True, True] and eq(v[ok], [6, 9, 12]); n += 1
    v, ok, _, _ = rolling("rolling_sum", x, None, 3, 1)
    assert ok.all() and eq(v, [1, 3, 6, 9, 12]); n += 1
    v, ok, _, _ = rolling("rolling_sum", x, None, 3, 2, True)
    assert ok.all() and eq(v, [3, 6, 9, 12, 9]); n += 1                                                    # centered: [i - 1, i + 1]
    v, ok, _, _ = rolling("rolling_sum", x, None, 4, 1, True)
    assert eq(v, [3, 6, 10, 14, 12]); n += 1                                                              # even window centered: h = 1, [i - 2, i + 1]
    v, ok, _, c = rolling("rolling_sum", x, np.array([1, 0, 0, 1, 1], bool), 2, 1)
    assert ok.tolist() == [True, True, False, True, True] and eq(v[ok], [1, 1, 4, 9]) and c.tolist() == [1, 1, 0, 1, 2]; n += 1
    v, ok, s, _ = rolling("rolling_sum", np.array([1.0, inf, 2.0, 3.0, 4.0]), None, 2)
    assert eq(v[ok], [inf, inf, 5.0, 7.0]) and eq(s[ok], [1.0, 2.0, 5.0, 7.0]); n += 1                     # the infinity leaves the window: finite again
    v, ok, _, _ = rolling("rolling_mean", np.array([2, 4, 9], np.int8), None, 2)
    assert v.dtype == np.float64 and eq(v[ok], [3.0, 6.5]); n += 1
    v, ok, _, _ = rolling("rolling_min", np.array([nan, 3.0, nan, 1.0]), None, 2, 1)
    assert eq(v, [nan, 3.0, 3.0, 1.0]); n += 1
    v, ok, _, _ = rolling("rolling_max", np.array([3, 1, 4, 1, 5], np.uint8), None, 3, 1, False, [(np.array([0, 0, 1, 1, 0]), None)])
    assert v.dtype == np.uint8 and eq(v, [3, 3, 4, 4, 5]); n += 1
    v, ok, _, _ = rolling("rolling_sum", np.array([127, 127, 2 ** 31 - 1], np.int32), None, 2)
    assert v.dtype == np.int32 and eq(v[ok], [254, -2 ** 31 + 126]); n += 1                                # wraps in Int32
    v, ok, _, _ = rolling("rolling_sum", np.array([True, True, False]), None, 2)
    assert v.dtype == np.uint32 and eq(v[ok], [2, 1]); n += 1
    v, ok, _, _ = rolling("rolling_sum", x, None, 9, 1)
    assert eq(v, [1, 3, 6, 10, 15]); n += 1                                                               # a window larger than the column
    return n
