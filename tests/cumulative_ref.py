"""numpy reference of cum_sum / cum_min / cum_max / cum_count and rank, plain and over partitions (TEST INFRASTRUCTURE).

Cumulative functions: per-partition loops over np.cumsum / np.fmin.accumulate / np.minimum.accumulate on the partition's valid rows in row order (reverse=True: the
rows walked from the partition's last to its first).  A null row stays null and contributes nothing.  Result dtypes: cum_sum Int8 / Int16 / UInt8 / UInt16 -> Int64,
Boolean -> UInt32, every other dtype its own (integer sums wrap as np.cumsum in that dtype does); cum_min / cum_max keep the dtype; cum_count UInt32, never null.
Float sums are computed in float64 whatever the operand (Float32 results are compared against that, see check()).

Rank: written from the definitions -- a stable sort of the partition's valid rows by the sort's order (NaN greatest, all NaNs tie, -0 == +0; descending flips the
values, never the tie order), then counting: ordinal = position + 1, min / max = the first / last position of the run of equal values + 1, average their mean, dense
= the number of distinct values up to and including the row's.

Partitions are those of a window: a null key part is a value of its own, NaN == NaN, -0 == +0.  self_check() runs hand-written vectors."""
import numpy as np

from tests import agg_edges as AE

RTOL = AE.RTOL
OPS = ("cum_sum", "cum_min", "cum_max", "cum_count")
METHODS = ("average", "min", "max", "dense", "ordinal")
SUM_DTYPE = {np.dtype(np.int8): np.int64, np.dtype(np.int16): np.int64, np.dtype(np.uint8): np.int64, np.dtype(np.uint16): np.int64, np.dtype(np.bool_): np.uint32}


_memo = {}


def _codes(values, valid):
    """dense codes of one key column by the window's equality; a null is code 0"""
    v = np.asarray(values)
    if v.dtype.kind == "f":
        v = v + 0.0                                   # -0 -> +0 (np.unique already holds every NaN equal)
    _, inv = np.unique(v, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int64) + 1
    if valid is not None:
        inv = np.where(np.asarray(valid, bool), inv, 0)
    return inv


def partition_index(keys, n):
    """the partitions of `keys` ([(values, valid or None)], or None / []: one partition) as (order, bounds): partition g is the rows order[bounds[g]:bounds[g + 1]],
    in row order"""
    if not keys:
        return np.arange(n), np.array([0, n] if n else [0])
    memo_key = (n,) + tuple((id(v), id(m)) for v, m in keys)          # the last key list is remembered: the checks of one frame's columns share their partitions
    if _memo.get("key") == memo_key:
        return _memo["value"]
    _memo["key"], _memo["hold"] = None, keys                          # (the arrays are held, so their ids stay theirs)
    joint = np.zeros(n, np.int64)
    for values, valid in keys:
        c = _codes(values, valid)
        _, joint = np.unique(joint * (int(c.max(initial=0)) + 1) + c, return_inverse=True)
        joint = joint.reshape(-1).astype(np.int64)
    order = np.argsort(joint, kind="stable")
    _memo["value"] = (order, np.r_[0, np.flatnonzero(np.diff(joint[order])) + 1, n])
    _memo["key"] = memo_key
    return _memo["value"]


def partitions(keys, n):
    """the same as a list of row-index arrays"""
    order, bounds = partition_index(keys, n)
    return [order[a:b] for a, b in zip(bounds[:-1].tolist(), bounds[1:].tolist())]


def result_dtype(op, dtype):
    dtype = np.dtype(dtype)
    if op == "cum_count":
        return np.dtype(np.uint32)
    if op == "cum_sum":
        return np.dtype(SUM_DTYPE.get(dtype, dtype))
    return dtype


def cum(op, x, valid=None, keys=None, reverse=False):
    """-> (values in the result dtype, float64 for a float cum_sum; valid mask, None for cum_count; for a float cum_sum also the running sum of |x|, else None)"""
    x = np.asarray(x)
    n = len(x)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    isf = x.dtype.kind == "f"
    out_dt = np.dtype(np.float64) if (isf and op == "cum_sum") else result_dtype(op, x.dtype)
    out = np.zeros(n, out_dt)
    scale = np.zeros(n, np.float64) if (isf and op == "cum_sum") else None
    order, bounds = partition_index(keys, n)
    lens = np.diff(bounds)
    s = order[bounds[:-1][lens == 1]]
    parts = [order[a:b] for a, b in zip(bounds[:-1][lens > 1].tolist(), bounds[1:][lens > 1].tolist())]
    if len(s):                                        # a partition of one row is the row itself (no loop over millions of them)
        if op == "cum_count":
            out[s] = ok[s]
        else:
            out[s] = x[s].astype(out_dt)
            if scale is not None:
                scale[s] = np.where(np.isfinite(x[s]), np.abs(x[s].astype(np.float64)), 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in parts:
            if reverse:
                p = p[::-1]
            if op == "cum_count":
                out[p] = np.cumsum(ok[p], dtype=np.uint32)
                continue
            rows = p[ok[p]]
            if not len(rows):
                continue
            v = x[rows]
            if op == "cum_sum":
                out[rows] = np.cumsum(v.astype(out_dt), dtype=out_dt)
                if scale is not None:
                    scale[rows] = np.cumsum(np.where(np.isfinite(v), np.abs(v.astype(np.float64)), 0.0))
            elif isf:
                out[rows] = (np.fmin if op == "cum_min" else np.fmax).accumulate(v)
            else:
                out[rows] = (np.minimum if op == "cum_min" else np.maximum).accumulate(v)
    return out, (None if op == "cum_count" else ok), scale


def rank(x, valid=None, method="average", descending=False, keys=None):
    """-> (Float64 for "average", UInt32 otherwise; valid mask)"""
    x = np.asarray(x)
    n = len(x)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    out = np.zeros(n, np.float64 if method == "average" else np.uint32)
    for p in partitions(keys, n):
        rows = p[ok[p]]
        if not len(rows):
            continue
        v = x[rows]
        if v.dtype.kind == "f":
            v = v + 0.0
        u, code = np.unique(v, return_inverse=True)                  # ascending, NaN greatest and all alike
        code = code.reshape(-1).astype(np.int64)
        if descending:
            code = len(u) - 1 - code
        order = np.argsort(code, kind="stable")                      # ties keep row order, descending or not
        sc = code[order]
        pos = np.arange(len(rows))
        head = np.r_[True, sc[1:] != sc[:-1]]
        first = np.maximum.accumulate(np.where(head, pos, 0))        # first position of the run
        tail = np.r_[head[1:], True]
        last = np.minimum.accumulate(np.where(tail, pos, len(rows))[::-1])[::-1]
        r = {"ordinal": pos + 1, "min": first + 1, "max": last + 1, "average": (first + 1 + last + 1) / 2.0, "dense": np.cumsum(head)}[method]
        out[rows[order]] = r
    return out, ok


def check_cum(got, got_valid, op, x, valid=None, keys=None, reverse=False, what=""):
    """One result column (values, valid mask or None) against the reference, every row in row order.  Validity bit for bit; integer results, cum_count and
    cum_min / cum_max (as numbers, NaN for NaN; the sign of a zero is not compared) exact; a float cum_sum at row i within RTOL * sum_{j<=i} |x_j| of the float64
    reference (a non-finite expectation matched in kind), plus one f32 ulp of the reference for a Float32 result -- the bound tests/agg_edges.py compare() gives
    the sum aggregate."""
    x = np.asarray(x)
    want, want_valid, scale = cum(op, x, valid, keys, reverse)
    got = np.asarray(got)
    assert len(got) == len(want), (what, len(got), len(want))
    assert got.dtype == result_dtype(op, x.dtype), (what, "dtype", got.dtype, result_dtype(op, x.dtype))
    if want_valid is None:
        assert got_valid is None or np.asarray(got_valid).all(), (what, "cum_count holds a null")
        sel = np.ones(len(want), bool)
    else:
        gv = np.ones(len(got), bool) if got_valid is None else np.asarray(got_valid, bool)
        assert np.array_equal(gv, want_valid), (what, "validity", np.flatnonzero(gv != want_valid)[:8])
        sel = want_valid
    g, w = got[sel], want[sel]
    if scale is None:
        if g.dtype.kind == "f":
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
        else:
            bad = g != w
        assert not bad.any(), (what, op, "rows", np.flatnonzero(sel)[bad][:8], g[bad][:8], w[bad][:8])
        return
    g = g.astype(np.float64)
    fin = np.isfinite(w)
    kind_ok = np.where(np.isnan(w), np.isnan(g), g == w)
    bound = RTOL * scale[sel]
    if got.dtype == np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            bound = bound + np.where(fin, np.spacing(np.abs(w).astype(np.float32)).astype(np.float64), 0.0)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(g) & (np.abs(g - w) <= bound)
    bad = np.where(fin, ~close, ~kind_ok)
    assert not bad.any(), (what, op, "rows", np.flatnonzero(sel)[bad][:8], g[bad][:8], w[bad][:8], bound[bad][:8])


def check_rank(got, got_valid, x, valid=None, method="average", descending=False, keys=None, what=""):
    """ranks are exact; validity bit for bit; "average" is Float64, the other methods UInt32"""
    want, want_valid = rank(x, valid, method, descending, keys)
    got = np.asarray(got)
    assert got.dtype == want.dtype and len(got) == len(want), (what, got.dtype, want.dtype, len(got), len(want))
    gv = np.ones(len(got), bool) if got_valid is None else np.asarray(got_valid, bool)
    assert np.array_equal(gv, want_valid), (what, "validity", np.flatnonzero(gv != want_valid)[:8])
    bad = got[want_valid] != want[want_valid]
    assert not bad.any(), (what, method, "rows", np.flatnonzero(want_valid)[bad][:8], got[want_valid][bad][:8], want[want_valid][bad][:8])


def self_check():
    """hand-written vectors; -> how many were checked"""
    n = 0
    nan, inf = np.nan, np.inf

    def eq(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))
    v, ok, _ = cum("cum_sum", np.array([1, 2, 3, 4], np.int64), np.array([1, 0, 1, 1], bool))
    assert eq(v[ok], [1, 4, 8]) and ok.tolist() == [True, False, True, True]; n += 1
    v, _, _ = cum("cum_sum", np.array([100, 100, 100], np.int8))
    assert v.dtype == np.int64 and eq(v, [100, 200, 300]); n += 1
    v, _, _ = cum("cum_sum", np.array([2 ** 31 - 1, 1, 1], np.int32))
    assert v.dtype == np.int32 and eq(v, [2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1]); n += 1                     # wraps
    v, _, _ = cum("cum_sum", np.array([True, False, True]))
    assert v.dtype == np.uint32 and eq(v, [1, 1, 2]); n += 1
    v, _, _ = cum("cum_sum", np.array([1.0, inf, -inf, 1.0]))
    assert eq(v, [1.0, inf, nan, nan]); n += 1                                                              # +inf then -inf: NaN from there on
    v, _, _ = cum("cum_sum", np.array([1, 2, 3, 4, 5], np.int64), None, [(np.array([7, 8, 7, 8, 7]), None)])
    assert eq(v, [1, 2, 4, 6, 9]); n += 1
    v, _, _ = cum("cum_sum", np.array([1, 2, 3, 4, 5], np.int64), None, [(np.array([7, 8, 7, 8, 7]), None)], reverse=True)
    assert eq(v, [9, 6, 8, 4, 5]); n += 1
    v, _, _ = cum("cum_min", np.array([nan, 3.0, nan, 1.0, 2.0]))
    assert eq(v, [nan, 3.0, 3.0, 1.0, 1.0]); n += 1                                                         # NaN ignored unless nothing else came yet
    v, _, _ = cum("cum_max", np.array([3, 1, 4, 1, 5], np.uint8), None, None, reverse=True)
    assert v.dtype == np.uint8 and eq(v, [5, 5, 5, 5, 5]); n += 1
    v, ok, _ = cum("cum_count", np.array([9, 9, 9, 9]), np.array([0, 1, 0, 1], bool))
    assert ok is None and v.dtype == np.uint32 and eq(v, [0, 1, 1, 2]); n += 1
    # a null key part is a partition of its own; NaN keys are one partition; -0 == +0
    v, _, _ = cum("cum_count", np.ones(6), None, [(np.array([nan, 0.0, nan, -0.0, 1.0, 1.0]), np.array([1, 1, 1, 1, 1, 0], bool))])
    assert eq(v, [1, 1, 2, 2, 1, 1]); n += 1
    x = np.array([10.0, 20.0, 10.0, nan, 20.0, nan, -0.0, 0.0])
    for method, asc, desc in (("ordinal", [3, 5, 4, 7, 6, 8, 1, 2], [5, 3, 6, 1, 4, 2, 7, 8]), ("min", [3, 5, 3, 7, 5, 7, 1, 1], [5, 3, 5, 1, 3, 1, 7, 7]),
                              ("max", [4, 6, 4, 8, 6, 8, 2, 2], [6, 4, 6, 2, 4, 2, 8, 8]), ("dense", [2, 3, 2, 4, 3, 4, 1, 1], [3, 2, 3, 1, 2, 1, 4, 4]),
                              ("average", [3.5, 5.5, 3.5, 7.5, 5.5, 7.5, 1.5, 1.5], [5.5, 3.5, 5.5, 1.5, 3.5, 1.5, 7.5, 7.5])):
        r, _ = rank(x, None, method)
        assert eq(r, asc), (method, r); n += 1
        r, _ = rank(x, None, method, descending=True)
        assert eq(r, desc), (method, r); n += 1
    r, ok = rank(np.array([5, 1, 5, 3], np.int32), np.array([1, 1, 0, 1], bool), "min", keys=[(np.array([0, 0, 0, 1]), None)])
    assert ok.tolist() == [True, True, False, True] and eq(r[ok], [2, 1, 1]); n += 1
    return n
