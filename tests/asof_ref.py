"""The join_asof contract as a plain per-row loop (test infrastructure; numpy and the standard library only).

join_asof(...) returns (idx, matched): for every left row the matched right row (0 where there is none) and whether there is one.  The contract is the one stated
at plx_join_asof_indices in include/polars_amd.h:
  * the candidates of a left row are the right rows whose by parts all equal its own (NaN == NaN, -0 == +0), in (on, right row) order; a null in any by part or a
    null `on`, on either side, makes the row match nothing;
  * backward: the last candidate with on_r <= on_l; forward: the first with on_r >= on_l; nearest: the smallest distance, among several at that distance the LAST in
    candidate order; strict makes every comparison strict;
  * a tolerance keeps the match found without it only if its distance is at most the tolerance (no fallback); integer distances are exact, float distances are
    |a - b| in f64 with equal values at distance 0, a NaN distance is within no tolerance and loses against any number.
`match_row` is the literal loop over the candidates.  join_asof walks each group's candidates the same way, but finds where to look with numpy's searchsorted on
the ranks of the `on` values, so that the larger test shapes stay quick; self_check() holds the two against each other on random inputs, besides the hand-written
vectors.  nearest_tie="backward" exists only for the cross-check against pandas.merge_asof, which sends a tie to the backward candidate and takes the first row of
a duplicated forward value.
"""
from __future__ import annotations

import math

import numpy as np

STRATEGIES = ("backward", "forward", "nearest")


def key_of(v):
    """a value as a key of the sort's total order: NaN greatest and equal to itself, -0 == +0; exact for every integer"""
    if isinstance(v, (float, np.floating)):
        f = float(v)
        return (1, 0.0) if math.isnan(f) else (0, f + 0.0)
    if isinstance(v, (bool, np.bool_)):
        return (0, int(v))
    return (0, int(v))


def distance(a, b):
    """of two raw values: exact for integers; floats: 0.0 for equal keys, else |a - b| in f64 (may be NaN or inf)"""
    if isinstance(a, (float, np.floating)) or isinstance(b, (float, np.floating)):
        return 0.0 if key_of(a) == key_of(b) else abs(float(a) - float(b))
    return abs(int(a) - int(b))


def closer_or_equal(d_new, d_best):
    """d_new <= d_best where a NaN distance loses against any number (two NaN distances are equal)"""
    nan_new, nan_best = isinstance(d_new, float) and math.isnan(d_new), isinstance(d_best, float) and math.isnan(d_best)
    if nan_new or nan_best:
        return nan_best
    return d_new <= d_best


def within(d, tolerance):
    if tolerance is None:
        return True
    return not (isinstance(d, float) and math.isnan(d)) and d <= tolerance


def match_row(on_l, cands, strategy, strict=False, tolerance=None, nearest_tie="forward"):
    """cands: [(on_r, right row)] in candidate order.  The matched right row or None: the literal loop."""
    kl = key_of(on_l)
    best = None
    if strategy == "backward":
        for v, j in cands:
            if key_of(v) < kl or (not strict and key_of(v) == kl):
                best = (v, j)
    elif strategy == "forward":
        for v, j in cands:
            if key_of(v) > kl or (not strict and key_of(v) == kl):
                best = (v, j)
                break
    elif nearest_tie == "forward":
        for v, j in cands:
            if strict and key_of(v) == kl:
                continue
            if best is None or closer_or_equal(distance(on_l, v), distance(on_l, best[0])):
                best = (v, j)
    else:
        back = fwd = None
        for v, j in cands:
            if key_of(v) < kl or (not strict and key_of(v) == kl):
                back = (v, j)
            if fwd is None and (key_of(v) > kl or (not strict and key_of(v) == kl)):
                fwd = (v, j)
        best = back if fwd is None or (back is not None and closer_or_equal(distance(on_l, back[0]), distance(on_l, fwd[0]))) else fwd
    if best is None or not within(distance(on_l, best[0]), tolerance):
        return None
    return best[1]


def _valid(valid, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid, bool)


def join_asof(left_on, right_on, left_by=(), right_by=(), *, left_on_valid=None, right_on_valid=None, left_by_valid=None, right_by_valid=None, strategy="backward",
              strict=False, tolerance=None, nearest_tie="forward", linear=False):
    """left_by / right_by: sequences of arrays; *_by_valid: sequences of bool arrays or None.  -> (idx int64[N], matched bool[N])"""
    assert strategy in STRATEGIES and len(left_by) == len(right_by)
    n, m = len(left_on), len(right_on)
    lv, rv = _valid(left_on_valid, n).copy(), _valid(right_on_valid, m).copy()
    for j in range(len(left_by)):
        lv &= _valid(None if left_by_valid is None else left_by_valid[j], n)
        rv &= _valid(None if right_by_valid is None else right_by_valid[j], m)
    groups = {}
    for j in range(m):
        if rv[j]:
            groups.setdefault(tuple(key_of(b[j]) for b in right_by), []).append((key_of(right_on[j]), j))
    cands = {}
    for g, rows in groups.items():
        rows.sort()
        keys = sorted(set(k for k, _ in rows))
        rank = {k: i for i, k in enumerate(keys)}
        cands[g] = (keys, np.array([rank[k] for k, _ in rows], np.int64), [(right_on[j], j) for _, j in rows])
    idx, matched = np.zeros(n, np.int64), np.zeros(n, bool)
    for i in range(n):
        if not lv[i]:
            continue
        c = cands.get(tuple(key_of(b[i]) for b in left_by))
        if c is None:
            continue
        keys, ranks, rows = c
        if linear or (isinstance(left_on[i], (float, np.floating)) and math.isinf(float(left_on[i]))):
            near = rows          # (from an infinite on_l every finite candidate is at the same distance: no window)
        else:
            # the rows of the closest value below, of an equal value and of the closest value above on_l: the only rows any rule can pick
            kl = key_of(left_on[i])
            lo = _bisect(keys, kl)
            eq = lo < len(keys) and keys[lo] == kl
            first = int(np.searchsorted(ranks, max(lo - 1, 0), "left"))
            last = int(np.searchsorted(ranks, min(lo + (1 if eq else 0), len(keys) - 1), "right"))
            near = rows[first:last]
        j = match_row(left_on[i], near, strategy, strict, tolerance, nearest_tie)
        if j is not None:
            idx[i], matched[i] = j, True
    return idx, matched


def _bisect(keys, k):
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = (lo + hi) // 2
        if keys[mid] < k:
            lo = mid + 1
        else:
            hi = mid
    return lo


def check(got_idx, got_valid, want_idx, want_matched, what=""):
    """row by row and bit by bit: got_valid None means every row matched"""
    gv = np.ones(len(want_idx), bool) if got_valid is None else np.asarray(got_valid, bool)
    assert len(got_idx) == len(want_idx), (what, len(got_idx), len(want_idx))
    bad = np.flatnonzero(gv != want_matched)
    assert len(bad) == 0, (what, "validity differs at rows", bad[:8].tolist(), gv[bad[:8]].tolist())
    bad = np.flatnonzero(want_matched & (np.asarray(got_idx).astype(np.int64) != want_idx))
    assert len(bad) == 0, (what, "matched row differs at rows", bad[:8].tolist(), np.asarray(got_idx)[bad[:8]].tolist(), want_idx[bad[:8]].tolist())
    if got_valid is None:
        assert want_matched.all(), what


def self_check() -> int:
    """the hand-written vectors of the contract, and the windowed walk against the literal loop on random inputs; returns how many checks ran"""
    n = 0

    def one(on_l, on_r, want, **kw):
        nonlocal n
        for linear in (False, True):
            idx, ok = join_asof(np.asarray(on_l), np.asarray(on_r), linear=linear, **kw)
            got = [int(i) if o else None for i, o in zip(idx, ok)]
            assert got == want, (on_l, on_r, kw, got, want)
            n += 1

    one([5], [3, 7], [1], strategy="nearest")                                   # an equidistant pair goes to the forward value
    one([5], [3, 7, 7, 9], [2], strategy="nearest")                             # a duplicated forward value goes to its last row
    one([5], [3, 7, 7], [2], strategy="nearest")
    one([5], [4, 5, 5, 6], [2], strategy="backward")                            # exact duplicates go to the last one
    one([5], [4, 5, 5, 6], [2], strategy="nearest")
    one([5], [4, 5, 5, 6], [1], strategy="forward")                             # ... and forward to the first
    one([5], [4, 5, 5, 7], [0], strategy="nearest", strict=True)                # a strict nearest skips an exact match
    one([5], [3, 5, 5, 6, 6], [4], strategy="nearest", strict=True)
    one([5], [5, 5], [None], strategy="backward", strict=True)
    one([5], [5, 5], [None], strategy="forward", strict=True)
    one([10], [1, 9, 20], [None], strategy="nearest", tolerance=0)              # a tolerance that rejects the found match does not fall back
    one([10], [1, 30], [None], strategy="backward", tolerance=8)
    one([10], [1, 30], [0], strategy="backward", tolerance=9)
    one([10], [12, 11], [1], strategy="forward")                                # candidates go in (on, right row) order whatever the row order
    one([10, 0, 25], [20, 10, 10], [2, None, 0], strategy="backward")
    one([-(2 ** 63)], [2 ** 63 - 1], [0], strategy="forward", tolerance=2 ** 64 - 1)
    one([-(2 ** 63)], [2 ** 63 - 1], [None], strategy="forward", tolerance=2 ** 64 - 2)
    nan, inf = float("nan"), float("inf")
    one([nan], [1.0, nan], [1], strategy="backward", tolerance=0.0)             # equal codes are distance 0
    one([inf], [inf], [0], strategy="nearest", tolerance=0.0)
    one([nan], [1.0], [0], strategy="backward")                                 # a NaN distance matches without a tolerance ...
    one([nan], [1.0], [None], strategy="backward", tolerance=inf)               # ... and is within none
    one([1.0], [0.5, nan], [0], strategy="nearest")                             # a NaN distance loses against any number
    one([0.0], [-0.0], [0], strategy="forward", strict=False)                   # -0 == +0
    one([0.0], [-0.0], [None], strategy="forward", strict=True)
    one([1, 1, 2], [1, 1], [0, None, 0], left_by=[np.array([7, 8, 7])], right_by=[np.array([7, 9])], strategy="backward")     # groups; a group absent on the right
    one([1, 1], [1, 1], [None, None], left_by=[np.array([7, 7])], right_by=[np.array([7, 7])], strategy="backward",
        left_by_valid=[np.array([False, True])], right_by_valid=[np.array([False, False])])                                       # a null in a by part matches nothing
    one([1, 1], [0, 1], [0, None], strategy="backward", left_on_valid=np.array([True, False]), right_on_valid=np.array([True, False]))
    one([5], [3, 7], [0], strategy="nearest", nearest_tie="backward")
    one([5], [2, 7, 7], [1], strategy="nearest", nearest_tie="backward")
    rng = np.random.default_rng(20)
    for trial in range(60):
        nl, nr = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        if trial % 2:
            lo, ro = rng.integers(-6, 7, nl), rng.integers(-6, 7, nr)
            tol = [None, 0, 2][trial % 3]
        else:
            pool = np.array([-inf, -1.5, -0.0, 0.0, 0.5, 2.0, inf, nan])
            lo, ro = pool[rng.integers(0, 8, nl)], pool[rng.integers(0, 8, nr)]
            tol = [None, 0.0, 1.5][trial % 3]
        lb, rb = [rng.integers(0, 3, nl)], [rng.integers(0, 3, nr)]
        kw = dict(left_on_valid=rng.random(nl) < 0.9, right_on_valid=rng.random(nr) < 0.9, tolerance=tol)
        for strategy in STRATEGIES:
            for strict in (False, True):
                for tie in ("forward", "backward"):
                    a = join_asof(lo, ro, lb, rb, strategy=strategy, strict=strict, nearest_tie=tie, **kw)
                    b = join_asof(lo, ro, lb, rb, strategy=strategy, strict=strict, nearest_tie=tie, linear=True, **kw)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (trial, strategy, strict, tie)
                    n += 1
    return n
