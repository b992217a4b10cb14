"""The exact plan text of the per-node hash joins (join::join_indices / join::join_indices_wide behind one driver, join_driver.hpp): the other join tests look for
fragments of it.  Three key routes x six kinds x the two frames in either position (so that inner and full joins build on either side).  The inputs are literals:
8 and 6 rows with a duplicated key on each side, a null key (a null in one part of a two-column key), keys that only one side has, and -1 as a key (its 64-bit
pattern is the single-key table's EMPTY word).  The `Join{...}` segment of pl.last_plan() must equal the text the parent of the driver refactoring printed for the same
inputs (PLANS: recorded there, never from the code under test), and the rows must equal a nested-loop join written in plain Python."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("inner", "left", "semi", "anti", "full", "right")
ROUTES = ("single", "packed", "wide")

# key parts per row; None = null.  `a` alone is the single key; (a, b) the two-column key: Int32 x Int32 packs into one Int64, Int64 x Float64 takes the wide route.
A_ROWS = {"a": [3, -1, 5, None, 3, 7, -1, 9], "b": [1, -1, 0, 2, 1, 4, -1, 1]}
B_ROWS = {"a": [-1, 3, 3, 2, 8, 5], "b": [-1, 1, 1, None, 0, 3]}
DTYPES = {"single": (np.int64,), "packed": (np.int32, np.int32), "wide": (np.int64, np.float64)}

# (route, kind, frames exchanged) -> the Join{...} segment on the parent commit
PLANS = {
    ("single", "inner", False): "Join{hash_join[build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=7], how=inner, gather x4}",
    ("single", "inner", True): "Join{hash_join[build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=7], how=inner, gather x4}",
    ("single", "left", False): "Join{hash_join[build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10], how=left, gather x4}",
    ("single", "left", True): "Join{hash_join[build=right rows=8 cap=2^4 dup-keys, probe rows=6, pairs=9], how=left, gather x4}",
    ("single", "semi", False): "Join{hash_semi_join[build=right rows=6 cap=2^4, probe rows=8, kept=5], gather x2}",
    ("single", "semi", True): "Join{hash_semi_join[build=right rows=8 cap=2^4, probe rows=6, kept=4], gather x2}",
    ("single", "anti", False): "Join{hash_anti_join[build=right rows=6 cap=2^4, probe rows=8, kept=3], gather x2}",
    ("single", "anti", True): "Join{hash_anti_join[build=right rows=8 cap=2^4, probe rows=6, kept=2], gather x2}",
    ("single", "full", False): "Join{hash_full_join[build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10, unmatched build rows=2], how=full, gather x4}",
    ("single", "full", True): "Join{hash_full_join[build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10, unmatched build rows=2], how=full, gather x4}",
    ("single", "right", False): "Join{hash_join[build=left rows=8 cap=2^4 dup-keys, probe rows=6, pairs=9], how=right, gather x4}",
    ("single", "right", True): "Join{hash_join[build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10], how=right, gather x4}",
    ("packed", "inner", False): "Join{packed 2 key columns into Int64; hash_join[build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=6], how=inner, gather x6}",
    ("packed", "inner", True): "Join{packed 2 key columns into Int64; hash_join[build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=6], how=inner, gather x6}",
    ("packed", "left", False): "Join{packed 2 key columns into Int64; hash_join[build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10], how=left, gather x6}",
    ("packed", "left", True): "Join{packed 2 key columns into Int64; hash_join[build=right rows=8 cap=2^4 dup-keys, probe rows=6, pairs=9], how=left, gather x6}",
    ("packed", "semi", False): "Join{packed 2 key columns into Int64; hash_semi_join[build=right rows=6 cap=2^4, probe rows=8, kept=4], gather x3}",
    ("packed", "semi", True): "Join{packed 2 key columns into Int64; hash_semi_join[build=right rows=8 cap=2^4, probe rows=6, kept=3], gather x3}",
    ("packed", "anti", False): "Join{packed 2 key columns into Int64; hash_anti_join[build=right rows=6 cap=2^4, probe rows=8, kept=4], gather x3}",
    ("packed", "anti", True): "Join{packed 2 key columns into Int64; hash_anti_join[build=right rows=8 cap=2^4, probe rows=6, kept=3], gather x3}",
    ("packed", "full", False): "Join{packed 2 key columns into Int64; hash_full_join[build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10, unmatched build rows=3], how=full, gather x6}",
    ("packed", "full", True): "Join{packed 2 key columns into Int64; hash_full_join[build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10, unmatched build rows=3], how=full, gather x6}",
    ("packed", "right", False): "Join{packed 2 key columns into Int64; hash_join[build=left rows=8 cap=2^4 dup-keys, probe rows=6, pairs=9], how=right, gather x6}",
    ("packed", "right", True): "Join{packed 2 key columns into Int64; hash_join[build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10], how=right, gather x6}",
    ("wide", "inner", False): "Join{wide_hash_join[words=2 (Float64 key part), build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=6], how=inner, gather x6}",
    ("wide", "inner", True): "Join{wide_hash_join[words=2 (Float64 key part), build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=6], how=inner, gather x6}",
    ("wide", "left", False): "Join{wide_hash_join[words=2 (Float64 key part), build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10], how=left, gather x6}",
    ("wide", "left", True): "Join{wide_hash_join[words=2 (Float64 key part), build=right rows=8 cap=2^4 dup-keys, probe rows=6, pairs=9], how=left, gather x6}",
    ("wide", "semi", False): "Join{wide_hash_semi_join[words=2 (Float64 key part), build=right rows=6 cap=2^4, probe rows=8, kept=4], gather x3}",
    ("wide", "semi", True): "Join{wide_hash_semi_join[words=2 (Float64 key part), build=right rows=8 cap=2^4, probe rows=6, kept=3], gather x3}",
    ("wide", "anti", False): "Join{wide_hash_anti_join[words=2 (Float64 key part), build=right rows=6 cap=2^4, probe rows=8, kept=4], gather x3}",
    ("wide", "anti", True): "Join{wide_hash_anti_join[words=2 (Float64 key part), build=right rows=8 cap=2^4, probe rows=6, kept=3], gather x3}",
    ("wide", "full", False): "Join{wide_hash_full_join[words=2 (Float64 key part), build=right rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10, unmatched build rows=3], how=full, gather x6}",
    ("wide", "full", True): "Join{wide_hash_full_join[words=2 (Float64 key part), build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10, unmatched build rows=3], how=full, gather x6}",
    ("wide", "right", False): "Join{wide_hash_join[words=2 (Float64 key part), build=left rows=8 cap=2^4 dup-keys, probe rows=6, pairs=9], how=right, gather x6}",
    ("wide", "right", True): "Join{wide_hash_join[words=2 (Float64 key part), build=left rows=6 cap=2^4 dup-keys, probe rows=8, pairs=10], how=right, gather x6}",
}


def _frame(pl, rows, route, rowcol):
    cols = []
    for name, dt in zip(("a", "b"), DTYPES[route]):
        valid = np.array([v is not None for v in rows[name]])
        cols.append(pl.Series(name, np.array([0 if v is None else v for v in rows[name]], dtype=dt), validity=valid))
    return pl.DataFrame(cols + [pl.Series(rowcol, np.arange(len(rows["a"]), dtype=np.int64))])


def _keys(rows, route):
    return list(zip(*(rows[name] for name in ("a", "b")[:len(DTYPES[route])])))


def reference(lkeys, rkeys, how):
    """nested loops over the key tuples: (left row, right row) with None for the missing side; semi / anti: the kept left rows"""
    def eq(x, y):
        return None not in x and None not in y and x == y
    if how in ("semi", "anti"):
        return [(i, None) for i, x in enumerate(lkeys) if any(eq(x, y) for y in rkeys) == (how == "semi")]
    pairs = [(i, j) for i, x in enumerate(lkeys) for j, y in enumerate(rkeys) if eq(x, y)]
    if how in ("left", "full"):
        pairs += [(i, None) for i in range(len(lkeys)) if all(p[0] != i for p in pairs)]
    if how in ("right", "full"):
        pairs += [(None, j) for j in range(len(rkeys)) if all(p[1] != j for p in pairs)]
    return pairs


def _column(out, name):
    v, valid = out[name]._download()
    return [int(x) if ok else None for x, ok in zip(v, valid if valid is not None else np.ones(len(v), bool))]


def run_case(pl, route, how, exchanged):
    """-> (the Join{...} segment of the plan, the output rows as (left row, right row), the reference rows)"""
    left, right = (B_ROWS, A_ROWS) if exchanged else (A_ROWS, B_ROWS)
    L, R = _frame(pl, left, route, "lrow"), _frame(pl, right, route, "rrow")
    out = L.lazy().join(R.lazy(), on=["a", "b"][:len(DTYPES[route])], how=how).collect(no_fusion=True)
    seg = re.search(r"Join\{[^}]*\}", pl.last_plan())
    lrow = _column(out, "lrow")
    rrow = _column(out, "rrow") if how not in ("semi", "anti") else [None] * len(lrow)
    return seg.group(0) if seg else None, list(zip(lrow, rrow)), reference(_keys(left, route), _keys(right, route), how)


def _sorted(pairs):
    return sorted(pairs, key=lambda p: tuple(-1 if v is None else v for v in p))


@pytest.mark.parametrize("exchanged", [False, True], ids=["8x6", "6x8"])
@pytest.mark.parametrize("how", KINDS)
@pytest.mark.parametrize("route", ROUTES)
def test_plan_text_and_rows(pl, route, how, exchanged):
    seg, got, want = run_case(pl, route, how, exchanged)
    print(seg)
    assert seg == PLANS[(route, how, exchanged)]
    if how in ("semi", "anti"):
        assert got == want                       # the kept rows, in left order
    else:
        assert _sorted(got) == _sorted(want)     # no order was asked for
