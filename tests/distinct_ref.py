"""Reference for n_unique / unique() in plain numpy / Python: every value becomes a canonical token -- one NaN, -0 -> +0, a null a token of its own,
integers exact at any magnitude -- and classes of equal tokens are counted, or their rows picked, in row order.  Everything here is an exact integer or an exact
set of rows: there is no tolerance.  Where pandas is installed, self_check() compares with pandas.Series.nunique(dropna=False) and
DataFrame.drop_duplicates(keep=...) on NaN-free cases."""
import math

import numpy as np

KEEPS = ("any", "first", "last", "none")
NULL = ("null",)            # no value equals it


def canon(v, ok=True):
    """a value as the sort's equality sees it: null == null, NaN == NaN whatever the payload, -0 == +0"""
    if not ok:
        return NULL
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (float, np.floating)):
        return "nan" if math.isnan(v) else float(v) + 0.0
    return int(v)


def tokens(values, valid=None):
    values = np.asarray(values)
    ok = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    return [canon(v, m) for v, m in zip(values.tolist() if values.dtype.kind in "iub" else values, ok.tolist())]


def n_unique(values, valid=None):
    """distinct values, a null counting as one; 0 for an empty column"""
    return len(set(tokens(values, valid)))


def unique_rows(cols, keep):
    """row indices (ascending) that unique(keep) keeps over the columns [(values, valid or None)]"""
    assert keep in KEEPS
    parts = [tokens(v, m) for v, m in cols]
    classes = {}
    for r, key in enumerate(zip(*parts)):
        classes.setdefault(key, []).append(r)
    if keep == "last":
        rows = [rs[-1] for rs in classes.values()]
    elif keep == "none":
        rows = [rs[0] for rs in classes.values() if len(rs) == 1]
    else:
        rows = [rs[0] for rs in classes.values()]
    return sorted(rows)


def self_check():
    """the reference against pandas on NaN-free data (nulls as a mask); returns the number of comparisons, 0 without pandas"""
    try:
        import pandas as pd
    except ImportError:
        return 0
    rng = np.random.default_rng(416)
    done = 0
    for n in (0, 1, 2, 63, 64, 65, 500):
        a = rng.integers(-3, 4, n).astype(np.int64)
        b = rng.integers(0, 3, n).astype(np.int32)
        x = rng.integers(0, 5, n).astype(np.float64) / 4
        am = rng.random(n) > 0.2
        sa = pd.Series(pd.array(a, dtype="Int64")).mask(~am)
        assert n_unique(a, am) == sa.nunique(dropna=False), n
        assert n_unique(x) == pd.Series(x).nunique(dropna=False), n
        done += 2
        frame = pd.DataFrame({"a": sa, "b": b, "x": x})
        for subset, cols in ((["a"], [(a, am)]), (["a", "b"], [(a, am), (b, None)]), (["a", "b", "x"], [(a, am), (b, None), (x, None)])):
            for keep, pk in (("first", "first"), ("any", "first"), ("last", "last"), ("none", False)):
                want = frame.drop_duplicates(subset=subset, keep=pk).index.tolist()
                assert unique_rows(cols, keep) == want, (n, subset, keep)
                done += 1
    return done
