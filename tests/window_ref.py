"""Reference for window expressions (`f.over(keys)`) in plain numpy / Python, independent of the engine: the rows become canonical key tokens (the
tokens of tests/distinct_ref.py: one NaN, -0 -> +0, a null a token of its own, per key part), every partition's aggregate is computed once with numpy and given back
by row.  Quantiles come from tests/quantile_ref.py, distinct counts from tests/distinct_ref.py; sum / mean / min / max / count / len are computed the way
tests/agg_edges.py computes a group (its `aggregate`: exact integers, float sums as exact fractions rounded once); var / std are numpy's two-pass np.var, the
reference of tests/program_eval_var.py.

over(keys, values, valid, op, ...) -> (per-row list of Python numbers, None for null; the partition id of every row)."""
import numpy as np

from tests import agg_edges as AE
from tests import distinct_ref as D
from tests import quantile_ref as Q

OPS = ("sum", "mean", "min", "max", "count", "len", "var", "std", "quantile", "n_unique")
NP_NAME = {np.dtype(v): k for k, v in AE.NP.items()}


def partitions(keys):
    """keys: [(values, valid or None)] -> (ids per row in first-occurrence order, number of partitions)"""
    n = len(keys[0][0])
    parts = [D.tokens(v, m) for v, m in keys]
    seen, ids = {}, np.zeros(n, np.int64)
    for r, key in enumerate(zip(*parts)):
        ids[r] = seen.setdefault(key, len(seen))
    return ids, len(seen)


def aggregate(values, valid, op, ddof=1, q=0.5, interpolation="linear"):
    """one partition -> a Python number, or None for null.  values: a numpy array in the column's dtype (bool for Boolean)"""
    values = np.asarray(values)
    ok = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    vv = values[ok]
    if op == "len":
        return len(values)
    if op == "count":
        return int(ok.sum())
    if op == "n_unique":
        return D.n_unique(values, ok)
    if op in ("var", "std"):
        x = vv.astype(np.float64)
        if len(x) <= ddof:
            return None
        v = float(np.var(x, ddof=ddof))
        return float(np.sqrt(v)) if op == "std" else v
    if op == "quantile":
        return Q.ref_quantile(vv, q, interpolation)
    name = NP_NAME[values.dtype]                               # (Boolean: sum counts the trues as UInt32, mean is their share)
    rows = list(zip(values.tolist(), ok.tolist()))
    return AE.aggregate(rows, name, op)


def over(keys, values, valid, op, **params):
    """-> (want, ids): want[r] = the aggregate of the partition of row r (None: null)"""
    ids, G = partitions(keys)
    n = len(ids)
    per = []
    for g in range(G):
        sel = ids == g
        per.append(aggregate(None if values is None else np.asarray(values)[sel], None if valid is None else np.asarray(valid)[sel], op, **params)
                   if values is not None else int(sel.sum()))
    return [per[ids[r]] for r in range(n)], ids


def self_check():
    """the reference against itself on what it must get right whatever the engine does: token equality, nulls as partitions, broadcast by row"""
    k = (np.array([1.0, np.nan, -0.0, 0.0, np.nan, 1.0]), np.array([True, True, True, True, True, False]))
    ids, G = partitions([k])
    assert ids.tolist() == [0, 1, 2, 2, 1, 3] and G == 4
    ids, G = partitions([(np.array([1, 1, 1, 1]), np.array([False, False, True, True])), (np.array([1, 2, 1, 2]), None)])
    assert G == 4                                             # (null, 1) != (null, 2)
    want, _ = over([(np.array([0, 1, 0, 1, 2]), None)], np.array([1, 2, 3, 4, 5], np.int64), np.array([True, True, True, False, False]), "sum")
    assert want == [4, 2, 4, 2, 0]
    want, _ = over([(np.array([0, 1, 0, 1, 2]), None)], np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([True, True, True, False, False]), "mean")
    assert want == [2.0, 2.0, 2.0, 2.0, None]
    want, _ = over([(np.array([0, 0, 1]), None)], np.array([1.0, 3.0, 5.0]), None, "var")
    assert want == [2.0, 2.0, None]
    want, _ = over([(np.array([0, 0, 1]), None)], None, None, "len")
    assert want == [2, 2, 1]
    return 6
