"""Tables and the exact reference of the grouped-aggregate edge tests (tests/test_agg_edges_cpu.py, tests/test_gpu_agg_edges.py, tests/groupby_route_worker.py).
Plain numpy and Python arithmetic: nothing here imports the product.

A table is a set of groups; a group is a short list of (value, valid, kept) rows of one value dtype, and its `kind` says which edge it puts into an aggregate cell:
NaN, infinities, signed zeros, denormals, the largest finite values, integers at the bounds of their type, sums that wrap, groups without a valid row.  The null
key carries an edge kind; one group lives only in rows that the filter f > 0 rejects (it must not appear behind the filter); one keeps only null rows behind it.
A layout orders the rows (clustered / interleaved / shuffled), a key builder turns group ids into the key columns of one group-by route.

reference() is exact: Python integers wrapped to the output dtype, fractions.Fraction for float sums and every mean (correctly rounded, +-inf beyond the range).
Null rows carry a payload that would show in every aggregate (NaN / the type's maximum / True): a kernel that reads a value without its validity bit fails."""
import math
from fractions import Fraction

import numpy as np

try:
    from tests import groupby_route_inputs as R
except ImportError:                                    # (started as a script from tests/: the worker)
    import groupby_route_inputs as R

RTOL = R.RTOL                    # BASELINE.json north_star: the project's margin for float sums
NP = {"Float64": np.float64, "Float32": np.float32, "Int8": np.int8, "Int16": np.int16, "Int32": np.int32, "Int64": np.int64,
      "UInt8": np.uint8, "UInt16": np.uint16, "UInt32": np.uint32, "UInt64": np.uint64, "Boolean": np.bool_}
FLOATS = ("Float64", "Float32")
INTS = tuple(d for d in NP if d not in FLOATS and d != "Boolean")
OPS = ("sum", "mean", "min", "max", "count", "len")
LAYOUTS = ("clustered", "interleaved", "shuffled")
ROUTES = ("lds", "dense", "hash", "wide")
N_IDS = 40                       # group ids 0..39 (the LDS route packs int16 ids in [-1, 40) into its table) + the null key
NULL_GID = -1
N_TARGET = 12_000
NAN, INF = float("nan"), float("inf")


def ops_of(dtype):
    return ("sum", "mean", "count", "len") if dtype == "Boolean" else OPS


def out_dtype(dtype, op):
    """The result's dtype name: count / len UInt32; sum Int64 for 1- and 2-byte integers, UInt32 for Boolean, else the input's; mean Float32 for Float32, else Float64."""
    if op in ("count", "len"):
        return "UInt32"
    if op == "sum":
        return "UInt32" if dtype == "Boolean" else ("Int64" if dtype in ("Int8", "Int16", "UInt8", "UInt16") else dtype)
    if op == "mean":
        return "Float32" if dtype == "Float32" else "Float64"
    return dtype


def null_payload(dtype):
    return NAN if dtype in FLOATS else (True if dtype == "Boolean" else int(np.iinfo(NP[dtype]).max))


# ------------------------------------------------------------------------------------------------ edge groups
def edge_groups(dtype):
    """{kind: [(value, valid)]}, the rows in the order a clustered layout keeps.  Values are Python numbers that the dtype holds exactly."""
    V = lambda *xs: [(x, True) for x in xs]
    N = lambda k=1: [(null_payload(dtype), False)] * k
    rng = np.random.default_rng(130)
    if dtype == "Boolean":
        return {"all_null": N(4), "all_true": V(True, True, True), "all_false": V(False, False), "mixed": V(True, False, False, True, True),
                "one_valid_among_nulls": N(2) + V(True) + N(3), "benign_130": V(*(bool(b) for b in rng.random(130) < 0.4))}
    if dtype in FLOATS:
        fi = np.finfo(NP[dtype])
        MAX, DEN = float(fi.max), float(fi.smallest_subnormal)
        benign = [float(NP[dtype](x)) for x in rng.uniform(-8, 8, 130)]
        return {"all_null": N(4), "all_nan": V(NAN, NAN, NAN),
                "nan_ordered_first": V(2.5, NAN, NAN), "nan_ordered_last": V(NAN, NAN, -2.5), "nan_ordered_middle": V(NAN, 1.5, NAN),
                "pos_inf_only": V(INF, INF), "neg_inf_only": V(-INF), "both_inf": V(INF, -INF),
                "pos_inf_finite": V(1.0, INF, -3.0), "neg_inf_finite": V(-INF, 4.0, 2.0),
                "neg_zero_then_pos_zero": V(-0.0, 0.0), "pos_zero_then_neg_zero": V(0.0, -0.0), "lone_neg_zero": V(-0.0),
                "lone_denormal": V(DEN), "lone_max": V(MAX), "lone_lowest": V(-MAX), "two_max": V(MAX, MAX), "two_lowest": V(-MAX, -MAX),
                "nan_and_null": V(NAN) + N(2) + V(NAN), "one_valid_among_nulls": N(2) + V(3.25) + N(3), "benign_130": V(*benign)}
    ii = np.iinfo(NP[dtype])
    lo, hi = int(ii.min), int(ii.max)
    span = min(hi, 1000)
    g = {"all_null": N(4), "lone_min": V(lo), "lone_max": V(hi), "min_and_max": V(lo, hi), "two_max": V(hi, hi), "two_min": V(lo, lo), "lone_zero": V(0),
         "one_valid_among_nulls": N(2) + V(hi - 3) + N(3), "benign_130": V(*(int(x) for x in rng.integers(max(lo, -span), span + 1, 130)))}
    if lo < 0:
        g["lone_minus_one"] = V(-1)
    if dtype == "UInt64":
        g["at_and_above_2_63"] = V(1 << 63, (1 << 63) + 5, hi)
        g["exact_sum_2_63_plus_1"] = V(1 << 62, 1 << 62, 1)
        g["exact_sum_2_63_minus_1"] = V(1 << 62, (1 << 62) - 1)
    if dtype == "Int64":
        g["exact_sum_2_63_plus_1"] = V(1 << 62, 1 << 62, 1)
        g["exact_sum_2_63_minus_1"] = V(1 << 62, (1 << 62) - 1)
        g["exact_sum_minus_2_63_minus_1"] = V(lo, -1)
        g["exact_sum_minus_2_63_plus_1"] = V(-(1 << 62), -(1 << 62), 1)
    return g


def key_kinds(dtype):
    """The three groups that are about keys and the filter: {kind: [(value, valid, kept)]}."""
    p = null_payload(dtype)
    if dtype == "Boolean":
        a, b, nk = True, False, [(True, True, True), (p, False, True), (True, True, True)]
    elif dtype in FLOATS:
        a, b, nk = 5.0, -6.0, [(NAN, True, True), (-1.25, True, True), (NAN, True, True)]
    else:
        ii = np.iinfo(NP[dtype])
        a, b, nk = int(ii.max), int(ii.min), [(int(ii.min), True, True), (int(ii.max), True, True)]
    return {"null_key": nk,
            "filter_only": [(a, True, False), (b, True, False), (p, False, False)],
            "null_after_filter": [(a, True, False), (p, False, True), (b, True, False), (p, False, True), (p, False, True)]}


def required_kinds(dtype):
    return list(edge_groups(dtype)) + list(key_kinds(dtype))


def _filler(dtype, rng, rows):
    if dtype == "Boolean":
        v = [bool(x) for x in rng.random(rows) < 0.5]
    elif dtype in FLOATS:
        v = [float(NP[dtype](x)) for x in rng.uniform(-100, 100, rows)]
    else:
        ii = np.iinfo(NP[dtype])
        v = [int(x) for x in rng.integers(max(int(ii.min), -1000), min(int(ii.max), 1000) + 1, rows)]
    ok, keep = rng.random(rows) > 0.1, rng.random(rows) > 0.3
    return [(v[i] if ok[i] else null_payload(dtype), bool(ok[i]), bool(keep[i])) for i in range(rows)]


# ------------------------------------------------------------------------------------------------ tables
_TABLES = {}


def table(dtype, layout, n_target=N_TARGET):
    """-> {"n", "gid" (int64 per row, NULL_GID = the null key), "v", "valid", "keep", "f" (Int32: the filter is f > 0), "kinds" {gid: kind},
    "groups" {gid: [(value, valid, kept)] in row order}}, of about n_target rows.  Edge kinds take the ids from 0, filler groups of benign values the rest up to N_IDS."""
    if (dtype, layout, n_target) in _TABLES:
        return _TABLES[dtype, layout, n_target]
    rng = np.random.default_rng(20 + list(NP).index(dtype))
    kinds, groups = {}, {}
    for kind, rows in edge_groups(dtype).items():
        kinds[len(groups)] = kind
        groups[len(groups)] = [(v, ok, True) for v, ok in rows]
    for kind, rows in key_kinds(dtype).items():
        gid = NULL_GID if kind == "null_key" else len([g for g in groups if g != NULL_GID])
        kinds[gid], groups[gid] = kind, list(rows)
    first_filler = len(groups) - 1
    assert first_filler < N_IDS - 4
    left = n_target - sum(len(r) for r in groups.values())
    fillers = list(range(first_filler, N_IDS))
    weights = np.arange(1, len(fillers) + 1, dtype=np.float64)
    sizes = np.maximum(2, (left * weights / weights.sum()).astype(int))
    if (n_target - left + int(sizes.sum())) % 128 == 0:
        sizes[0] += 1
    for gid, rows in zip(fillers, sizes):
        kinds[gid], groups[gid] = "filler", _filler(dtype, rng, int(rows))
    # clustered order: the null key's rows in the middle of the edge groups, not at either end
    order = sorted(g for g in groups if g != NULL_GID)
    order.insert(len(order) // 4, NULL_GID)
    gid = np.concatenate([np.full(len(groups[g]), g, np.int64) for g in order])
    pos = np.concatenate([np.arange(len(groups[g])) for g in order])
    flat = [r for g in order for r in groups[g]]
    n = len(flat)
    if layout == "clustered":
        perm = np.arange(n)
    elif layout == "interleaved":                       # round robin over the groups: row i of every group, then row i + 1
        perm = np.lexsort((gid, pos))
    elif layout == "shuffled":
        perm = np.random.default_rng(7).permutation(n)
    else:
        raise KeyError(layout)
    v = np.array([flat[i][0] for i in perm], dtype=NP[dtype])
    t = {"n": n, "dtype": dtype, "layout": layout, "gid": gid[perm], "v": v, "valid": np.array([flat[i][1] for i in perm], bool),
         "keep": np.array([flat[i][2] for i in perm], bool), "kinds": kinds}
    t["f"] = np.where(t["keep"], 1 + (np.arange(n) % 5), -(np.arange(n) % 3)).astype(np.int32)
    t["groups"] = {g: [(flat[i][0], flat[i][1], flat[i][2]) for i in perm[t["gid"] == g]] for g in groups}
    assert n % 128 != 0
    _TABLES[dtype, layout, n_target] = t
    return t


def group_rows(t, filtered):
    """{gid: [(value, valid)]} of the rows that take part (behind the filter: the kept rows; a group without any is absent)"""
    out = {}
    for g, rows in t["groups"].items():
        r = [(v, ok) for v, ok, keep in rows if keep or not filtered]
        if r:
            out[g] = r
    return out


# ------------------------------------------------------------------------------------------------ keys of a route
def key_values(route, ids):
    """the key columns' values for non-null group ids"""
    ids = np.asarray(ids, np.int64)
    if route == "lds":
        return {"k": (ids - 1).astype(np.int16)}                                 # int16 in [-1, 39): with the null slot, a 6-bit packed id
    if route == "dense":
        return {"k": np.where(ids == N_IDS - 1, 49_999, ids * 1249).astype(np.uint16)}      # spread to 49 999: 16 bits, beyond the LDS table
    if route == "hash":
        return {"k": R.sparse(ids * 125)}                                       # a span of 2^32: no dense range even where the range is known
    if route == "wide":
        return {"k": R.full64(ids), "k2": R.full64(ids + 12345)}
    raise KeyError(route)


def key_columns(route, gid):
    """{name: (values, valid or None)}: the first key column is null in the null key's rows (the second, on the wide route, holds 77 there: one null group)"""
    ok = gid != NULL_GID
    cols = key_values(route, np.where(ok, gid, 0))
    out = {"k": (cols["k"], ok.copy())}
    if "k2" in cols:
        out["k2"] = (np.where(ok, cols["k2"], np.int64(77)), None)
    return out


def gid_of_keys(route, got, ids=range(N_IDS)):
    """downloaded key columns {name: (values, valid or None)} -> the group id of every result row (KeyError: a key that no group has)"""
    ids = list(ids)
    cols = key_values(route, ids)
    index = {tuple(int(cols[c][j]) for c in cols): g for j, g in enumerate(ids)}
    kv, kok = got["k"]
    out = []
    for r in range(len(kv)):
        if kok is not None and not kok[r]:
            assert "k2" not in got or int(got["k2"][0][r]) == 77
            out.append(NULL_GID)
        else:
            out.append(index[tuple(int(got[c][0][r]) for c in cols)])
    return out


# ------------------------------------------------------------------------------------------------ the exact reference
def _wrap(x, dtype):
    bits = 8 * np.dtype(NP[dtype]).itemsize
    x &= (1 << bits) - 1
    return x - (1 << bits) if dtype.startswith("Int") and x >> (bits - 1) else x


def _float_sum(vals):
    """the f64 sum by the rules of the contract: NaN if a NaN or both infinities are there, else the one infinity, else the exact sum correctly rounded
    (+-inf beyond the f64 range)"""
    if any(v != v for v in vals) or (INF in vals and -INF in vals):
        return NAN
    if INF in vals or -INF in vals:
        return INF if INF in vals else -INF
    s = sum((Fraction(v) for v in vals), Fraction(0))
    try:
        return float(s)                                 # (correctly rounded; -0.0 + -0.0 is not told from 0.0: the sign of a zero sum is not compared)
    except OverflowError:
        return INF if s > 0 else -INF


def _narrow(x, dtype):
    if dtype != "Float32":
        return x
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def aggregate(rows, dtype, op):
    """one group: rows = [(value, valid)] -> a Python number, or None for null"""
    vals = [v for v, ok in rows if ok]
    if op == "len":
        return len(rows)
    if op == "count":
        return len(vals)
    isf = dtype in FLOATS
    if op in ("min", "max"):
        if not vals:
            return None
        if isf:
            vals = [v for v in vals if v == v]
            if not vals:
                return NAN
        return min(vals) if op == "min" else max(vals)
    if op == "sum":
        return _narrow(_float_sum(vals), dtype) if isf else _wrap(sum(int(v) for v in vals), out_dtype(dtype, "sum"))
    if op == "mean":
        if not vals:
            return None
        if not isf:
            return float(Fraction(sum(int(v) for v in vals), len(vals)))
        s = _float_sum(vals)
        if not math.isfinite(s):
            return s                                    # the mean is the sum over the count: an overflowed sum stays infinite
        return _narrow(float(sum((Fraction(v) for v in vals), Fraction(0)) / len(vals)), dtype)
    raise ValueError(op)


def reference(groups_of_rows, dtype, op):
    """{key: [(value, valid)]} -> {key: value or None}"""
    return {g: aggregate(rows, dtype, op) for g, rows in groups_of_rows.items()}


def abs_sum(rows):
    s = sum((Fraction(abs(v)) for v, ok in rows if ok and math.isfinite(v)), Fraction(0))
    try:
        return float(s)
    except OverflowError:
        return INF


# ------------------------------------------------------------------------------------------------ comparison (section 4 of the contract)
def scale_of(rows, dtype):
    """(sum |x| over the valid finite rows, number of valid rows): what the bound of a float sum / mean is made of"""
    scale = abs_sum(rows) if dtype in FLOATS else float(sum(abs(int(v)) for v, ok in rows if ok))
    return scale, sum(1 for _, ok in rows if ok)


def compare(got, want, dtype, op, rows, what=""):
    """One cell: `got` / `want` are Python numbers or None (null); rows: the group's [(value, valid)], or their scale_of().  -> the relative error
    |got - want| / sum |x| of a finite float sum / mean (0.0 otherwise).
    Validity bit for bit; integers, count, len equal; float min / max equal as numbers, NaN for NaN -- the sign of a zero is NOT compared (min_ign keeps whichever
    of -0.0 / +0.0 it met first: order-dependent on the device); float sum / mean: a non-finite expectation is matched in kind, a finite one within
    RTOL * sum |x| (/ count for the mean), plus one f32 ulp of the reference for Float32 results."""
    assert (got is None) == (want is None), (what, op, "validity", got, want)
    if want is None:
        return 0.0
    isf = dtype in FLOATS
    if op in ("count", "len") or (not isf and op in ("sum", "min", "max")):
        assert int(got) == int(want), (what, op, got, want)
        return 0.0
    got = float(got)
    if op in ("min", "max"):
        assert (got != got and want != want) or got == want, (what, op, got, want)
        return 0.0
    if not math.isfinite(want):
        assert (got != got) if want != want else got == want, (what, op, got, want)
        return 0.0
    scale, cnt = rows if isinstance(rows, tuple) else scale_of(rows, dtype)
    per = scale / (cnt if op == "mean" else 1)
    bound = RTOL * per
    if out_dtype(dtype, op) == "Float32":
        bound += float(np.spacing(np.float32(abs(want)))) if abs(want) < float(np.finfo(np.float32).max) else 0.0
    assert math.isfinite(got) and abs(got - want) <= bound, (what, op, got, want, bound)
    return abs(got - want) / per if per > 0 and math.isfinite(per) else 0.0


def cell(col, r):
    """(values, valid or None) of a downloaded column -> the Python value of row r, None for null"""
    v, ok = col
    return None if (ok is not None and not ok[r]) else v[r].item()


_EXPECTED = {}


def expected(rows_of, dtype, memo=None):
    """{gid: {op: value or None, "scale": scale_of()}} of a set of groups; computed once per `memo` key (the exact sums take Fractions: shared among the cases)"""
    if memo is not None and memo in _EXPECTED:
        return _EXPECTED[memo]
    out = {g: dict({op: aggregate(rows, dtype, op) for op in ops_of(dtype)}, scale=scale_of(rows, dtype)) for g, rows in rows_of.items()}
    if memo is not None:
        _EXPECTED[memo] = out
    return out


def table_expected(t, filtered):
    """expected() of a table's groups: the same for every layout of a dtype and size"""
    return expected(group_rows(t, filtered), t["dtype"], (t["dtype"], t["n"], filtered))


def check_groups(got, gids, want, dtype, what=""):
    """got: downloaded result columns named after OPS; gids: the group id of every result row; want: expected().  The set of groups is the reference's; every
    cell by compare(); the dtype of every column is out_dtype().  -> the worst relative error of the float sums / means."""
    assert sorted(gids) == sorted(want), (what, "groups", sorted(set(gids) ^ set(want)))
    worst = 0.0
    for op in ops_of(dtype):
        assert got[op][0].dtype == NP[out_dtype(dtype, op)], (what, op, got[op][0].dtype)
        for r, g in enumerate(gids):
            worst = max(worst, compare(cell(got[op], r), want[g][op], dtype, op, want[g]["scale"], (what, g)))
    return worst


# ------------------------------------------------------------------------------------------------ 2^24 rows: planted groups and a vectorised reference
def planted(key_ids, hot_id, n_ids, seed=5):
    """Benign random Int64 / Float64 value columns for the rows of `key_ids`, with every row of ~64 chosen group ids overwritten by the edge kinds (Int64 kinds
    in v, Float64 kinds in x; a group smaller than its kind keeps the kind's head).  The hot key is among them: its x rows are NaN or null but for one ordered
    value in its last row, its v rows null but for one INT64_MAX.  -> {"v": (values, valid), "x": (values, valid), "chosen": {gid: (int kind, float kind)}}."""
    rng = np.random.default_rng(seed)
    n = len(key_ids)
    v, vm = rng.integers(-1000, 1000, n).astype(np.int64), rng.random(n) > 0.05
    x, xm = rng.uniform(-1, 1, n), rng.random(n) > 0.05
    ik, fk = edge_groups("Int64"), edge_groups("Float64")
    ik.pop("benign_130"), fk.pop("benign_130")
    cand = [int(g) for g in rng.permutation(n_ids) if g != hot_id][:64]
    order = np.argsort(key_ids, kind="stable")
    sk = key_ids[order]
    chosen = {}
    for j, g in enumerate(cand):
        rows = order[np.searchsorted(sk, g, "left"):np.searchsorted(sk, g, "right")]
        if len(rows) == 0:
            continue
        a, b = list(ik)[j % len(ik)], list(fk)[j % len(fk)]
        for col, mask, kind, pad in ((v, vm, ik[a], null_payload("Int64")), (x, xm, fk[b], NAN)):
            mask[rows] = False                          # rows beyond the kind: null
            col[rows] = pad
            for r, (val, ok) in zip(rows, kind):
                col[r], mask[r] = val, ok
        chosen[g] = (a, b)
    if hot_id is None:
        return {"v": (v, vm), "x": (x, xm), "chosen": chosen}
    rows = np.nonzero(key_ids == hot_id)[0]
    v[rows], vm[rows] = np.iinfo(np.int64).max - 1, False
    v[rows[len(rows) // 2]], vm[rows[len(rows) // 2]] = np.iinfo(np.int64).max, True
    x[rows], xm[rows] = NAN, rng.random(len(rows)) > 0.5
    x[rows[-1]], xm[rows[-1]] = -7.5, True
    chosen[int(hot_id)] = ("hot", "hot")
    return {"v": (v, vm), "x": (x, xm), "chosen": chosen}


BIG = {"hot_fits": ("full64", 120_000, 77_777), "learned": ("plain", 300_000, None), "v1_edges": ("sparse", 300_000, None)}      # case -> (key form, ids, hot id)


def planted_case(name):
    """A 2^24-row case of tests/groupby_route_inputs.py (its keys decide the route) with the planted value columns: {"n", "key": (values, valid or None), "ids",
    "G", "v", "x", "codes" (group id per row, G for the null key), "chosen"}.  The rows of the chosen groups keep a valid key: no edge row leaves its group."""
    form, G, hot = BIG[name]
    case = R.build(name)
    key, kvalid = case["cols"]["key" if "key" in case["cols"] else "k"]
    ids = case["ids"] if "ids" in case else (key - 1000)
    if name == "v1_edges":
        p = {"v": case["cols"]["v"], "x": case["cols"]["x"], "chosen": case["chosen"]}
    else:
        p = planted(ids, hot, G)
        if kvalid is not None:
            kvalid = kvalid | np.isin(ids, np.array(sorted(p["chosen"])))
    codes = ids.astype(np.int64) if kvalid is None else np.where(kvalid, ids, G).astype(np.int64)
    return {"n": case["n"], "name": name, "key": (key, kvalid), "ids": ids, "G": G, "v": p["v"], "x": p["x"], "codes": codes, "chosen": p["chosen"]}


def codes_of_keys(name, key_col):
    """downloaded key column (values, valid or None) of a planted case's result -> the group code of every result row"""
    form, G, _ = BIG[name]
    k, ok = key_col
    if form == "plain":
        ids = k.astype(np.int64) - 1000
    elif form == "sparse":
        ids = (k.astype(np.int64) + 10 ** 12) // 1_000_003
    else:
        lut = R.full64(np.arange(G))
        sorter = np.argsort(lut)
        ids = sorter[np.minimum(np.searchsorted(lut[sorter], k), G - 1)]
    ids = np.clip(ids, 0, G - 1)
    back = {"plain": lambda i: i + 1000, "sparse": R.sparse, "full64": R.full64}[form](ids)
    valid = np.ones(len(k), bool) if ok is None else ok
    assert np.array_equal(back[valid], k[valid]), "a key value that no row has"
    return np.where(valid, ids, G).astype(np.int64)


def check_planted(got, case, col, what=""):
    """one query's downloaded result (key + columns named after OPS) of a planted case against reference_np of value column `col` -> worst relative error"""
    vals, ok = case[col]
    ref = case.setdefault("ref_" + col, reference_np(case["codes"], vals, ok, case.setdefault("order", np.argsort(case["codes"], kind="stable"))))
    codes = codes_of_keys(case["name"], got["key"])
    order = np.argsort(codes, kind="stable")
    assert np.array_equal(codes[order], ref["codes"]), (what, "the groups are not those of the reference", len(codes), len(ref["codes"]))
    for op in OPS:
        want = NP[out_dtype("Int64" if col == "v" else "Float64", op)]
        assert got[op][0].dtype == want, (what, op, got[op][0].dtype)
    return check_against_np(got, ref, order, col == "x", what)


def reference_np(codes, values, valid, order=None):
    """The grouped aggregates of one value column at any size: sort by group code, reduceat.  Int64 sums wrap as numpy's do; np.fmin / np.fmax ignore NaN and
    give NaN for an all-NaN group; inf - inf and NaN propagate through np.add.  -> {"codes", "len", "count", "sum", "mean", "min", "max"} per distinct code;
    mean / min / max are meaningful where count > 0."""
    order = np.argsort(codes, kind="stable") if order is None else order
    sc = codes[order]
    starts = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    u = sc[starts]
    G = len(u)
    out = {"codes": u, "len": np.diff(np.r_[starts, len(sc)]).astype(np.int64)}
    ok = valid[order]
    gi = (np.cumsum(np.r_[True, sc[1:] != sc[:-1]]) - 1)[ok]
    vv = values[order][ok]
    cnt = np.bincount(gi, minlength=G).astype(np.int64)
    vs = np.flatnonzero(np.r_[True, gi[1:] != gi[:-1]]) if len(gi) else np.zeros(0, np.int64)
    has = gi[vs] if len(gi) else np.zeros(0, np.int64)
    isf = values.dtype.kind == "f"
    with np.errstate(all="ignore"):
        s = np.zeros(G, values.dtype)
        mn, mx = np.zeros(G, values.dtype), np.zeros(G, values.dtype)
        if len(vs):
            s[has] = np.add.reduceat(vv, vs)
            mn[has] = (np.fmin if isf else np.minimum).reduceat(vv, vs)
            mx[has] = (np.fmax if isf else np.maximum).reduceat(vv, vs)
        fs = np.zeros(G)
        if len(vs):
            fs[has] = np.add.reduceat(vv.astype(np.float64), vs)
        mean = fs / np.maximum(cnt, 1)
        asum = np.zeros(G)
        if len(vs):
            asum[has] = np.add.reduceat(np.where(np.isfinite(vv.astype(np.float64)), np.abs(vv.astype(np.float64)), 0.0), vs)
    out.update(count=cnt, sum=s, mean=mean, min=mn, max=mx, abs_sum=asum)
    return out


def check_against_np(got, ref, order, dtype_is_float, what=""):
    """got: downloaded columns named after OPS, `order`: for every reference group the result row that holds it.  Section 4, vectorised.  -> worst relative error."""
    cnt, has = ref["count"], ref["count"] > 0
    col = lambda op: (got[op][0][order], np.ones(len(order), bool) if got[op][1] is None else got[op][1][order])
    for op in ("len", "count"):
        v, ok = col(op)
        assert ok.all() and np.array_equal(v.astype(np.int64), ref[op]), (what, op)
    worst = 0.0
    for op in ("sum", "mean", "min", "max"):
        v, ok = col(op)
        want_ok = np.ones(len(cnt), bool) if op == "sum" else has
        assert np.array_equal(ok, want_ok), (what, op, "validity", int((ok != want_ok).sum()))
        w = ref[op]
        if op == "sum":
            w = np.where(has, w, 0)
        g, w = v[want_ok], w[want_ok]
        if not dtype_is_float and op != "mean":
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, op, int((g != w).sum()))
            continue
        g, w = g.astype(np.float64), w.astype(np.float64)
        if op in ("min", "max"):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
        else:
            fin = np.isfinite(w)
            scale = ref["abs_sum"][want_ok] / (np.maximum(cnt[want_ok], 1) if op == "mean" else 1)
            with np.errstate(all="ignore"):
                err = np.abs(g - w)
                bad = np.where(fin, ~(np.isfinite(g) & (err <= RTOL * scale)), ~((g == w) | (np.isnan(g) & np.isnan(w))))
                rel = np.where(fin & (scale > 0), err / np.where(scale > 0, scale, 1.0), 0.0)
            worst = max(worst, float(np.nanmax(rel)) if len(rel) else 0.0)
        assert not bad.any(), (what, op, f"{int(bad.sum())} groups differ", g[bad][:5], w[bad][:5])
    return worst
