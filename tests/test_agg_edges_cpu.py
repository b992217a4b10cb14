"""The tables and the exact reference of tests/agg_edges.py, checked without a GPU: the reference agrees with the oracle's q_groupby (the pinned restatement of
Polars) on every table, every required kind of group is in every table, and the layouts have the properties the GPU cases rely on (a row count that is no
multiple of 128, an edge group inside one wave of a clustered table, one that spans workgroups in a shuffled one, the two groups that the filter decides).

The reference is exact arithmetic and not the oracle itself: the oracle's Kahan f64 mean of [INT64_MAX, INT64_MIN] is 0.0 where the exact mean is -0.5 (inside
the bound of either; pinned below)."""
import math

import numpy as np
import pytest

from tests import agg_edges as E

OP_CODE = {"sum": 0, "mean": 1, "min": 2, "max": 3, "count": 4, "len": 5}      # oracle/pyoracle.py AGG_*


def oracle_groups(orc, t, filtered):
    """orc.q_groupby on the table's rows (behind the filter: the kept rows) -> (downloaded-style columns named after the ops, the group id of every result row)"""
    sel = t["keep"] if filtered else np.ones(t["n"], bool)
    keys = E.key_columns("hash", t["gid"][sel])
    v, ok = t["v"][sel], t["valid"][sel]
    aggs = [(op, OP_CODE[op], None if op == "len" else v, None if op == "len" else ok) for op in E.ops_of(t["dtype"])]
    r = orc.q_groupby([keys["k"][0]], [keys["k"][1]], aggs)
    got = {op: (r[op][0], r[op][1]) for op in E.ops_of(t["dtype"])}
    return got, E.gid_of_keys("hash", {"k": r["key_0"]})


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("dtype", list(E.NP))
def test_reference_agrees_with_the_oracle(orc, dtype, layout):
    t = E.table(dtype, layout)
    for filtered in (False, True):
        got, gids = oracle_groups(orc, t, filtered)
        what = (dtype, layout, "filtered" if filtered else "all rows")
        if dtype == "Boolean":       # the oracle's group-by takes a Boolean column as its UInt8 view (sum: Int64); orc.reduce pins the UInt32 of the Boolean sum
            assert got["sum"][0].dtype == np.int64 and orc.reduce(orc.AGG_SUM, np.array([True, True, False]))[1] == orc.U32
            got["sum"] = (got["sum"][0].astype(np.uint32), got["sum"][1])
        E.check_groups(got, gids, E.table_expected(t, filtered), dtype, what)


def test_the_known_disagreement_with_the_oracle_is_inside_the_bound(orc):
    lo, hi = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
    rows = [(hi, True), (lo, True)]
    assert E.aggregate(rows, "Int64", "mean") == -0.5 and E.aggregate(rows, "Int64", "sum") == -1
    r = orc.q_groupby([np.zeros(2, np.int64)], [None], [("m", orc.AGG_MEAN, np.array([hi, lo], np.int64), None)])
    assert float(r["m"][0][0]) == 0.0
    E.compare(float(r["m"][0][0]), -0.5, "Int64", "mean", rows)


def test_reference_rules():
    A = E.aggregate
    V = lambda *xs: [(x, True) for x in xs]
    nan, inf, big = E.NAN, E.INF, float(np.finfo(np.float64).max)
    assert A(V(nan, nan), "Float64", "min") != A(V(nan, nan), "Float64", "min") and A(V(nan, 2.0, nan), "Float64", "max") == 2.0
    assert A([(nan, False)], "Float64", "min") is None and A([(nan, False)], "Float64", "mean") is None and A([(nan, False)], "Float64", "sum") == 0.0
    assert math.isnan(A(V(inf, -inf), "Float64", "sum")) and A(V(inf, 1.0), "Float64", "sum") == inf and A(V(-inf, 1.0), "Float64", "mean") == -inf
    assert A(V(big, big), "Float64", "sum") == inf and A(V(-big, -big), "Float64", "sum") == -inf and A(V(big, big), "Float64", "mean") == inf
    f32 = float(np.finfo(np.float32).max)
    assert A(V(f32, f32), "Float32", "sum") == inf and A(V(f32, f32), "Float32", "mean") == f32
    assert A(V(-0.0, 0.0), "Float64", "min") == 0.0
    assert A(V(127, 127), "Int8", "sum") == 254 and A(V(255, 255), "UInt8", "sum") == 510 and A(V(65535, 65535), "UInt16", "sum") == 131070
    assert A(V(2 ** 31 - 1, 2 ** 31 - 1), "Int32", "sum") == -2 and A(V(2 ** 32 - 1, 2 ** 32 - 1), "UInt32", "sum") == 2 ** 32 - 2
    assert A(V(-2 ** 63, -2 ** 63), "Int64", "sum") == 0 and A(V(2 ** 64 - 1, 2 ** 64 - 1), "UInt64", "sum") == 2 ** 64 - 2
    assert A(V(1 << 62, 1 << 62, 1), "Int64", "sum") == -2 ** 63 + 1 and A(V(1 << 62, 1 << 62, 1), "UInt64", "sum") == 2 ** 63 + 1
    assert A(V(2 ** 64 - 1), "UInt64", "max") == 2 ** 64 - 1 and A(V(2 ** 64 - 1, 1), "UInt64", "mean") == 2.0 ** 63
    assert A(V(True, False, True), "Boolean", "sum") == 2 and E.out_dtype("Boolean", "sum") == "UInt32" and E.out_dtype("Int16", "sum") == "Int64"
    assert [E.out_dtype("Float32", op) for op in E.OPS] == ["Float32", "Float32", "Float32", "Float32", "UInt32", "UInt32"]


def test_compare_refuses_what_the_contract_refuses():
    rows = [(1.0, True), (2.0, True)]
    E.compare(3.0 + 2e-6, 3.0, "Float64", "sum", rows)
    for got, want, op in ((3.0 + 4e-6, 3.0, "sum"), (None, 3.0, "sum"), (3.0, None, "min"), (E.INF, E.NAN, "sum"), (E.NAN, E.INF, "sum"), (1e308, E.INF, "sum"),
                          (E.NAN, 1.0, "min"), (1.0, E.NAN, "max"), (1.5 + 2e-6, 1.5, "mean")):
        with pytest.raises(AssertionError):
            E.compare(got, want, "Float64", op, rows)
    with pytest.raises(AssertionError):
        E.compare(4, 5, "Int64", "sum", [(5, True)])
    E.compare(-0.0, 0.0, "Float64", "min", [(0.0, True)])          # the sign of a zero is not compared


@pytest.mark.parametrize("dtype", list(E.NP))
def test_every_table_has_every_required_kind_and_the_layouts_their_properties(dtype):
    want = {"Boolean": {"all_true", "all_false", "mixed", "all_null"},
            "float": {"all_null", "all_nan", "nan_ordered_first", "nan_ordered_last", "nan_ordered_middle", "pos_inf_only", "neg_inf_only", "both_inf", "pos_inf_finite",
                      "neg_inf_finite", "neg_zero_then_pos_zero", "pos_zero_then_neg_zero", "lone_neg_zero", "lone_denormal", "lone_max", "two_max", "two_lowest",
                      "nan_and_null", "one_valid_among_nulls", "benign_130"},
            "int": {"all_null", "lone_min", "lone_max", "min_and_max", "two_max", "two_min", "lone_zero", "one_valid_among_nulls", "benign_130"}}
    need = set(want["Boolean" if dtype == "Boolean" else "float" if dtype in E.FLOATS else "int"]) | {"null_key", "filter_only", "null_after_filter"}
    if dtype in ("Int8", "Int16", "Int32", "Int64"):
        need.add("lone_minus_one")
    if dtype == "UInt64":
        need |= {"at_and_above_2_63", "exact_sum_2_63_plus_1", "exact_sum_2_63_minus_1"}
    if dtype == "Int64":
        need |= {"exact_sum_2_63_plus_1", "exact_sum_2_63_minus_1", "exact_sum_minus_2_63_minus_1", "exact_sum_minus_2_63_plus_1"}
    assert need <= set(E.required_kinds(dtype))
    for layout in E.LAYOUTS:
        t = E.table(dtype, layout)
        kinds = t["kinds"]
        assert need <= set(kinds.values()), (layout, need - set(kinds.values()))
        assert t["n"] % 128 != 0 and 11_000 < t["n"] < 13_000 and t["v"].dtype == E.NP[dtype]
        assert kinds[E.NULL_GID] == "null_key" and len({g for g in kinds if g != E.NULL_GID}) == E.N_IDS and max(kinds) == E.N_IDS - 1
        assert np.array_equal(t["f"] > 0, t["keep"])
        span = {g: (int(np.nonzero(t["gid"] == g)[0].min()), int(np.nonzero(t["gid"] == g)[0].max())) for g in kinds}
        edge = [g for g, k in kinds.items() if k != "filler"]
        if layout == "clustered":
            assert any(a // 64 == b // 64 and b > a for a, b in (span[g] for g in edge))
            assert all(b - a + 1 == len(t["groups"][g]) for g, (a, b) in span.items())
        if layout == "shuffled":
            assert any(b - a > 2048 for a, b in (span[g] for g in edge))
        if layout == "interleaved":
            assert len(set(t["gid"][:E.N_IDS + 1].tolist())) == E.N_IDS + 1          # the first rows: one of every group
        by = {k: g for g, k in kinds.items()}
        unf, fil = E.group_rows(t, False), E.group_rows(t, True)
        assert by["filter_only"] in unf and by["filter_only"] not in fil
        g = by["null_after_filter"]
        assert any(ok for _, ok in unf[g]) and fil[g] and not any(ok for _, ok in fil[g])
        if dtype != "Boolean":
            assert [E.aggregate(fil[g], dtype, op) for op in E.OPS] == [0, None, None, None, 0, len(fil[g])]
        # the value of a kind: what it is there for
        if dtype in E.FLOATS:
            big = float(np.finfo(E.NP[dtype]).max)
            assert E.aggregate(unf[by["two_max"]], dtype, "sum") == E.INF and E.aggregate(unf[by["two_lowest"]], dtype, "sum") == -E.INF
            assert E.aggregate(unf[by["lone_max"]], dtype, "min") == big and math.isnan(E.aggregate(unf[by["nan_and_null"]], dtype, "max"))
            assert 0 < E.aggregate(unf[by["lone_denormal"]], dtype, "sum") < float(np.finfo(E.NP[dtype]).tiny)
        elif dtype != "Boolean":
            ii = np.iinfo(E.NP[dtype])
            wraps = np.dtype(E.NP[dtype]).itemsize >= 4
            assert (E.aggregate(unf[by["two_max"]], dtype, "sum") != 2 * int(ii.max)) == wraps
            assert E.aggregate(unf[by["lone_max"]], dtype, "min") == int(ii.max) and E.aggregate(unf[by["lone_min"]], dtype, "max") == int(ii.min)


@pytest.mark.parametrize("route", E.ROUTES)
def test_key_builders_are_injective_and_of_the_route(route):
    cols = E.key_values(route, np.arange(E.N_IDS))
    assert len({tuple(int(cols[c][j]) for c in cols) for j in range(E.N_IDS)}) == E.N_IDS
    k = cols["k"]
    if route == "lds":
        assert k.dtype == np.int16 and int(k.min()) == -1 and int(k.max()) < 40
    if route == "dense":
        assert k.dtype == np.uint16 and int(k.max()) == 49_999
    if route in ("hash", "wide"):
        assert k.dtype == np.int64 and int(k.max()) - int(k.min()) > 1 << 28
    t = E.table("Int64", "shuffled")
    kc = E.key_columns(route, t["gid"])
    got = {c: (v[:500], None if ok is None else ok[:500]) for c, (v, ok) in kc.items()}
    assert E.gid_of_keys(route, got) == t["gid"][:500].tolist()


def test_vectorised_reference_against_the_exact_one_on_a_planted_sample():
    """reference_np (the reference of the 2^24-row cases) on 2^16 rows with the same planted groups and a hot key, against aggregate() group by group"""
    rng = np.random.default_rng(3)
    n, G, hot = 1 << 16, 1500, 777
    ids = rng.integers(0, G, n)
    ids[rng.random(n) < 0.5] = hot
    p = E.planted(ids, hot, G)
    assert len(p["chosen"]) == 65 and hot in p["chosen"]
    ints, floats = {a for a, _ in p["chosen"].values()}, {b for _, b in p["chosen"].values()}
    assert ints >= set(E.edge_groups("Int64")) - {"benign_130"} and floats >= set(E.edge_groups("Float64")) - {"benign_130"}
    for col, dtype in (("v", "Int64"), ("x", "Float64")):
        vals, ok = p[col]
        ref = E.reference_np(ids, vals, ok)
        assert np.array_equal(ref["codes"], np.unique(ids))
        got = {op: (ref[op], None if op in ("sum", "count", "len") else ref["count"] > 0) for op in E.OPS}
        got["count"], got["len"] = (ref["count"].astype(np.uint32), None), (ref["len"].astype(np.uint32), None)
        rows_of = {int(g): [(vals[r].item(), bool(ok[r])) for r in np.nonzero(ids == g)[0]] for g in ref["codes"]}
        E.check_groups(got, [int(g) for g in ref["codes"]], E.expected(rows_of, dtype), dtype, col)
        # and the vectorised comparison accepts the reference itself
        assert E.check_against_np(got, ref, np.arange(len(ref["codes"])), dtype == "Float64", col) == 0.0
    hv, hm = p["x"][0][ids == hot], p["x"][1][ids == hot]
    assert hm[-1] and hv[-1] == -7.5 and np.isnan(hv[:-1][hm[:-1]]).all() and hm[:-1].any()
    iv, im = p["v"][0][ids == hot], p["v"][1][ids == hot]
    assert im.sum() == 1 and iv[im][0] == np.iinfo(np.int64).max
