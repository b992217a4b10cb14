"""The inputs of the group-by route tests (tests/groupby_route_inputs.py) have the properties that make each GPU case reach its route -- computed here from the
builders alone, next to the planner arithmetic each property is derived from -- and the numpy reference agrees with a row-by-row evaluation.  No GPU: the only use
of the product is the compile-only plx_debug_program_json on placeholder columns, for the number of aggregate cells (n_aggs) the LDS table sizes depend on."""
import ctypes as C

import numpy as np
import pytest

import groupby_route_inputs as R


def n_agg_cells(case):
    """aggregate cells of the compiled query (mean = sum + count, count of a non-null column = len, ...)"""
    import polars_amd as pl
    from polars_amd import _ffi as F
    sers = []
    for name, (v, ok) in case["cols"].items():
        dt = pl.Categorical([], pl.UInt32) if name in case.get("dictionary", ()) else {"int8": pl.Int8, "int16": pl.Int16, "int32": pl.Int32, "int64": pl.Int64, "float64": pl.Float64}[v.dtype.name]
        h = C.c_uint64()
        F.check(F.lib().plx_column_placeholder(dt.physical, case["n"], int(ok is not None), 0, 0, 0, C.byref(h)))
        sers.append(pl.Series._from_handle(name, h.value, dt))
    return len(R.query(pl, pl.DataFrame(sers).lazy(), case).debug_program()["aggs"])


def distinct(case, rows=None):
    return len(np.unique(R.key_codes(case, rows)[0]))


def test_sample_rows_restate_the_planner_geometry():
    n = 17_000_003
    r = R.sample_rows(n)
    per, stride = 131072, (n // 8) & ~127
    assert len(r) == 8 * per and r[0] == 0 and r[per] == stride and r[-1] == 7 * stride + per - 1 and stride % 128 == 0
    assert np.array_equal(R.prefix_rows(n), np.arange(1 << 22)) and len(R.prefix_rows(1000)) == 1000


def test_planner_arithmetic_known_values():
    # slots the plan descriptions of the existing GPU tests report: 3 cells -> 4606 (tests/test_gpu_partition_geometry.py), 2 cells -> 6142
    assert R.hash_slots(3) == 4606 and R.hash_slots(2) == 6142
    assert R.hash_slots(3, wide_words=2) == 2632
    assert R.v1_plan(2, 9100) == (12, 6)
    assert abs(R.estimate_groups(7000, 1 << 20) - 7000) < 1 and R.estimate_groups(1 << 20, 1 << 20) == 1e18
    assert R.hash_plan(2, 4e6) is None and R.hash_plan(2, 1.2e6) == 8


def test_reference_agrees_with_a_row_loop():
    rng = np.random.default_rng(1)
    n = 5000
    a, b = rng.integers(-3, 3, n).astype(np.int64), rng.integers(0, 4, n).astype(np.int16)
    ok_b = rng.random(n) > 0.2
    v, x = rng.integers(-50, 50, n).astype(np.int64), rng.uniform(-1, 1, n)
    ok_x = rng.random(n) > 0.5
    ok_x[(a == 0) & ok_b & (b == 1)] = False                   # one group without any valid x
    ref = R.reference([a, b], [None, ok_b], [("s", "sum", (v, None)), ("c", "count", (x, ok_x)), ("mn", "min", (x, ok_x)), ("mx", "max", (v, None)), ("m", "mean", (x, ok_x)),
                                            ("xs", "sum", (x, ok_x)), ("n", "len", None)])
    groups = {}
    for i in range(n):
        groups.setdefault((int(a[i]), int(b[i]) if ok_b[i] else None), []).append(i)
    assert len(ref["codes"]) == len(groups) == 6 * 5
    ua, ub = ref["uniques"]
    for gi, code in enumerate(ref["codes"].tolist()):
        ia, ib = divmod(code, len(ub) + 1)
        rows = groups[(int(ua[ia]), int(ub[ib]) if ib < len(ub) else None)]
        xs = [x[i] for i in rows if ok_x[i]]
        A = ref["aggs"]
        assert A["s"][0][gi] == sum(int(v[i]) for i in rows) and A["n"][0][gi] == len(rows) and A["c"][0][gi] == len(xs) and A["mx"][0][gi] == max(int(v[i]) for i in rows)
        assert A["mn"][1][gi] == A["m"][1][gi] == bool(xs) and A["xs"][1][gi]
        if xs:
            assert A["mn"][0][gi] == min(xs) and abs(A["m"][0][gi] - sum(xs) / len(xs)) < 1e-12 and abs(A["xs"][0][gi] - sum(xs)) < 1e-12
        else:
            assert A["xs"][0][gi] == 0.0
    # ... and assert_groups_equal finds a wrong group, a missing null group and a moved row
    got = {"a": (ua[ref["codes"] // (len(ub) + 1)], None), "b": (np.append(ub, 0)[ref["codes"] % (len(ub) + 1)], ref["codes"] % (len(ub) + 1) < len(ub))}
    got.update({k: (val.copy(), ok.copy()) for k, (val, ok) in ref["aggs"].items()})
    perm = rng.permutation(len(ref["codes"]))
    shuffled = {k: (val[perm], None if ok is None else ok[perm]) for k, (val, ok) in got.items()}
    R.assert_groups_equal(shuffled, ref, ["a", "b"])
    bad = dict(got); s = got["s"][0].copy(); s[3] += 1; s[4] -= 1; bad["s"] = (s, got["s"][1])          # (the total stays the same)
    with pytest.raises(AssertionError):
        R.assert_groups_equal(bad, ref, ["a", "b"])
    bad = dict(got); bad["b"] = (got["b"][0], np.ones(len(ref["codes"]), bool))
    with pytest.raises(AssertionError):
        R.assert_groups_equal(bad, ref, ["a", "b"])
    big = np.full(4, 2 ** 62, np.int64)                        # integer sums beyond 2^53 take np.add.at
    assert R.reference([np.zeros(4, np.int64)], [None], [("s", "sum", (big // 4 + 1, None))])["aggs"]["s"][0][0] == 4 * (2 ** 60 + 1)


def test_empty_and_single_row_references():
    e = np.zeros(0, np.int64)
    ref = R.reference([e, e], [None, None], [("s", "sum", (e, None)), ("n", "len", None)])
    assert len(ref["codes"]) == 0 and len(ref["aggs"]["s"][0]) == 0
    ref = R.reference([np.array([5], np.int64)], [None], [("s", "sum", (np.array([-7], np.int64), None)), ("n", "len", None)])
    assert ref["aggs"]["s"][0].tolist() == [-7] and ref["aggs"]["n"][0].tolist() == [1]


@pytest.mark.parametrize("name", ["dense_flag", "dense_small"])
def test_dense_cases_pack_into_13_to_28_bits(name):
    """run_fused_groupby: <= 12 bits take lds_table, 13..28 bits dense_hbm_table when the partitioned route is not taken: no_partition, or fewer than 2^24 rows."""
    case = R.build(name)
    assert 13 <= R.packed_bits(case) <= 28 and R.packed_bits(case) == 9 + 6
    assert (case["n"] >= 1 << 24) == (name == "dense_flag")
    assert case["cols"]["b"][1] is not None and case["cols"]["x"][1] is not None        # a nullable key and a nullable value


def test_hash_nosample_is_below_the_sampling_threshold():
    """size_hash_table: n <= 2 * 2^22 rows -> no sample, cap = 2^max(10, ceil_log2(2 n))."""
    case = R.build("hash_nosample")
    assert case["n"] <= 1 << 23 and R.ceil_log2(2 * case["n"]) == 23
    k = case["cols"]["k"][0]
    assert int(k.max()) - int(k.min()) >= 1 << 26              # not a dense range: the raw 64-bit key, never a packed id


def test_grow_case_prefix_hides_the_keys():
    """no_partition -> size_hash_table samples the first 2^22 rows: d keys there -> cap = 2^max(12, ceil_log2(2 d + 1)); the table grows x4 per overflow, and a table
    of fewer slots than keys must overflow: from 2^12 at least three times until 2^18 >= the distinct keys."""
    case = R.build("grow")
    d = distinct(case, R.prefix_rows(case["n"]))
    total = distinct(case)
    assert d <= 400 and total >= 100_000 and case["n"] > 1 << 23
    G = min(R.estimate_groups(d, 1 << 22), case["n"])
    assert max(12, R.ceil_log2(int(G * 2.0) + 1)) == 12
    assert (1 << 16) < total < 0.6 * (1 << 18)                 # 2^12, 2^14 and 2^16 slots cannot hold them; 2^18 does at a load of 0.57


def test_overflow_retry_case_arithmetic():
    """Single key, second generation.  The strided sample holds 4096..8000 keys, none of them hot -> G ~ d, plan_for = 1.3 G: with two cells 6142 slots a partition and
    64 partitions.  All keys number ~1e6 > 64 x 6142 and > 128 x 6142: two overflows (growth: max(2 x, 1.01 x this plan's slots) -> 128, then 256 partitions); the
    third and last attempt holds them (256 x 6142 slots, load 0.64).
    First generation (PLX_PART_V=1): the first 2^22 rows hold the same few keys -> 64 partitions x 2^12 slots < keys: lds-overflow+, then the HBM hash table from
    2^14 slots, which is fewer than the keys too: grow+."""
    case = R.build("overflow_retry")
    n = case["n"]
    assert n_agg_cells(case) == 2
    codes, _ = R.key_codes(case)
    d, n_hot, G = R.sample_estimate(codes[R.sample_rows(n)])
    total = len(np.unique(codes))
    assert 4096 <= d <= 8000 and n_hot == 0 and 4096 <= G <= 8000 and total >= 990_000
    slots = R.hash_slots(2)
    lp0 = R.hash_plan(2, 1.3 * G)
    assert lp0 == 6 and total > (slots + 2) << 6
    est1 = max(2.6 * G, (slots << 6) * 1.01)
    assert R.hash_plan(2, est1) == 7 and total > (slots + 2) << 7
    est2 = max(2 * est1, (slots << 7) * 1.01)
    assert R.hash_plan(2, est2) == 8 and total < 0.7 * (slots << 8)
    # first generation
    dp = len(np.unique(codes[R.prefix_rows(n)]))
    assert dp <= 8000 and R.estimate_groups(dp, 1 << 22) >= 4096
    ls, lp = R.v1_plan(2, 1.3 * R.estimate_groups(dp, 1 << 22))
    assert (ls, lp) == (12, 6) and total > ((1 << ls) + 2) << lp
    assert max(12, R.ceil_log2(int(2 * R.estimate_groups(dp, 1 << 22)) + 1)) == 14 and total > 1 << 14


def _hot_case(name):
    case = R.build(name)
    codes, null_code = R.key_codes(case)
    sampled = codes[R.sample_rows(case["n"])]
    u, cnt = np.unique(sampled, return_counts=True)
    assert cnt.max() >= len(sampled) * 0.45                    # one key holds about half of the sampled rows
    return case, R.sample_estimate(sampled, null_code), len(np.unique(codes))


def test_hot_fits_case_arithmetic():
    """Heavy hitters in the sample -> plan_for = 4 G.  Six cells (sum, len, min, sum, count, ...) -> 2631 slots; 4 G ~ 4.8e5 fits 256 partitions, where the 1.3 G
    of a sample without hot keys would take 128: the partition count shows which rule planned.  (+- 5 % on the estimate does not change either.)"""
    case, (d, n_hot, G), total = _hot_case("hot_fits")
    cells = n_agg_cells(case)
    assert n_hot >= 1 and 100_000 <= total <= 125_000 and abs(G - total) < 0.05 * total
    assert case["cols"]["key"][1] is not None and case["cols"]["x"][1] is not None
    k = case["cols"]["key"][0]
    assert int(k.max()) - int(k.min()) > 1 << 62               # the learned key range never packs: the second run compiles the same key program and finds the cached sample
    for f in (0.95, 1.0, 1.05):
        assert R.hash_plan(cells, 4 * G * f) == 8 and R.hash_plan(cells, 1.3 * G * f) == 7
    assert total < 0.7 * (R.hash_slots(cells) << 8)


def test_hot_fallback_case_arithmetic():
    """~1e6 keys and a hot one, three cells (4606 slots): 4 G fits no plan (512 x 4606 x 0.95 = 2.24e6), the fallback 1.3 G takes 512 partitions."""
    case, (d, n_hot, G), total = _hot_case("hot_fallback")
    cells = n_agg_cells(case)
    assert cells == 3 and n_hot >= 1 and total >= 990_000 and abs(G - total) < 0.1 * total
    for f in (0.9, 1.0, 1.1):
        assert R.hash_plan(3, 4 * G * f) is None and R.hash_plan(3, 1.3 * G * f) == 9


def test_learned_case_looks_dense():
    case = R.build("learned")
    k = case["cols"]["key"][0]
    assert case["n"] >= 1 << 24 and int(k.max()) - int(k.min()) < 1 << 26 and n_agg_cells(case) == 2


@pytest.mark.parametrize("name", ["packed_hash", "packed_overflow"])
def test_packed_id_cases_arithmetic(name):
    """Packed ids of more than 25 bits take hash partitions (partition_plan2: direct-address tables up to 25 bits), at most 28 bits fall back to the dense HBM table.
    plan_for = min(2^bits, n, 1.3 x sampled estimate); ONE attempt.  packed_hash: the estimate is right, the tables hold the ids.  packed_overflow: the sample sees
    a few thousand ids -> 64 partitions, fewer slots than ids -> lds-overflow+ (no P=), dense_hbm_table."""
    case = R.build(name)
    cells = n_agg_cells(case)
    bits = R.packed_bits(case)
    assert 25 < bits <= 28 and bits == 26
    assert (cells << (bits + 3)) <= 8 << 30                    # the dense table is allowed (run_fused_groupby)
    codes, _ = R.key_codes(case)
    d, n_hot, G = R.sample_estimate(codes[R.sample_rows(case["n"])])
    total = len(np.unique(codes))
    lp = R.hash_plan(cells, min(float(1 << bits), case["n"], 1.3 * G))
    if name == "packed_hash":
        assert 280_000 <= total <= 320_000 and abs(G - total) < 0.1 * total and lp is not None and total < 0.8 * (R.hash_slots(cells) << lp)
        assert case["cols"]["b"][1] is not None and case["cols"]["x"][1] is not None
    else:
        assert 2000 <= d <= 8000 and total >= 1_900_000 and lp == 6 and total > (R.hash_slots(cells) + 2) << 6


def test_join_cases_arithmetic():
    """The bound from the plan (one group per surviving build row) replaces the estimate: plan_for = 1.02 x bound + 64.  The probe rows use 40 000 of the ~294 000
    surviving build rows, so a plan made from any sample of the joined rows would take fewer partitions than the one made from the bound:
    single key, three cells: 128 against 64 partitions; wide keys (two words, three cells: 2632 slots): 256 against 64."""
    j = R.build_join()
    assert j["n"] >= 1 << 24 and 280_000 <= j["build_rows"] < 300_000 and len(np.unique(j["build"]["k"])) == 300_000
    case = R.joined_case(j, "join_single_key")
    assert case["n"] == j["n"]                                 # every probe row finds its build row
    used = len(np.unique(case["cols"]["k"][0]))
    assert used == 40_000
    hint = j["build_rows"] * 1.02 + 64.0
    assert R.hash_plan(3, hint) == 7 and R.hash_plan(3, used * 1.3) == 6
    assert R.hash_plan(3, hint, wide_words=2) == 8 and R.hash_plan(3, used * 1.3, wide_words=2) == 6
    packed = R.joined_case(j, "join_packed_ids")
    assert 12 < R.packed_bits(packed) <= 25                    # direct-address LDS tables


@pytest.mark.parametrize("name,cells", [("v2_unavailable", 3), ("v1_single_key", None), ("v1_packed_ids", 2), ("v1_wide_keys", None)])
def test_remaining_cases(name, cells):
    """v2_unavailable / v1_single_key: sparse keys, >= 2^24 rows, >= 4096 groups (run_fused_groupby asks for that many before it partitions).  v1_single_key: the
    prefix sample's estimate x 1.3 has a first-generation plan.  v1_packed_ids: est = min(2^bits, n) has one."""
    case = R.build(name)
    assert case["n"] >= 1 << 24
    if cells is not None:
        assert n_agg_cells(case) == cells
    if name == "v1_wide_keys":
        assert all(int(case["cols"][k][0].max()) - int(case["cols"][k][0].min()) > 1 << 62 for k in case["keys"])      # nothing to pack
        return
    if name == "v1_packed_ids":
        bits = R.packed_bits(case)
        assert 12 < bits <= 28 and R.v1_plan(2, min(1 << bits, case["n"])) is not None
        return
    codes, _ = R.key_codes(case)
    dp = len(np.unique(codes[R.prefix_rows(case["n"])]))
    G = R.estimate_groups(dp, 1 << 22)
    assert G >= 4096 and int(case["cols"]["k"][0].max()) - int(case["cols"]["k"][0].min()) >= 1 << 26
    if name == "v1_single_key":
        ls, lp = R.v1_plan(n_agg_cells(case), 1.3 * G)
        assert len(np.unique(codes)) < 0.5 * ((1 << ls) << lp)
        assert case["cols"]["k"][1] is not None and case["cols"]["x"][1] is not None
