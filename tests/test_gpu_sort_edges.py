"""The stable arg-sort and the top-k selection of kernels_sort.hip at their tile, digit, null and value edges: the rank sort up to and at its 2048-row / 8-key limits,
the radix passes on short and partial tiles and at the ranking-round edges, every digit alone, tiles built against the uint8 counts and the match-any ballots, and
the radix select at its bucket-walk, fall-back, tie and threshold edges -- through arg_sort_by and through the frame front ends.

The tables are tests/sort_edges.py (pinned without a GPU by tests/test_sort_edges_cpu.py); the reference is the oracle's sort_indices.  Every comparison is exact: the
index vector is uint32 and equal to the reference's element for element (the sort is stable, so ties are compared too), and every case asserts the route text of
pl.last_plan() it was built for, so that none passes on another path."""
import ctypes as C

import numpy as np
import pytest

from tests import sort_edges as E

pytestmark = pytest.mark.gpu
DIRECTIONS = [(d, nl) for d in (False, True) for nl in (False, True)]


def series(pl, name, v, valid=None):
    dt = [k for k, t in E.NP.items() if np.dtype(t) == v.dtype][0]
    return pl.Series(name, v, dtype=getattr(pl, E.PLDT[dt]), validity=valid)


def arg_sort(pl, keys, limit=-1):
    sers = [series(pl, "k%d" % j, k[0], k[1]) for j, k in enumerate(keys)]
    got = pl.arg_sort_by(sers, [k[2] for k in keys], [k[3] for k in keys], limit=limit).to_numpy()
    return got, pl.last_plan()


def check(pl, keys, what, route=None, limit=-1):
    """the index vector against the oracle, exactly, and the route (default: the one this many rows and keys must take, with its exact pass counts)"""
    got, plan = arg_sort(pl, keys, limit)
    want = E.reference(keys, limit)
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.dtype, got.shape, plan)
    assert np.array_equal(got, want), (what, plan, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    assert plan == (E.sort_route(keys) if route is None else route), (what, plan)
    return got, plan


# ============================================================================================================ 1. lengths on both paths
LENGTHS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4096 + 255, 4096 + 256, 4096 + 257, 4096 + 1023, 4096 + 1024, 4096 + 1025,
           2 * 4096 - 1, 2 * 4096, 2 * 4096 + 1, 3 * 4096 + 63, 3 * 4096 + 64, 3 * 4096 + 65]


@pytest.mark.parametrize("n", LENGTHS)
def test_one_key_at_the_length_edges_of_both_paths(pl, n):
    """small_rank_sort_kernel's second trip (1025 .. 2048 rows), the 2048 / 2049 hand-over, and the radix passes on tiles that end inside a wave, a sub-tile or a
    ranking round of 1024 keys, and on whole tiles"""
    i64, f64, valid = E.value_table("i64", n), E.value_table("f64", n), E.VALIDITY["third"](n)
    for d, nl in DIRECTIONS:
        for keys in ([(i64, None, d, nl)], [(f64, valid, d, nl)]):
            _, plan = check(pl, keys, (n, d, nl, keys[0][0].dtype))
            assert plan.startswith("rank_sort[rows=%d," % n if n <= E.SMALL_MAX else "radix_sort[rows=%d," % n), plan


def low_cardinality_keys(n, n_keys):
    """the first n_keys - 1 keys are constant or take two or three values; the last decides"""
    i = np.arange(n, dtype=np.int64)
    front = [(np.full(n, -5, dtype=np.int64), None, False, False), ((i % 2).astype(bool), None, True, False), (np.full(n, 200, dtype=np.uint8), None, False, True),
             ((i % 3 - 1).astype(np.int16), (i % 5) != 0, False, True), (np.where(i % 2 == 0, -0.0, 0.0).astype(np.float32), None, True, False),
             (np.full(n, 2.5), np.zeros(n, bool), False, False), (np.full(n, 2 ** 32 - 1, dtype=np.uint32), None, True, True), ((i % 2).astype(np.uint16), None, True, False)]
    return front[8 - (n_keys - 1):] + [(E.value_table("i32", n), None, True, False)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2048])
def test_nine_keys_take_the_radix_path_and_eight_the_rank_sort(pl, n):
    """kSmallMaxKeys from both sides: with nine keys the count / scan / scatter pass meets a tile shorter than one 256-key sub-tile, and tiles that end inside a wave"""
    keys = low_cardinality_keys(n, 9)
    _, plan = check(pl, keys, (n, 9))
    assert plan.startswith("radix_sort[rows=%d, keys=9," % n), plan
    keys = low_cardinality_keys(n, 8)
    check(pl, keys, (n, 8), route=E.rank_route(n, 8))


# ==================================================================================================== 2. every dtype at its value edges
@pytest.mark.parametrize("dt", E.DTYPES)
def test_every_dtype_at_its_value_edges(pl, dt):
    """encode_value for every dtype (the integer extremes, u64 above 2^63, +-inf, the largest and smallest finite values, float32 denormals widened to f64, -0 == +0,
    the three NaNs as one greatest value) in both directions and null placements, under every validity pattern: through the rank sort (1500 rows) and the radix sort
    (2049 rows, and 4096 + 257).  An all-null or one-valid key still orders the nulls by placement and keeps ties in row order: the oracle's vector says so."""
    for n in (1500, E.SMALL_MAX + 1, E.TILE + 257):
        v = E.value_table(dt, n)
        for vname, vf in E.VALIDITY.items():
            valid = vf(n)
            for d, nl in DIRECTIONS:
                got, plan = check(pl, [(v, valid, d, nl)], (dt, n, vname, d, nl))
                if n > E.SMALL_MAX and not d and (dt == "bool" or dt in E.UNSIGNED):
                    # an ascending unsigned key sorts at most its own `width` digits (a Boolean one).  `passes` also counts the null-rank pass sort_by_key adds
                    # where nulls and valid rows meet, so that one is taken off first
                    null_pass = 1 if valid is not None and valid.any() and not valid.all() else 0
                    assert int(plan.split("passes=")[1].split(",")[0]) - null_pass <= E.width(dt), (dt, vname, plan)
                if vname == "all_null":
                    assert np.array_equal(got, np.arange(n)), (dt, n, d, nl)
                if vname == "one_valid":
                    row = n // 2
                    rest = np.delete(np.arange(n), row)
                    assert np.array_equal(got, np.concatenate([[row], rest] if nl else [rest, [row]])), (dt, n, d, nl)


# ============================================================================================================================ 3. digits
@pytest.mark.parametrize("d", range(8))
def test_one_digit_alone_is_sorted_and_the_other_seven_are_skipped(pl, d):
    n = E.TILE + 257
    route = "radix_sort[rows=%d, keys=1, passes=1, uniform digits skipped=7]" % n
    for variant in E.DIGIT_VARIANTS:
        for signed in (False, True):
            for desc in (False, True):
                check(pl, [(E.digit_keys(d, n, variant, signed), None, desc, False)], (d, variant, signed, desc), route=route)


def test_a_constant_key_costs_no_pass(pl):
    """every digit of every key uniform: no pass runs and sort_indices fills the identity; under a second key only that key orders"""
    n = E.TILE + 257
    for const in (np.full(n, E.DIGIT_BASE, dtype=np.uint64), np.full(n, -1.5), np.full(n, True)):
        for desc in (False, True):
            got, plan = check(pl, [(const, None, desc, False)], (const.dtype, desc))
            assert "passes=0" in plan and np.array_equal(got, np.arange(n)), plan
    second = (E.value_table("f64", n), E.VALIDITY["third"](n), True, True)
    got, plan = check(pl, [(np.full(n, 7, dtype=np.int64), None, False, False), second], "constant first key")
    assert np.array_equal(got, E.reference([second]))
    got, plan = check(pl, [(np.full(n, 7, dtype=np.int64), np.zeros(n, bool), False, False), second], "all-null first key")
    assert np.array_equal(got, E.reference([second]))


# ============================================================================================================================= 4. tiles
@pytest.mark.parametrize("name", list(E.tile_patterns(64)))
def test_tile_patterns_on_the_lowest_and_the_highest_digit(pl, name):
    """radix_scatter_kernel's ranking: sorted and reversed tiles, sawteeth around the wave and the sub-tile, match-any groups of every size from 1 to 64, a tile that is
    constant on the digit next to one that is not (counts of 64 in every uint8 cell, prefixes up to 960), and every digit value 16 times per tile.  As the second of
    two keys the first key's pass has to keep the order this pass made."""
    n = 2 * E.TILE + 65
    p = E.tile_patterns(n)[name]
    first = ((np.arange(n) * 7) % 3).astype(np.uint8)
    for d in (0, 7):
        for signed in (False, True):
            key = (E.place_digit(p, d, signed), None, False, False)
            _, plan = check(pl, [key], (name, d, signed))
            assert "passes=1, uniform digits skipped=7" in plan, plan
            check(pl, [(first, None, True, False), key], (name, d, signed, "second key"))


# =============================================================================================================== 5. multi-key stability
@pytest.mark.parametrize("n", [E.SMALL_MAX, E.SMALL_MAX + 1])
def test_three_keys_that_tie(pl, n):
    i = np.arange(n)
    zeros = (np.where(i % 2 == 0, -0.0, 0.0).astype(np.float32), None, True, False)             # -0 == +0: every row ties
    nulls = (E.value_table("i16", n), np.zeros(n, bool), False, True)                          # all null: every row ties
    check(pl, [zeros, nulls, (E.value_table("u64", n), E.VALIDITY["third"](n), True, False)], (n, "third key decides"))
    nans = (E.from_bits("f64", [E.NAN_BITS["f64"][k % 3] for k in range(n)]), None, False, True)   # the three NaNs are one value: every row ties
    got, _ = check(pl, [zeros, nulls, nans], (n, "all tie"))
    assert np.array_equal(got, np.arange(n))


# ===================================================================================================================== 6. top-k selection
def topk_route(case, limit, rounds, cand):
    keys = case["keys"]
    n = len(keys[0][0])
    if cand is None:
        return E.sort_route(keys)
    codes = E.select_codes(keys[0])
    s = np.uint64(8 * (8 - rounds))
    bound = codes[E.reference(keys, limit)[limit - 1]] >> s
    rows = np.flatnonzero((codes >> s) <= bound)
    assert len(rows) == cand
    return E.select_route(rounds, cand) + E.sort_route(keys, rows)


@pytest.mark.parametrize("name", [c["name"] for c in E.topk_tables()])
def test_top_k_selection(pl, name):
    """The radix select at: one round with 2048 candidates (the rank sort through the candidate permutation) and 2049 (the radix sort with an initial permutation), the
    bucket walk where the bucket holds exactly `limit` rows and where one more row spills into the next bucket, all eight rounds with ties at the bound, candidates
    just below, at and above n / 2, a null code tying with a valid one (0 with nulls first, all ones with nulls last), every dtype as first key in both directions, a
    Boolean first key, and the n > 65536 / limit < n / 4 thresholds.  The route text carries the rounds and the candidate count the table was built for."""
    case = E.topk_case(name)
    for limit, rounds, cand in case["picks"]:
        got, plan = check(pl, case["keys"], (name, limit), route=topk_route(case, limit, rounds, cand), limit=limit)
        assert ("top_k_select" in plan) == (cand is not None), plan
        assert len(got) == min(limit, len(case["keys"][0][0]))


def test_top_k_answers_that_can_be_read_off_the_tables(pl):
    """what the selection must return, stated without the oracle"""
    n = E.N1
    tied = E.spread(n, 5000)
    got, _ = arg_sort(pl, E.topk_case("tied_5000")["keys"], 10)
    assert np.array_equal(got, tied[:10])                                                      # the first ten tied rows in row order
    keys = E.topk_case("tied_5000_second_key")["keys"]
    got, _ = arg_sort(pl, keys, 10)
    k2 = keys[1][0][tied].astype(np.int64)
    assert np.array_equal(got, tied[np.argsort(-k2, kind="stable")[:10]])                      # the ten the descending second key picks
    k, valid, _, _ = E.topk_case("nulls_first_z3000_min0")["keys"][0]
    got, _ = arg_sort(pl, E.topk_case("nulls_first_z3000_min0")["keys"], 100)
    assert not valid[got].any()                                                                # all nulls
    k, valid, _, _ = E.topk_case("nulls_first_z50_min30")["keys"][0]
    got, _ = arg_sort(pl, E.topk_case("nulls_first_z50_min30")["keys"], 60)
    assert not valid[got[:50]].any() and valid[got[50:]].all() and (k[got[50:]] == np.iinfo(np.int64).min).all()      # the nulls first although i64.min shares their code
    for name in ("u64_max", "u8_255", "u32_zero_desc"):
        keys = E.topk_case("nulls_last_" + name)["keys"]
        got, _ = arg_sort(pl, keys, 100)
        assert keys[0][1][got[:40]].all() and not keys[0][1][got[40:]].any()                   # the 40 valid rows, then nulls
    for dt in E.FLOATS:
        keys = E.topk_case("dtype_%s_desc" % dt)["keys"]
        got, _ = arg_sort(pl, keys[:1], 100)
        nan_rows = np.flatnonzero(np.isnan(keys[0][0]) & (keys[0][1] if keys[0][1] is not None else True))
        assert np.array_equal(got[:len(nan_rows)], nan_rows), dt                               # the NaNs of all three patterns first, in row order


def test_top_k_limit_zero_and_negative(pl):
    keys = E.topk_case("limit_thresholds")["keys"]
    got, plan = arg_sort(pl, keys, 0)
    assert got.dtype == np.uint32 and got.shape == (0,) and plan == "sort[empty]", plan
    check(pl, keys, "no limit", limit=-1)


# ---- through the front ends
def front_end_frame(pl):
    n = E.N1
    i = np.arange(n, dtype=np.int64)
    host = {"a": (E.topk_case("one_round_2048")["keys"][0][0], None), "b": (E.value_table("f64", n), E.VALIDITY["third"](n)), "flag": ((i % 5) < 2, (i % 7) != 3),
            "row": (i.astype(np.uint32), None)}
    words = ["w%02d" % ((k * 13) % 41) for k in range(n)]
    df = pl.DataFrame([series(pl, c, v, m) for c, (v, m) in host.items()] + [pl.Series("s", words)])
    return df, host, words


def same_rows(out, host, words, rows, what):
    """the whole frame against rows `rows` of the host columns: validity bit for bit, values on the valid rows bit for bit"""
    assert out.columns == list(host) + ["s"] and out.height == len(rows), (what, out.columns, out.height)
    for c, (v, m) in host.items():
        got, ok = out[c]._download()
        ok = np.ones(len(rows), bool) if ok is None else ok
        want_ok = np.ones(len(rows), bool) if m is None else m[rows]
        assert np.array_equal(ok, want_ok), (what, c)
        g, w = got[ok], v[rows][ok]
        assert g.dtype == w.dtype and np.array_equal(E.bits_of(g) if g.dtype.kind == "f" else g, E.bits_of(w) if w.dtype.kind == "f" else w), (what, c)
    assert out["s"].to_list() == [words[r] for r in rows], (what, "s")


def test_top_k_through_the_frame_front_ends(pl):
    """slice-over-sort with a positive offset (offset + length is the limit), head, tail (no pushdown), DataFrame.top_k / bottom_k with `reverse` per key: whole frames,
    a Boolean, a nullable and a string column aboard, so the gather behind the sort is compared too"""
    df, host, words = front_end_frame(pl)
    n = E.N1
    a, b = host["a"], host["b"]
    by = dict(descending=[False, True], nulls_last=[False, True])
    keys = [(a[0], None, False, False), (b[0], b[1], True, True)]
    order = E.reference(keys)
    out = df.lazy().sort("a", "b", **by).slice(5, 95).collect()
    assert "Sort{" + E.select_route(1, E.SMALL_MAX) + E.rank_route(E.SMALL_MAX, 2) in pl.last_plan(), pl.last_plan()
    same_rows(out, host, words, order[5:100], "slice(5, 95)")
    out = df.lazy().sort("a", "b", **by).head(1500).collect()
    assert E.select_route(1, E.SMALL_MAX) in pl.last_plan(), pl.last_plan()
    same_rows(out, host, words, order[:1500], "head")
    out = df.lazy().sort("a", "b", **by).tail(70).collect()
    assert "top_k_select" not in pl.last_plan() and "Sort{radix_sort[rows=%d, keys=2," % n in pl.last_plan(), pl.last_plan()
    same_rows(out, host, words, order[-70:], "tail")
    out = df.bottom_k(90, by=["a", "b"], reverse=[False, True])
    assert E.select_route(1, E.SMALL_MAX) in pl.last_plan(), pl.last_plan()
    same_rows(out, host, words, E.reference([(a[0], None, False, True), (b[0], b[1], True, True)], 90), "bottom_k")
    out = df.top_k(90, by=["b", "a"], reverse=[False, True])
    assert "top_k_select[" in pl.last_plan(), pl.last_plan()
    same_rows(out, host, words, E.reference([(b[0], b[1], True, True), (a[0], None, False, True)], 90), "top_k")


def test_series_top_k_and_bottom_k_with_nulls_and_nans(pl):
    n = E.N1
    v, valid = E.value_table("f64", n), E.VALIDITY["third"](n)
    s = series(pl, "b", v, valid)
    for k in (1, 50, 3000):
        for method, desc in ((s.top_k, True), (s.bottom_k, False)):
            got = method(k)
            assert "top_k_select[" in pl.last_plan(), pl.last_plan()
            rows = E.reference([(v, valid, desc, True)], k)
            values, ok = got._download()
            assert ok is None and valid[rows].all() and np.array_equal(E.bits_of(values), E.bits_of(v[rows])), (k, desc)
    top = s.top_k(10).to_numpy()
    assert np.isnan(top).all()                                                                 # NaN is the greatest value


def test_the_route_text_is_the_sort_s_own(pl):
    """last_plan() after an arg-sort names that sort, whatever an earlier call on the thread left behind.  Every route assertion of this file stands on it.

    Found by this test: Series.arg_sort and arg_sort_by did not clear the plan note that Series.unique() (or a collect() with lowering notes) leaves for last_plan(),
    so after such a call last_plan() kept returning "distinct_mask[...]" instead of the sort's route.  Both now clear the note first (frame.py)."""
    s = series(pl, "a", E.value_table("i32", 300))
    assert len(s.unique().to_numpy()) == len(np.unique(E.value_table("i32", 300)))
    s.arg_sort()
    assert pl.last_plan() == E.rank_route(300, 1), pl.last_plan()
    s.unique()
    pl.arg_sort_by([s, s], [False, True])
    assert pl.last_plan() == E.rank_route(300, 2), pl.last_plan()


# ==================================================================================================== 7. refusals through the C entry point
def test_refusals_leave_the_library_usable(pl):
    from polars_amd import _ffi as F
    a, b = series(pl, "a", np.arange(10, dtype=np.int64)), series(pl, "b", np.arange(11, dtype=np.int64))
    flags = (C.c_uint8 * 2)(0, 0)
    h = C.c_uint64()
    assert F.lib().plx_sort_indices((C.c_uint64 * 2)(a._h, b._h), 2, flags, flags, -1, C.byref(h)) == 5            # PLX_ERR_SHAPE
    assert b"different lengths" in F.lib().plx_last_error()
    assert F.lib().plx_sort_indices((C.c_uint64 * 1)(a._h), 0, flags, flags, -1, C.byref(h)) == 1                  # PLX_ERR_INVALID
    with pytest.raises(pl.PlxError) as e:
        pl.arg_sort_by([a, b])
    assert e.value.code == 5
    check(pl, [(np.arange(10, dtype=np.int64), None, True, False)], "after the refusals")
