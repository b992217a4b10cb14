"""Pins tests/sort_edges.py without a GPU: the two forms of the reference (the vectorised sort_indices and the pure-Python restatement of the reference comparator)
agree on every table small enough for the latter, every top-k table's stated candidate count equals a direct count over the first key's codes, every table has the
property it is named for, and the restated geometry still matches kernels_sort.hip."""
import functools
import os
import re

import numpy as np
import pytest

from tests import sort_edges as E

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "polars_amd", "csrc")
DIRECTIONS = [(d, nl) for d in (False, True) for nl in (False, True)]


def both_forms(orc, keys, what):
    a, b = orc.sort_indices(keys), orc.sort_indices_cmp(keys)
    assert a.dtype == np.uint32 and np.array_equal(a, b), (what, np.flatnonzero(a != b)[:8])


# ------------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("dt", E.DTYPES)
def test_both_forms_of_the_reference_agree_on_the_value_tables(orc, dt):
    """negative and payload NaNs, float32 denormals, u64 above 2^63, the integer extremes, -0 / +0 ties, under every validity pattern, direction and null placement"""
    n = 1500
    v = E.value_table(dt, n)
    for vname, vf in E.VALIDITY.items():
        for d, nl in DIRECTIONS:
            both_forms(orc, [(v, vf(n), d, nl)], (dt, vname, d, nl))
    both_forms(orc, [(v, E.VALIDITY["third"](n), True, False), (E.second_key(n), None, False, False)], (dt, "two keys"))


@pytest.mark.parametrize("d", range(8))
def test_both_forms_of_the_reference_agree_on_the_digit_and_tile_tables(orc, d):
    n = E.TILE + 1
    for variant in E.DIGIT_VARIANTS:
        for signed in (False, True):
            both_forms(orc, [(E.digit_keys(d, n, variant, signed), None, signed, False)], (d, variant, signed))
    if d in (0, 7):
        for name, p in E.tile_patterns(n).items():
            both_forms(orc, [(E.second_key(n) % 3, None, False, False), (E.place_digit(p, d, signed=d == 7), None, False, False)], (d, name))


# ------------------------------------------------------------------------------------------------------------------ top-k tables
@functools.lru_cache(maxsize=None)
def full_order(name):
    return E.reference(E.topk_case(name)["keys"])


def at_or_below(codes, order, limit, shift):
    """rows whose first-key code, cut to the digits above `shift`, is at or below the limit-th row's: the class the selection keeps after the round at `shift`"""
    s = np.uint64(shift)
    return int(((codes >> s) <= (codes[order[limit - 1]] >> s)).sum())


@pytest.mark.parametrize("name", [c["name"] for c in E.topk_tables()])
def test_topk_tables_state_the_candidate_class(name):
    case = E.topk_case(name)
    keys = case["keys"]
    n = len(keys[0][0])
    codes = E.select_codes(keys[0])
    order = full_order(name)
    for limit, rounds, cand in case["picks"]:
        if not E.selects(n, limit):
            assert rounds == 0 and cand is None, (name, limit)
            continue
        assert 1 <= rounds <= 8, (name, limit)
        shift = 8 * (8 - rounds)
        good_enough = max(2 * limit, E.SMALL_MAX)
        count = at_or_below(codes, order, limit, shift)
        assert count <= good_enough or shift == 0, (name, limit, count)                         # the walk stops at this round ...
        for earlier in range(shift + 8, 64, 8):
            assert at_or_below(codes, order, limit, earlier) > good_enough, (name, limit, earlier)    # ... and at none before it
        if cand is None:
            assert count >= n // E.SELECT_KEEP_DIV, (name, limit, count)
        else:
            assert count == cand and count < n // E.SELECT_KEEP_DIV, (name, limit, count, cand)


def test_topk_tables_hold_the_cases_they_are_named_for():
    names = [c["name"] for c in E.topk_tables()]
    assert len(set(names)) == len(names)
    n = E.N1
    k = E.topk_case("one_round_2048")["keys"][0][0]
    small = np.flatnonzero(k < (1 << 56))
    assert len(small) == E.SMALL_MAX and small[0] == 0 and small[-1] == n - 1 and len(np.unique(k[small])) == E.SMALL_MAX and (k[k >= E.SMALL_MAX] >= (1 << 56)).all()
    assert len(E.topk_case("one_round_2048_three_strides")["keys"][0][0]) == E.N3 == 3 * 65536 + 1
    k = E.topk_case("tied_5000")["keys"][0][0]
    assert int((k == k.min()).sum()) == 5000 and k[0] == k.min() and k[-1] == k.min()
    assert [c for c in names if c.startswith("tied_3")] == ["tied_%d" % t for t in (n // 2 + 1, n // 2, n // 2 - 1)]
    for z, mins in ((50, 30), (3000, 30)):
        k, valid, _, nl = E.topk_case("nulls_first_z%d_min%d" % (z, mins))["keys"][0]
        assert not nl and int((~valid).sum()) == z and int(((k == np.iinfo(np.int64).min) & valid).sum()) == mins
        codes = E.select_codes((k, valid, False, False))
        assert int((codes == 0).sum()) == z + mins                                               # the tie the case is about
    for name, desc, edge, all_ones in (("u64_max", False, 2 ** 64 - 1, True), ("u8_255", False, 255, False), ("u32_zero_desc", True, 0, True)):
        key = E.topk_case("nulls_last_" + name)["keys"][0]
        codes = E.select_codes(key)
        assert key[3] and int(key[1].sum()) == 40 < 100 and key[2] == desc and int(((key[0] == edge) & key[1]).sum()) == 5
        assert codes[key[1]].max() == codes[(key[0] == edge) & key[1]].min()                         # the edge value ends the valid rows ...
        assert bool((codes[(key[0] == edge) & key[1]] == np.uint64(2 ** 64 - 1)).all()) == all_ones  # ... on the nulls' own code (not for u8: 255 is code 255)
    for dt in E.FLOATS:
        v = E.topk_case("dtype_%s_desc" % dt)["keys"][0][0]
        assert set(E.bits_of(v[np.isnan(v)]).tolist()) == set(E.NAN_BITS[dt]) and np.isinf(v).sum() == 2 * E.EXTREME_REPEAT
        assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    for dt in E.DTYPES:
        if dt != "bool" and dt not in E.FLOATS:
            v = E.topk_case("dtype_%s_asc" % dt)["keys"][0][0]
            assert v.dtype == E.NP[dt] and int((v == np.iinfo(v.dtype).min).sum()) == E.EXTREME_REPEAT == int((v == np.iinfo(v.dtype).max).sum())


# ---------------------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("dt", E.DTYPES)
def test_value_tables_hold_the_edges(dt):
    base = E.base_values(dt)
    for n in (len(base), 1500, E.SMALL_MAX + 1, E.TILE + 257):
        v = E.value_table(dt, n)
        assert v.dtype == E.NP[dt] and len(v) == n
        assert set(E.bits_of(v).tolist()) == set(E.bits_of(base).tolist()), (dt, n)               # every edge, bit for bit (the three NaNs stay three)
        assert (v[1:] != v[:-1]).any()
    if dt == "bool":
        return
    w = E.width(dt)
    pairs = E.bits_of(E.byte_pairs(dt)).astype(np.uint64)
    for d in range(w):
        assert int(pairs[2 * d] ^ pairs[2 * d + 1]) & ~(0xff << (8 * d)) == 0 and pairs[2 * d] != pairs[2 * d + 1]
    if dt in E.FLOATS:
        t, fi = E.NP[dt], np.finfo(E.NP[dt])
        denorm = np.nextafter(t(0), t(1))
        for x in (fi.max, -fi.max, fi.tiny, -fi.tiny, denorm, -denorm, t(2.0 ** -149), t(-2.0 ** -149), t(np.inf), t(-np.inf)):
            assert x in base, (dt, x)
        zeros = base[base == 0]
        assert len(zeros) == 5 and int(np.signbit(zeros).sum()) == 2                               # 0 of "min .. max", and -0 / +0 twice each
        assert set(E.bits_of(base[np.isnan(base)]).tolist()) == set(E.NAN_BITS[dt]) and np.isfinite(E.byte_pairs(dt)).all()
        assert denorm > 0 and t(2.0 ** -149) > 0
    else:
        ii = np.iinfo(E.NP[dt])
        for x in (ii.min, ii.min + 1, 0, 1, ii.max - 1, ii.max) + ((-1,) if ii.min < 0 else ()):
            assert x in base.tolist(), (dt, x)


def test_validity_patterns():
    assert list(E.VALIDITY) == ["none", "third", "walk", "all_null", "one_valid", "words"]
    for n in (1500, E.SMALL_MAX + 1, E.TILE + 257):
        assert E.VALIDITY["none"](n) is None
        assert int(E.VALIDITY["third"](n).sum()) == n - len(range(2, n, 3))
        walk = E.VALIDITY["walk"](n)
        for w in range((n + 63) // 64):
            word = walk[64 * w:64 * w + 64]
            row = (7 * w) % 64
            assert int(word.sum()) == (1 if row < len(word) else 0) and (row >= len(word) or word[row])
        assert not E.VALIDITY["all_null"](n).any() and int(E.VALIDITY["one_valid"](n).sum()) == 1
        words = E.VALIDITY["words"](n)
        assert words[:64].all() and not words[64:128].any() and words[128:192].all()


@pytest.mark.parametrize("d", range(8))
def test_digit_tables_differ_in_one_byte_only(d):
    n = E.TILE + 257
    others = ~(0xff << (8 * d)) & (2 ** 64 - 1)
    for signed in (False, True):
        a = E.digit_keys(d, n, "all256", signed)
        assert a.dtype == (np.int64 if signed else np.uint64)
        u = a.view(np.uint64)
        assert len(np.unique(u & np.uint64(others))) == 1 and len(np.unique((u >> np.uint64(8 * d)) & np.uint64(255))) == 256
        u = E.digit_keys(d, n, "two", signed).view(np.uint64)
        vals, counts = np.unique((u >> np.uint64(8 * d)) & np.uint64(255), return_counts=True)
        assert len(np.unique(u & np.uint64(others))) == 1 and len(vals) == 2 and sorted(counts.tolist()) == [255, n - 255]


def test_tile_patterns_are_what_they_are_named_for():
    n = 2 * E.TILE + 65
    p = E.tile_patterns(n)
    assert set(p) == {"sorted", "reversed", "groups", "tile_constant", "sixteen_each"} | {"saw%d" % k for k in E.SAW_PERIODS}
    assert all(v.dtype == np.uint8 and len(v) == n for v in p.values())
    assert (np.diff(p["sorted"].astype(int)) >= 0).all() and (np.diff(p["reversed"].astype(int)) <= 0).all() and len(np.unique(p["sorted"])) == 256
    for k in E.SAW_PERIODS:
        s = p["saw%d" % k].astype(int)
        assert np.array_equal(s[k:], s[:-k]) and len(np.unique(s[:k])) == min(k, 256)
    for w in range(n // 64):                      # match-any groups of every size from 1 to 64 in every whole tile, the other lanes alone with their value
        counts = np.bincount(p["groups"][64 * w:64 * w + 64], minlength=256)
        assert sorted(counts[counts > 0].tolist()) == sorted([1] * (63 - w % 64) + [w % 64 + 1]), w
    c = p["tile_constant"]
    assert len(np.unique(c[:E.TILE])) == 1 and len(np.unique(c[E.TILE:2 * E.TILE])) > 200 and len(np.unique(c[2 * E.TILE:])) == 1 and c[0] != c[-1]
    for t in range(2):
        assert np.bincount(p["sixteen_each"][t * E.TILE:(t + 1) * E.TILE], minlength=256).tolist() == [16] * 256
    for t in range(n // 64):                      # ... and inside a wave a value comes four times: the uint8 counts and uint16 prefixes add up over 16 sub-tiles
        assert set(np.bincount(p["sixteen_each"][64 * t:64 * t + 64], minlength=256).tolist()) <= {0, 4}
    k = E.place_digit(p["sorted"], 7, signed=True)
    assert k.dtype == np.int64 and (k < 0).any() and (k > 0).any()


# -------------------------------------------------------------------------------------------------------------------- the geometry
def test_restated_constants_match_the_source():
    """a change of the sort's geometry fails here instead of silently moving the edges away from the tests"""
    src = open(os.path.join(CSRC, "kernels_sort.hip")).read()
    cfg = open(os.path.join(CSRC, "kconfig.hpp")).read()

    def const(text, name):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m, name
        return int(m.group(1))
    assert const(cfg, "kBlock") == E.BLOCK and "using k::kBlock;" in src
    assert const(src, "kItems") == E.ITEMS and "constexpr int kTile = kBlock * kItems;" in src and E.TILE == E.BLOCK * E.ITEMS
    assert const(src, "kIPT") == E.IPT and E.ROUND == E.IPT * E.BLOCK and "kIPT * kBlock keys" in src
    assert const(src, "kSmallBlock") == E.SMALL_BLOCK and const(src, "kSmallMax") == E.SMALL_MAX and const(src, "kSmallMaxKeys") == E.SMALL_MAX_KEYS
    assert "if (m <= kSmallMax && (int)keys.size() <= kSmallMaxKeys)" in src
    assert "if (limit >= 0 && limit < n / %d && n > %d)" % (E.SELECT_LIMIT_DIV, E.SELECT_MIN_ROWS) in src
    assert "if (cand_rows < (uint64_t)n / %d)" % E.SELECT_KEEP_DIV in src
    assert "std::max<uint64_t>(2 * (uint64_t)limit, (uint64_t)kSmallMax)" in src and "if (c + h[b] >= need) break;" in src
    assert E.selects(E.N1, E.N1 // 4 - 1) and not E.selects(E.N1, E.N1 // 4) and not E.selects(E.SELECT_MIN_ROWS, 10) and not E.selects(E.N1, -1)
