"""The inputs of the hash-join build recovery tests (tests/join_build_inputs.py) have the properties that send HashBuild::run (engine.cpp) down each of its branches --
computed here from the builders alone, next to the sizing arithmetic each property follows from -- and the numpy reference agrees with a row-by-row join.  No GPU."""
import numpy as np
import pytest

import join_build_inputs as J


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(name):
        if name not in built:
            built[name] = J.build(name)
        return built[name]
    return get


def test_sizing_arithmetic_known_values():
    # sample blocks at b * ((H / 4) & ~127), 2^18 rows each
    r = J.sample_rows(J.H)
    assert len(r) == 4 << 18 and [int(r[b << 18]) for b in range(4)] == [0, 1 << 22, 2 << 22, 3 << 22] and int(r[-1]) == (3 << 22) + (1 << 18) - 1
    n = 17_000_003
    r = J.sample_rows(n)
    assert int(r[1 << 18]) == (n // 4) & ~127 and int(r[1 << 18]) % 128 == 0 and len(r) == 4 << 18
    # est = hits / seen * H * 1.25 + 4096
    keep = np.zeros(J.H, bool)
    assert J.sampled_estimate(keep) == (0, 1 << 20, 4096)
    keep[: 1 << 17] = True                                     # half of the first block: 1/8 of the sampled rows
    assert J.sampled_estimate(keep) == (1 << 17, 1 << 20, (J.H >> 3) * 5 // 4 + 4096)
    # log2_cap = max(min, ceil_log2(x * 1.6)) from a sample, x * 2.0 from an exact count
    assert [J.ceil_log2(x) for x in (0, 1, 2, 3, 4, 5, 1 << 20, (1 << 20) + 1)] == [0, 0, 1, 2, 2, 3, 20, 21]
    assert J.log2_cap(4096, True, 4) == 13 and J.log2_cap(4096, True, 8) == 13 and J.log2_cap(0, False, 4) == 4 and J.log2_cap(0, False, 8) == 8
    assert J.log2_cap(1 << 20, False, 4) == 21 and J.log2_cap((1 << 20) + 1, False, 4) == 22 and J.log2_cap(1 << 20, True, 4) == 21 and J.log2_cap(1_310_721, True, 4) == 22
    # window of a key = (key * 0x55fbfd6bfc5458e9 mod 2^64) >> (64 - (log2_cap - 13))
    keys = np.array([1, -1, 12345678901234567, -(1 << 63)], np.int64)
    for cap in (21, 22, 27):
        want = [((int(k) & J.M64) * 0x55FBFD6BFC5458E9 & J.M64) >> (64 - (cap - 13)) for k in keys]
        assert J.window_of(keys, cap).tolist() == want and max(want) < 1 << (cap - 13)
    # the windowed build only for log2_cap >= 21; by default only for build sides of >= 2^24 rows
    big, small = {"part_build": None, "rk": np.zeros(1 << 24, np.int8)}, {"part_build": None, "rk": np.zeros(1000, np.int8)}
    assert J.windowed(big, 21) and not J.windowed(big, 20) and not J.windowed(small, 22)
    assert J.windowed(dict(small, part_build="2"), 21) and not J.windowed(dict(small, part_build="2"), 20) and not J.windowed(dict(big, part_build="0"), 24)


def test_reference_agrees_with_a_row_loop():
    rng = np.random.default_rng(3)
    nb, n = 400, 3000
    rk = rng.integers(0, 300, nb).astype(np.int64)             # keys repeat, up to several times
    case = {"rk": rk, "s": (rng.random(nb) < 0.7).astype(np.int8), "a": rng.integers(0, 3, nb).astype(np.int64), "pk": rng.integers(0, 400, n).astype(np.int64),
            "x": rng.integers(-50, 50, n).astype(np.int64)}
    case["order"], case["porder"] = np.argsort(rk, kind="stable"), np.argsort(case["pk"], kind="stable")
    want, unmatched, table = [], [], {}
    for b in range(nb):
        if case["s"][b]:
            table.setdefault(int(rk[b]), []).append(b)
    for p in range(n):
        rows = table.get(int(case["pk"][p]), [])
        want += [(p, b) for b in rows]
        if not rows:
            unmatched.append(p)
    p, b, un = J.pairs(case)
    sp, sb = J.sort_pairs(p, b)
    assert list(zip(sp.tolist(), sb.tolist())) == sorted(want) and sorted(un.tolist()) == unmatched and len(want) > len({p_ for p_, _ in want}) > 0      # some probe rows match several build rows
    agg = {}
    for p_, b_ in want:
        g = agg.setdefault((int(case["pk"][p_]), int(case["a"][b_])), [0, 0])
        g[0] += int(case["x"][p_]); g[1] += 1
    k, a, sx, cnt = J.groups(case)
    assert list(zip(k.tolist(), a.tolist())) == sorted(agg) and [agg[key] for key in sorted(agg)] == [[s_, c_] for s_, c_ in zip(sx.tolist(), cnt.tolist())]


@pytest.mark.parametrize("name", J.CASES)
def test_every_case_is_a_hash_table_build_of_hashed_keys(cases, name):
    c = cases(name)
    n = len(c["rk"])
    assert n == (J.H_SMALL if c["part_build"] else J.H) and len(c["pk"]) == (J.N_PROBE_SMALL if c["part_build"] else J.N_PROBE) and len(c["pk"]) > n      # R builds an inner join
    assert c["s"].dtype == np.int8 and c["a"].dtype == np.int64 and c["rk"].dtype == np.int64 and c["x"].dtype == np.int64
    # the keys are id * odd constant mod 2^64, as in tests/test_gpu_join_partitioned.py
    assert J.HASH_MULT % 2 == 1 and np.array_equal(c["rk"], J.hashed(c["rid"]))
    # DirectBuild::try_build: a key range above 256 x the build rows is not eligible for the direct-address table
    assert int(c["rk"].max()) - int(c["rk"].min()) + 1 > 256 * n
    # the build rows' keys are distinct except where the case plants second rows
    sk = c["rk"][c["order"]]
    assert bool(np.all(sk[1:] >= sk[:-1]))
    if name in ("windowed_finds_duplicates", "misjudged_and_duplicates"):
        assert bool(np.any(sk[1:] == sk[:-1])) and bool(np.all(sk[2:] != sk[:-2]))       # each key occurs at most twice
    else:
        assert bool(np.all(sk[1:] != sk[:-1]))
    # about 5 % of the probe rows hit a surviving build row
    p, _, un = J.pairs(c)
    hits = len(c["pk"]) - len(un)
    assert 0.01 * len(c["pk"]) < hits < 0.09 * len(c["pk"]) and len(p) >= hits
    for route in ("group_by", "frame"):
        assert J.sizing(c, route) == J.sizing(c, "group_by")        # every table here is above both callers' minimum size


def no_window_overflows(c, cap):
    return int(J.window_fills(J.survivors(c)[0], cap).max()) <= J.WINDOW


def test_sample_right(cases):
    c = cases("sample_right")
    z = J.sizing(c)
    hits, seen, est = J.sampled_estimate(c["s"] != 0)
    assert z["sampled"] and seen == 1 << 20 and z["first"] == J.log2_cap(est, True, 4) == 24        # the cap follows from the sampled rows alone
    assert z["load"] <= 0.7 and J.windowed(c, z["first"]) and no_window_overflows(c, z["first"])      # neither a resize nor a crowded window


def test_sample_load(cases):
    c = cases("sample_load")
    z = J.sizing(c)
    assert z["sampled"] and z["first"] == 23 and z["load"] > 0.7 and z["exact"] == 24
    assert J.windowed(c, 23) and no_window_overflows(c, 23)                                          # every window's fill <= 8192: the overflow branch is not taken
    assert J.windowed(c, 24) and no_window_overflows(c, 24)


def test_sample_overflow_windowed(cases):
    c = cases("sample_overflow_windowed")
    z = J.sizing(c)
    assert z["sampled"] and z["first"] == 22 and J.windowed(c, 22) and z["exact"] == 25
    assert z["passing"] > (1 << 22) + 1                       # more records than the cells hold: cell_key / cell_row have cap + 1 entries
    assert not no_window_overflows(c, 22) and J.windowed(c, 25) and no_window_overflows(c, 25)


def test_sample_sees_nothing(cases):
    c = cases("sample_sees_nothing")
    z = J.sizing(c)
    assert J.sampled_estimate(c["s"] != 0)[0] == 0 and z["first"] == 13 and not J.windowed(c, 13)      # a plain build into 8192 slots
    assert 2_900_000 < z["passing"] < 3_100_000 and z["passing"] > 1 << 13 and z["exact"] >= 21
    keep = np.nonzero(c["s"] != 0)[0]
    assert int(keep[-1]) - int(keep[0]) + 1 == len(keep) and (1 << 18) <= int(keep[0]) and int(keep[-1]) < 1 << 22     # one run, between two sample blocks
    assert J.windowed(c, z["exact"]) and no_window_overflows(c, z["exact"])


def test_crowded_window(cases):
    c = cases("crowded_window")
    z = J.sizing(c)
    assert not z["sampled"] and z["first"] == z["exact"] == 22 and J.windowed(c, 22)
    fills = np.sort(J.window_fills(J.survivors(c)[0], 22))
    assert J.WINDOW < int(fills[-1]) <= 2 * J.WINDOW and int(fills[-2]) < J.WINDOW                      # one window overflows; the plain table's runs stay far below 65 536
    assert 2 * J.WINDOW < J.PROBE_LIMIT // 2
    crowded = c["rk"][c["crowded_rows"]]
    assert len(crowded) == 9000 and bool(np.all(c["s"][c["crowded_rows"]] != 0))
    assert len(np.unique(J.mul64(crowded, J.TABLE_MULT).view(np.uint64) >> np.uint64(50))) == 1         # their table hashes share the top 14 bits
    assert np.isin(c["pk"], crowded).sum() > 100                                                     # and probe rows look for them


def test_windowed_finds_duplicates(cases):
    c = cases("windowed_finds_duplicates")
    z = J.sizing(c)
    assert not z["sampled"] and z["first"] == z["exact"] == 22 and J.windowed(c, 22) and no_window_overflows(c, 22)
    sk, rows = J.survivors(c)
    twice = sk[1:][sk[1:] == sk[:-1]]
    assert 11_000 < len(twice) < 13_000                       # duplicates among the passing rows, about 1 % of the keys
    assert int(np.count_nonzero(sk == -1)) == 2 and int(np.count_nonzero(c["pk"] == -1)) >= 2            # the EMPTY pattern, twice, and looked for
    same = c["a"][rows[1:]][sk[1:] == sk[:-1]] == c["a"][rows[:-1]][sk[1:] == sk[:-1]]
    assert same.any() and not same.all()                      # rows of a key that are one group, and rows that are two
    assert np.isin(c["pk"], twice).sum() > 100


def test_misjudged_and_duplicates(cases):
    c = cases("misjudged_and_duplicates")
    z = J.sizing(c)
    assert z["sampled"] and z["first"] == 22 and J.windowed(c, 22) and z["exact"] == 25 and z["passing"] > (1 << 22) + 1
    assert np.array_equal(c["s"], cases("sample_overflow_windowed")["s"])
    sk, _ = J.survivors(c)
    twice = sk[1:][sk[1:] == sk[:-1]]
    assert len(twice) == 1000 and np.isin(c["pk"], twice).sum() > 10
