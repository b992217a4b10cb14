"""Every recovery branch of the hash-join build (engine.cpp HashBuild::run), driven on purpose through both fused join routes (join -> group-by: FusedJoinGroupBy,
join -> frame: FusedJoinFrame, inner and left): a sample that was right, a sampled table that came out too full, sampled tables that overflowed (windowed and plain), a
crowded window on a rightly sized table, duplicate keys found by the windowed build, and a misjudged sample together with duplicates.  tests/join_build_inputs.py builds
each case and carries the numpy reference; tests/test_join_build_inputs_cpu.py proves on the CPU that each input has the properties that select its branch.  Here the
plan text proves that the branch ran (resized(overflow,from=2^N)+ | resized(load,from=2^N)+ | windowed-off+ | chained+ in front of the build's description, and the
table's final cap=2^N, both taken from the CPU module's arithmetic) and EVERY pair / group is compared with the reference, exactly: all values are integers.

A rebuilt table that kept state of the attempt it replaces, lost rows, or chained rows twice changes a pair or a per-group len / sum."""
import re

import numpy as np
import pytest

import join_build_inputs as J

pytestmark = pytest.mark.gpu

MARKERS = ("resized(overflow,", "resized(load,", "windowed-off+", "chained+")
# case -> (the markers of its retries, which sizing gives the final cap, multi-value)
EXPECT = {
    "sample_right": ((), "first", False),
    "sample_load": (("resized(load,",), "exact", False),
    "sample_overflow_windowed": (("resized(overflow,",), "exact", False),
    "sample_sees_nothing": (("resized(overflow,",), "exact", False),
    "crowded_window": (("windowed-off+",), "first", False),
    "windowed_finds_duplicates": (("chained+",), "first", True),
    "misjudged_and_duplicates": (("resized(overflow,", "chained+"), "exact", True),
}
_cases = {}


def case_of(name):
    """the case, its sizing and its reference, computed once and left unchanged"""
    if name not in _cases:
        c = J.build(name)
        p, b, unmatched = J.pairs(c)
        _cases[name] = (c, J.sizing(c), {"pairs": J.sort_pairs(p, b), "unmatched": unmatched, "groups": J.group_rows(c["pk"][p], c["a"][b], c["x"][p])})
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def release_inputs():
    """the cases hold a few GB of host arrays: gone when the module is done"""
    yield
    _cases.clear()
    J.large_shared.cache_clear()


def set_env(monkeypatch, c):
    if c["part_build"]:
        monkeypatch.setenv("PLX_JOIN_PART_BUILD", c["part_build"])      # read at every build
        monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")                # the join -> frame route at fewer than 2^24 probe rows


def build_text(plan):
    m = re.search(r"hash table cap=2\^(\d+)(?: \[([^\]]*)\])?", plan)
    assert m, plan
    return int(m.group(1)), m.group(2) or ""


def check_plan(plan, name, route, known_duplicates=False):
    c, z, _ = case_of(name)
    markers, cap_from, multi = EXPECT[name]
    assert ("FusedJoinGroupBy{" if route == "group_by" else "FusedJoinFrame{") in plan and "hash table cap=" in plan, plan
    cap, how = build_text(plan)
    if known_duplicates:                                  # the column remembers that its keys repeat: chains from the first attempt, nothing found during this run
        markers = tuple(m for m in markers if m != "chained+")
    for m in MARKERS:
        assert how.count(m) == (1 if m in markers else 0), (m, plan)
    if any(m.startswith("resized(") for m in markers):
        assert f"from=2^{z['first']})+" in how, plan
    assert cap == z[cap_from], (cap, z, plan)
    assert ("multi-value" in plan) == multi and ("unique-keys" in plan) == (not multi), plan
    # the build that produced the table: windowed unless the keys repeat or the windowed build was switched off
    assert ("partitioned build(" in how) == (J.windowed(c, cap) and not multi and "windowed-off+" not in markers), plan
    if route == "group_by":
        assert ("join_build" in how) == ("partitioned build(" not in how), plan
    rest = re.sub(r"^(?:resized\((?:overflow|load),from=2\^\d+\)\+|windowed-off\+|chained\+)*", "", how)
    assert not any(m in rest for m in MARKERS), plan      # the markers come first, the build's own description after them


def check_groups(out, name):
    k, a, sx, n = case_of(name)[2]["groups"]
    assert out.height == len(k), (out.height, len(k))
    gk, ga, gs, gn = (np.asarray(out[col].to_numpy()) for col in ("k", "a", "sx", "n"))
    assert gs.dtype == np.int64
    o = np.lexsort((ga, gk))
    assert np.array_equal(gk[o], k) and np.array_equal(ga[o], a), "the groups (key, build attribute) are not those of the reference"
    assert np.array_equal(gn[o].astype(np.int64), n), "len"
    assert np.array_equal(gs[o], sx), "sum"


def check_pairs(out, name, how):
    c, _, ref = case_of(name)
    want_p, want_b = ref["pairs"]
    lr = np.asarray(out["lr"].to_numpy())
    rr, ok = out["rr"]._download()
    ok = np.ones(len(rr), bool) if ok is None else np.asarray(ok, bool)
    if how == "inner":
        assert bool(ok.all()) and out.height == len(want_p), (out.height, len(want_p))
    else:   # a left join keeps every probe row without a match, once, with a null build side
        assert out.height == len(want_p) + len(ref["unmatched"]), (out.height, len(want_p), len(ref["unmatched"]))
        alone = np.zeros(len(c["pk"]), np.int64)
        alone[ref["unmatched"]] = 1
        assert np.array_equal(np.bincount(lr[~ok], minlength=len(alone)), alone), "unmatched probe rows"
    got_p, got_b = J.sort_pairs(lr[ok], np.asarray(rr)[ok])
    assert np.array_equal(got_p, want_p) and np.array_equal(got_b, want_b), "the (probe row, build row) pairs are not those of the reference"


@pytest.mark.parametrize("name", J.CASES)
def test_join_group_by_route(pl, monkeypatch, name):
    """L.join(R.filter(s != 0), on=k).group_by(k, a).agg(x.sum(), len).  Two library-owned columns allocated just before the join keep their bytes (a sanity check of the
    pool around a windowed build whose first table was too small for the rows that pass -- cases 3 and 7; the bound itself is in join_fill_kernel)."""
    c, _, _ = case_of(name)
    set_env(monkeypatch, c)
    L, R = J.frames(pl, c)
    g = np.arange(1 << 20, dtype=np.int64) * 0x9E3779B97F4A7C1
    guard = pl.DataFrame({"g0": g, "g1": ~g})
    out = J.group_by_query(pl, L, R).collect()
    plan = pl.last_plan()
    print(f"plan[{name}]: {plan}")
    check_plan(plan, name, "group_by")
    check_groups(out, name)
    assert np.asarray(guard["g0"].to_numpy()).tobytes() == g.tobytes() and np.asarray(guard["g1"].to_numpy()).tobytes() == (~g).tobytes()
    if name == "windowed_finds_duplicates":
        # the same frames again: the key column knows that it repeats, the build starts chained -- and gives the same groups
        out2 = J.group_by_query(pl, L, R).collect()
        plan2 = pl.last_plan()
        check_plan(plan2, name, "group_by", known_duplicates=True)
        check_groups(out2, name)


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("name", J.CASES)
def test_join_frame_route(pl, monkeypatch, name, how):
    """The same join collected as a frame of row numbers (lr of L, rr of R): the multiset of pairs.  Left: R builds whatever the lengths, unmatched probe rows carry nulls."""
    c, _, _ = case_of(name)
    set_env(monkeypatch, c)
    L, R = J.frames(pl, c)
    out = J.frame_query(pl, L, R, how).collect()
    plan = pl.last_plan()
    print(f"plan[{name},{how}]: {plan}")
    check_plan(plan, name, "frame")
    check_pairs(out, name, how)
    if name == "windowed_finds_duplicates" and how == "inner":
        out2 = J.frame_query(pl, L, R, how).collect()
        check_plan(pl.last_plan(), name, "frame", known_duplicates=True)
        check_pairs(out2, name, how)


@pytest.mark.parametrize("name", ["sample_overflow_windowed", "misjudged_and_duplicates"])
def test_two_runs_on_fresh_frames_print_the_same_plan(pl, name):
    """Which of the two an overflowed first attempt notices -- the overflow alone, or two rows of a key as well -- is not determined; the plan text is."""
    c, _, _ = case_of(name)
    plans = []
    for _ in range(2):
        L, R = J.frames(pl, c)
        J.group_by_query(pl, L, R).collect()
        plans.append(pl.last_plan())
    assert plans[0] == plans[1], plans
