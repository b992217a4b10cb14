"""Grouped aggregates at value edges, on every group-by route, against the exact reference of tests/agg_edges.py (checked on the CPU, against the oracle, by
tests/test_agg_edges_cpu.py): NaN, infinities, signed zeros, denormals, the largest finite values, integers at the bounds of their type, wrapping sums, groups
without a valid row, the null key, a group that only the filter's rejected rows hold and one whose surviving rows are all null.

The query is always group_by(keys).agg(sum, mean, min, max, count of the value column; len), unfiltered and behind filter(f > 0), fused and per node
(no_fusion=True).  Every case asserts its route's marker in pl.last_plan() before it compares.  Comparison (agg_edges.compare): the set of groups is the
reference's; validity bit for bit; integers, count, len and the output dtypes equal; float min / max equal as numbers with NaN for NaN -- the sign of a zero is
not compared, because min_ign keeps whichever of -0.0 / +0.0 it met first and the order of the atomics is not fixed; float sum / mean: non-finite expectations
matched in kind, finite ones within RTOL * sum |x| (RTOL = 1e-6, BASELINE.json north_star), Float32 results one f32 ulp more.

What each route reaches:
  lds_table            LdsAggSink: LDS table fill, accumulate with the identity skip, merge of the copies into the HBM cells, finalisers
  dense_hbm_table      init_acc_kernel, HbmAggSink atomics (float min / max: the CAS loops on bit patterns), FIN_MINMAX_F / FIN_MINMAX_I / FIN_TRUNC32 / FIN_NARROW / FIN_MEAN
  hash_hbm_table       HashAggSink: wave pre-aggregation through shfl_xor + agg_combine (clustered layout), then the same atomics; [generic] and [jit] programs
  wide_hash_hbm_table  the same sink behind the wide-key table
  no keys              RegAggSink and partials_finish_kernel
  FusedJoinGroupBy     in place and pair form
  partitioned v2 / v3  part2_agg's LDS tables (hash and direct), the hot list's fill, accumulate and merge; first generation: part_agg (tests/groupby_route_worker.py)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import agg_edges as E
from tests import groupby_route_inputs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = {"lds": "lds_table(", "dense": "dense_hbm_table(", "hash": "]+hash_hbm_table(", "wide": "wide_hash_hbm_table("}
FUSED_TYPES = [d for d in E.NP if d not in ("Float32", "Boolean")]      # Float32 values are aggregated through an f64 view, never fused; Boolean: as the engine routes it
WORST = {}


def note(route, worst):
    WORST[route] = max(WORST.get(route, 0.0), worst)
    print(f"worst relative error [{route}]: {WORST[route]:.3e} (bound {E.RTOL:.0e})")


def series(pl, name, v, ok=None):
    return pl.Series(name, v, validity=ok)


def aggs(pl, dtype, col="v"):
    return [getattr(pl.col(col), op)().alias(op) for op in E.ops_of(dtype) if op != "len"] + [pl.len().alias("len")]


def table_frame(pl, t, route):
    cols = dict(E.key_columns(route, t["gid"])) if route else {}
    cols.update(v=(t["v"], t["valid"]), f=(t["f"], None))
    return pl.DataFrame([series(pl, name, v, ok) for name, (v, ok) in cols.items()]), [c for c in cols if c.startswith("k")]


def runs(pl, lf, dtype, keys, marker, **kw):
    """the query unfiltered and behind the filter, fused and per node -> (filtered, name, downloaded result); the fused plan must hold `marker` (None: not asserted)"""
    for filtered in (False, True):
        src = lf.filter(pl.col("f") > 0) if filtered else lf
        q = src.group_by(*keys).agg(*aggs(pl, dtype)) if keys else src.select(*aggs(pl, dtype))
        for name, more in (("fused", {}), ("per_node", {"no_fusion": True})):
            out = q.collect(**kw, **more)
            plan = pl.last_plan()
            if name == "fused" and marker is not None:
                assert marker in plan, (marker, plan)
            yield filtered, name, R.download(out)


# ---- a. the small routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("dtype", list(E.NP))
@pytest.mark.parametrize("route", E.ROUTES)
def test_small_routes(pl, monkeypatch, route, dtype, layout):
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    t = E.table(dtype, layout)
    df, keys = table_frame(pl, t, route)
    kw = {"no_partition": True} if route == "hash" else {}
    marker = MARKER[route] if dtype in FUSED_TYPES else None
    for filtered, name, got in runs(pl, df.lazy(), dtype, keys, marker, **kw):
        what = (route, dtype, layout, name, "filtered" if filtered else "all rows")
        worst = E.check_groups(got, E.gid_of_keys(route, got), E.table_expected(t, filtered), dtype, what)
        note(MARKER[route].strip("]+("), worst)


# ---- b. no keys: the table as one group ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("dtype", list(E.NP))
def test_no_keys(pl, dtype, layout):
    t = E.table(dtype, layout)
    df, _ = table_frame(pl, t, None)
    marker = "Fused" if dtype in FUSED_TYPES else None
    for filtered, name, got in runs(pl, df.lazy(), dtype, [], marker):
        sel = t["keep"] if filtered else np.ones(t["n"], bool)
        rows = {0: [(v.item(), bool(ok)) for v, ok in zip(t["v"][sel], t["valid"][sel])]}
        want = E.expected(rows, dtype, ("one group", dtype, filtered))          # (the multiset, and with it the exact result, is the same for every layout)
        assert len(got["len"][0]) == 1
        note("no keys", E.check_groups(got, [0], want, dtype, ("no keys", dtype, layout, name, filtered)))


@pytest.mark.parametrize("dtype", ["Float64", "Float32", "Int32", "Int64", "UInt64"])
def test_no_keys_one_edge_kind_at_a_time(pl, dtype):
    """the whole table as one group always holds a NaN and both bounds; here every edge kind is a column of its own, padded with nulls: the scalar path of
    RegAggSink and partials_finish_kernel meets each kind alone"""
    for kind, rows in E.edge_groups(dtype).items():
        rows = [(E.null_payload(dtype), False)] * 70 + rows + [(E.null_payload(dtype), False)] * 200
        v, ok = np.array([r[0] for r in rows], E.NP[dtype]), np.array([r[1] for r in rows], bool)
        df = pl.DataFrame([series(pl, "v", v, ok), series(pl, "f", np.ones(len(v), np.int32))])
        want = E.expected({0: rows}, dtype)
        for filtered, name, got in runs(pl, df.lazy(), dtype, [], "Fused" if dtype in FUSED_TYPES else None):
            note("no keys", E.check_groups(got, [0], want, dtype, ("no keys", dtype, kind, name, filtered)))


# ---- c. the generic interpreter against the run-time compiled program --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["Int64", "Float64"])
def test_generic_interpreter_and_run_time_compiled_program(pl, monkeypatch, dtype):
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    F = pl._ffi
    t = E.table(dtype, "shuffled")
    df, keys = table_frame(pl, t, "hash")
    for filtered in (False, True):
        src = df.lazy().filter(pl.col("f") > 0) if filtered else df.lazy()
        q = src.group_by(*keys).agg(*aggs(pl, dtype))
        generic = q.collect(no_partition=True)
        plan = pl.last_plan()
        assert "[generic]" in plan and MARKER["hash"] in plan, plan
        try:
            F.jit_set_min_rows(0)
            before = F.jit_stats()[0]
            jit = q.collect(no_partition=True)
            plan = pl.last_plan()
            assert "[jit]" in plan and MARKER["hash"] in plan and F.jit_stats()[0] > before, plan
        finally:
            F.jit_set_min_rows(1 << 22)
        for name, out in (("generic", generic), ("jit", jit)):
            got = R.download(out)
            note("hash_hbm_table " + name, E.check_groups(got, E.gid_of_keys("hash", got), E.table_expected(t, filtered), dtype, (name, dtype, filtered)))


# ---- d. join -> group-by, both forms ---------------------------------------------------------------------------------------------------------
def join_runs(pl, q, marker):
    for name, more in (("fused", {}), ("per_node", {"no_fusion": True})):
        out = q.collect(**more)
        plan = pl.last_plan()
        if name == "fused":
            assert marker in plan, (marker, plan)
        yield name, R.download(out)


@pytest.mark.parametrize("dtype", ["Int64", "Float64"])
def test_join_group_by_in_place(pl, monkeypatch, dtype):
    """2^8 build rows with unique keys, ~2^12 probe rows whose value column carries the edge groups, grouped by the join key (the null key's rows find no build row)"""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    t = E.table(dtype, "shuffled", 1 << 12)
    probe, keys = table_frame(pl, t, "hash")
    bk = E.key_values("hash", np.arange(1 << 8))["k"]                      # ids 0..39 are the table's groups, the rest find no probe row
    build = pl.DataFrame([series(pl, "k", bk), series(pl, "c", np.arange(len(bk), dtype=np.float64))])
    for filtered in (False, True):
        src = probe.lazy().filter(pl.col("f") > 0) if filtered else probe.lazy()
        q = src.join(build.lazy(), on="k").group_by("k").agg(*aggs(pl, dtype))
        want = {g: w for g, w in E.table_expected(t, filtered).items() if g != E.NULL_GID}
        for name, got in join_runs(pl, q, "FusedJoinGroupBy{build="):
            note("join in place", E.check_groups(got, E.gid_of_keys("hash", got), want, dtype, ("in place", dtype, name, filtered)))


@pytest.mark.parametrize("dtype", ["Int64", "Float64"])
def test_join_group_by_pair_form(pl, monkeypatch, dtype):
    """~2^8 build rows whose value column carries the edge groups and whose int16 column y is the group; 2^12 probe rows: every build row is found once, the rows
    of the filler groups more often.  The filter is on the build side."""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    t = E.table(dtype, "shuffled", 1 << 8)
    nb = t["n"]
    rng = np.random.default_rng(4)
    bk = R.sparse(rng.permutation(1000)[:nb])
    y = E.key_columns("lds", t["gid"])["k"]
    build = pl.DataFrame([series(pl, "k", bk), series(pl, "y", *y), series(pl, "v", t["v"], t["valid"]), series(pl, "f", t["f"])])
    filler = np.nonzero(np.array([t["kinds"][int(g)] == "filler" for g in t["gid"]]))[0]
    hits = np.concatenate([np.arange(nb), filler[rng.integers(0, len(filler), (1 << 12) - nb)]])
    rng.shuffle(hits)
    probe = pl.DataFrame([series(pl, "k", bk[hits]), series(pl, "w", rng.uniform(0, 1, len(hits)))])
    for filtered in (False, True):
        sel = hits[t["keep"][hits]] if filtered else hits
        rows_of = {}
        for r in sel:
            rows_of.setdefault(int(t["gid"][r]), []).append((t["v"][r].item(), bool(t["valid"][r])))
        want = E.expected(rows_of, dtype)
        b = build.lazy().filter(pl.col("f") > 0) if filtered else build.lazy()
        q = probe.lazy().join(b, on="k").group_by("y").agg(*aggs(pl, dtype))
        for name, got in join_runs(pl, q, "FusedJoinGroupBy{pair form"):
            gids = E.gid_of_keys("lds", {"k": got["y"]})
            note("join pair form", E.check_groups(got, gids, want, dtype, ("pair form", dtype, name, filtered)))


# ---- e. the partitioned routes: 2^24 rows (they start there) -----------------------------------------------------------------------------------
def planted_frame(pl, case):
    return pl.DataFrame([series(pl, "key", *case["key"])] + [series(pl, c, *case[c]) for c in ("v", "x")])


def planted_query(pl, df, col):
    return df.lazy().group_by("key").agg(*[getattr(pl.col(col), op)().alias(op) for op in E.OPS[:-1]], pl.len().alias("len"))


def test_partitioned_hash_with_a_hot_list(pl):
    """the keys of "hot_fits" (one key holds half of the rows, 120 000 groups, 64-bit keys, a null key): the hot key's cells live in the hot list, and they hold
    an all-NaN-but-the-last-row group and a lone INT64_MAX among nulls; 64 more groups carry every other edge kind.  One query per value column."""
    case = E.planted_case("hot_fits")
    df = planted_frame(pl, case)
    for col in ("v", "x"):
        out = planted_query(pl, df, col).collect()
        plan = pl.last_plan()
        print(f"plan[hot_fits {col}]: {plan}")
        assert re.search(r"partitioned\(v[23],hash", plan) and re.search(r"hot=[1-9]", plan) and "hbm_table" not in plan, plan
        note("partitioned hash + hot list", E.check_planted(R.download(out), case, col, ("hot_fits", col)))


def test_partitioned_direct_after_the_key_range_is_learned(pl, monkeypatch):
    """the keys of "learned": the first run learns the key range (hash partitions), the second takes the direct-address tables"""
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    case = E.planted_case("learned")
    df = planted_frame(pl, case)
    for col in ("v", "x"):
        for attempt in ("first run", "second run"):
            out = planted_query(pl, df, col).collect()
            plan = pl.last_plan()
            print(f"plan[learned {col} {attempt}]: {plan}")
            if attempt == "second run":
                assert re.search(r"partitioned\(v3,direct", plan), plan
            elif col == "v":
                assert re.search(r"partitioned\(v[23],hash", plan) and "key_range_learned" in plan, plan
            else:                                                           # (the range is the frame's: the second column's first run may already have it)
                assert re.search(r"partitioned\(v[23],(hash|direct)", plan), plan
            route = "partitioned hash" if "hash" in re.search(r"partitioned\(v[23],(\w+)", plan).group(1) else "partitioned direct"
            note(route, E.check_planted(R.download(out), case, col, ("learned", col, attempt)))


# ---- f. the first-generation kernels -----------------------------------------------------------------------------------------------------------
def test_first_generation_partition_kernels_at_value_edges():
    e = dict(os.environ)
    e["PLX_PART_V"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "groupby_route_worker.py"), "v1_edges"], capture_output=True, text=True, timeout=240, cwd=ROOT, env=e)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-1500:], r.stderr[-2500:])
