"""Every route of the fused group-by driver (engine.cpp run_fused_groupby: lds_table, partitioned_packed_ids, dense_hbm_table, size_hash_table,
partitioned_wide_keys, partitioned_single_key, hash_hbm_table, partitioned_v1 / partitioned_v2 behind them), driven on purpose: each case builds an input whose
properties -- checked on the CPU by tests/test_groupby_route_inputs_cpu.py, next to the planner arithmetic they come from -- make the planner take one route, proves
from pl.last_plan() that it did, and compares EVERY group with the numpy reference of tests/groupby_route_inputs.py: the key tuples (the null group included) are
the same set, integer aggregates / count / len are exact, float aggregates within RTOL = 1e-6.  The retries after an overflow re-run a pass over all rows: a
retry that double-counted, kept state of the failed attempt or put rows into the wrong group changes a signed per-group sum.

Every planned case is here; none turned out to be unreachable through the Python API.  Where a case asserts a partition count or a number of retries, the CPU
test derives it from the input; where it does not, only the marker is asserted.

The first-generation kernels (PLX_PART_V=1, read once per process) run in tests/groupby_route_worker.py, one fresh child process per case."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import groupby_route_inputs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V23 = r"partitioned\(v[23],"


def run(pl, case, df=None, **kw):
    df = R.frame(pl, case) if df is None else df
    out = R.query(pl, df.lazy(), case).collect(**kw)
    plan = pl.last_plan()
    print(f"plan[{case.get('name', '')}]: {plan}")
    return out, plan, df


def check(out, case, what=""):
    R.assert_groups_equal(R.download(out), R.case_reference(case), case["keys"], what)


def parts(plan):
    """P of the partitioned pass that produced the result"""
    return int(re.search(V23 + r"(?:hash|direct),P=(\d+),", plan).group(1))


@pytest.mark.parametrize("name", ["dense_flag", "dense_small"])
def test_dense_hbm_table(pl, name):
    """Case 1.  A 15-bit packed id (a nullable key column, a nullable value): >= 2^24 rows with no_partition, and fewer rows without the flag."""
    case = R.build(name)
    out, plan, _ = run(pl, case, no_partition=(name == "dense_flag"))
    assert "dense_hbm_table(G=32768)" in plan and "partitioned(" not in plan, plan
    check(out, case, name)


def test_hash_hbm_table_without_a_sample(pl):
    """Case 2.  A sparse nullable Int64 key, n <= 2^23: the table is sized from the row count alone."""
    case = R.build("hash_nosample")
    out, plan, _ = run(pl, case)
    assert "hash_hbm_table(cap=2^23)" in plan and "sample(" not in plan and "grow+" not in plan, plan
    check(out, case)


def test_hash_hbm_table_grows_after_an_overflow(pl):
    """Case 3.  The first 2^22 rows hold 300 keys, all rows 150 000: a table of 2^12 slots, grown x4 at least three times; every attempt is a pass over all rows
    into a fresh table."""
    case = R.build("grow")
    out, plan, _ = run(pl, case, no_partition=True)
    assert plan.count("grow+") >= 3 and "sample(distinct=" in plan and re.search(r"hash_hbm_table\(cap=2\^(18|2\d)\)", plan) and "partitioned(" not in plan, plan
    check(out, case)


def test_single_key_lds_overflow_and_retry(pl):
    """Case 4.  The strided sample sees 7000 keys, the input 1e6: 64 and then 128 partitions of 6142 slots cannot hold them (fewer slots than keys); the third attempt, at
    256 partitions, does.  Three scatter + aggregate passes over all rows, each into buffers of its own; the key range is learned from the attempt that succeeded."""
    case = R.build("overflow_retry")
    out, plan, df = run(pl, case)
    assert "lds-overflow(P=64)+" in plan and "lds-overflow(P=128)+" in plan and plan.count("lds-overflow(P=") == 2 and "lds-overflow+" not in plan, plan
    assert re.search(V23 + "hash,P=256,", plan) and "lds_hash_table(slots=6142)" in plan and "hbm_table" not in plan and "hot=0+" in plan, plan
    assert "key_range_learned" in plan, plan
    check(out, case, "first run")
    k = case["cols"]["key"][0]
    # the learned range is that of ALL rows: the second run packs the key with it into a 40-bit id.  Its one attempt, planned from the same sample, overflows like the
    # first run's (this call site does not name its P); 40 bits are too many for the dense table, and the single-key route retries as above
    out2, plan2, _ = run(pl, case, df=df)
    assert "lds-overflow+" in plan2 and plan2.count("lds-overflow(P=") == 2 and re.search(V23 + "hash,P=256,", plan2) and "hbm_table" not in plan2, plan2
    check(out2, case, "second run")
    assert int(np.asarray(out2["key"].to_numpy()).min()) == int(k.min()) and int(np.asarray(out2["key"].to_numpy()).max()) == int(k.max())


def test_single_key_hot_list_planned_for_four_times_the_estimate_and_cached_sample(pl):
    """Cases 5 and 7.  One key holds half of the rows (a nullable key, a nullable f64 value: sum, count, min, mean): the hot list is aggregated in the scatter pass and the
    tables are planned for 4 x the estimate -- 256 partitions, where 1.3 x would take 128.  The second run of the same query on the same frame finds the sample cached
    (the learned key range spans more than 2^62: the key does not pack, its program is the same) and gives the same groups."""
    case = R.build("hot_fits")
    out, plan, df = run(pl, case)
    m = re.search(r"hot=(\d+)\+", plan)
    assert m and int(m.group(1)) > 0 and re.search(V23 + "hash,", plan) and parts(plan) == 256 and "lds-overflow" not in plan and "cached_" not in plan, plan
    check(out, case, "first run")
    out2, plan2, _ = run(pl, case, df=df)
    assert "cached_sample(" in plan2 and re.search(V23 + "hash,", plan2) and parts(plan2) == 256 and re.search(r"hot=[1-9]\d*\+", plan2), plan2
    check(out2, case, "second run")


def test_single_key_hot_list_fallback_to_the_plain_estimate(pl):
    """Case 6.  ~1e6 keys and a hot one: 4 x the estimate fits no plan, the first attempt is planned for 1.3 x instead -- with the hot list still in place."""
    case = R.build("hot_fallback")
    out, plan, _ = run(pl, case)
    assert re.search(V23 + "hash,P=512,", plan) and re.search(r"hot=[1-9]\d*\+", plan) and "lds_hash_table(slots=4606)" in plan and "lds-overflow" not in plan, plan
    check(out, case)


def test_key_range_learned_then_direct(pl, monkeypatch):
    """Case 8 (the plans of tests/test_gpu_datagen.py::test_dropped_statistics_change_the_plan_not_the_result): both runs against the reference, group by group."""
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    case = R.build("learned")
    out, plan, df = run(pl, case)
    assert "hash" in plan and "key_range_learned" in plan, plan
    check(out, case, "first run")
    out2, plan2, _ = run(pl, case, df=df)
    assert re.search(r"partitioned\(v3,direct", plan2), plan2
    check(out2, case, "second run")


def test_packed_ids_hash_partitions_from_a_sample(pl):
    """Case 9.  Two key columns (one nullable) packing into 26 bits, ~3e5 occupied ids, a nullable value: too many bits for direct-address LDS tables."""
    case = R.build("packed_hash")
    out, plan, _ = run(pl, case)
    assert "sample(distinct=" in plan and re.search(V23 + "hash,", plan) and "lds-overflow" not in plan and "hbm_table" not in plan, plan
    check(out, case)


def test_packed_ids_one_attempt_then_the_dense_table(pl):
    """Case 10.  The sample sees 6000 ids, the input 2e6: the one attempt overflows (this call site does not name its P) and the dense HBM table takes all rows."""
    case = R.build("packed_overflow")
    out, plan, _ = run(pl, case)
    assert "lds-overflow+" in plan and "lds-overflow(P=" not in plan and "dense_hbm_table(G=67108864)" in plan and "partitioned(" not in plan, plan
    assert plan.index("sample(distinct=") < plan.index("lds-overflow+") < plan.index("dense_hbm_table("), plan
    check(out, case)


@pytest.fixture(scope="module")
def join_frames(pl):
    j = R.build_join()
    P = pl.DataFrame({k: j["probe"][k] for k in ("k", "w", "x")})
    B = pl.DataFrame({k: j["build"][k] for k in ("k", "y", "z", "h", "c")})
    yield j, P, B
    j.clear()


@pytest.mark.parametrize("which", ["join_single_key", "join_packed_ids", "join_wide_keys"])
def test_group_bound_from_the_plan(pl, join_frames, which):
    """Cases 11-13.  join -> group_by whose aggregates read a build-side column (the pair form) and whose keys are functions of the build row: the plan knows a bound,
    one group per surviving build row, and it replaces the sampled estimate.  The probe rows reach only 40 000 build rows, so the partition count shows which of the
    two planned: 128 (single key) and 256 (wide keys) from the bound, 64 from any estimate.  Reference: the join on the host (np.searchsorted), then the group-by."""
    j, P, B = join_frames
    c = pl.col
    case = R.joined_case(j, which)
    q = P.lazy().join(B.lazy().filter(c("z") != 3), on="k").group_by(*case["keys"]).agg(*R.agg_exprs(pl, case["aggs"], {"wc": c("w") * c("c")}))
    out = q.collect()
    plan = pl.last_plan()
    print(f"plan[{which}]: {plan}")
    assert "FusedJoinGroupBy{pair form" in plan and f"groups<={j['build_rows']}(plan)+" in plan and "lds-overflow" not in plan, plan
    if which == "join_single_key":
        assert re.search(V23 + "hash,", plan) and parts(plan) == 128 and "lds_hash_table(slots=4606)" in plan, plan
    elif which == "join_packed_ids":
        assert re.search(V23 + "(direct|hash),", plan), plan
    else:
        assert re.search(V23 + "hash,P=256,", plan) and "lds_wide_key_table(words=2,slots=2632)" in plan, plan
    check(out, case, which)


def test_no_specialised_partition_kernel_falls_back_to_the_hbm_table(pl):
    """Case 14.  sum / min / len over a sparse key is neither of the shapes with ahead-of-time partition kernels; with the JIT off the partitioned pass reports that it
    has no kernel and the HBM hash table takes over (the generic interpreter)."""
    F = pl._ffi
    case = R.build("v2_unavailable")
    try:
        F.jit_set_min_rows(-1)
        out, plan, _ = run(pl, case)
    finally:
        F.jit_set_min_rows(1 << 22)
    assert "v2-unavailable+" in plan and plan.index("v2-unavailable+") < plan.index("hash_hbm_table(cap=2^") and "partitioned(" not in plan, plan
    check(out, case)


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("keys", [["k"], ["k", "k2"]])
def test_empty_and_single_row_inputs(pl, n, keys):
    """Case 15 (fewer than 2^24 rows by definition): no rows -> no groups; one row -> one group."""
    k = R.sparse(np.arange(7, 7 + n))
    case = {"n": n, "keys": keys, "aggs": [("s", "sum", "v"), ("n", "len", None)],
            "cols": {"k": (k, None), "k2": (R.full64(np.arange(3, 3 + n)), None), "v": (np.full(n, -5, np.int64), None)}}
    out, plan, _ = run(pl, case)
    assert out.height == n
    if n == 1:      # one raw 64-bit key: the hash table at its smallest; two keys of one value each pack into 1 + 1 bits: the LDS table
        assert ("hash_hbm_table(cap=2^10)" if len(keys) == 1 else "lds_table(G=4,") in plan, plan
    check(out, case)


@pytest.mark.parametrize("case", ["v1_single_key", "v1_packed_ids", "v1_wide_keys", "v1_single_key_overflow"])
def test_first_generation_partition_kernels(case):
    """PLX_PART_V=1: both call sites of partitioned_v1 (single key -- nullable key and value; packed ids -- dictionary codes), wide keys (not partitioned by this
    generation, as found) and the overflow of case 4's input, which this generation answers with the HBM hash table."""
    e = dict(os.environ)
    e["PLX_PART_V"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "groupby_route_worker.py"), case], capture_output=True, text=True, timeout=240, cwd=ROOT, env=e)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-1500:], r.stderr[-2500:])
