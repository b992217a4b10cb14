"""One group-by under PLX_PART_V=1 (the first-generation partition kernels; the variable is read once per process: tests/test_gpu_groupby_routes.py starts this script
once per case).  argv: the case name.  Builds the input with tests/groupby_route_inputs.py, checks the route markers of the plan and every group against the numpy
reference, prints the plan and OK."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_edges as E  # noqa: E402
import groupby_route_inputs as R  # noqa: E402
import polars_amd as pl  # noqa: E402

V1_PARTITIONED = (["partitioned(P=", "lds_hash_table(slots="], ["partitioned(v2", "partitioned(v3", "lds-overflow"])
CASES = {      # case -> (input, markers the plan must contain, markers it must not contain)
    "v1_single_key": ("v1_single_key", *V1_PARTITIONED),
    "v1_packed_ids": ("v1_packed_ids", *V1_PARTITIONED),
    "v1_wide_keys": ("v1_wide_keys", ["wide_hash_hbm_table(words=2,cap=2^"], ["partitioned("]),      # as found: wide keys are not partitioned by the first generation
    "v1_edges": ("v1_edges", *V1_PARTITIONED),      # the planted edge groups of tests/agg_edges.py: one query per value column, checked by its own comparison
    "v1_single_key_overflow": ("overflow_retry", ["lds-overflow+", "grow+", "hash_hbm_table(cap=2^"], ["lds-overflow(P=", "partitioned("]),
}


def main():
    assert os.environ.get("PLX_PART_V") == "1"
    inp, want, never = CASES[sys.argv[1]]
    pl.init(0)
    if sys.argv[1] == "v1_edges":
        return edges(want, never)
    case = R.build(inp)
    out = R.query(pl, R.frame(pl, case).lazy(), case).collect()
    plan = pl.last_plan()
    print(f"plan[{sys.argv[1]}]: {plan}")
    for w in want:
        assert w in plan, (w, plan)
    for w in never:
        assert w not in plan, (w, plan)
    if sys.argv[1] == "v1_single_key_overflow":
        assert plan.index("lds-overflow+") < plan.index("grow+") < plan.index("hash_hbm_table(")
    R.assert_groups_equal(R.download(out), R.case_reference(case), case["keys"], sys.argv[1])
    print("OK")


def edges(want, never):
    """sum, mean, min, max, count of v (Int64 edge kinds) and then of x (Float64 edge kinds) + len, every group against the vectorised reference"""
    case = E.planted_case("v1_edges")
    df = pl.DataFrame([pl.Series("key", case["key"][0], validity=case["key"][1])] + [pl.Series(c, case[c][0], validity=case[c][1]) for c in ("v", "x")])
    for col in ("v", "x"):
        out = df.lazy().group_by("key").agg(*[getattr(pl.col(col), op)().alias(op) for op in E.OPS[:-1]], pl.len().alias("len")).collect()
        plan = pl.last_plan()
        print(f"plan[v1_edges {col}]: {plan}")
        for w in want:
            assert w in plan, (w, plan)
        for w in never:
            assert w not in plan, (w, plan)
        worst = E.check_planted(R.download(out), case, col, ("v1_edges", col))
        print(f"worst relative error [v1 partitioned, {col}]: {worst:.3e}")
    print("OK")


if __name__ == "__main__":
    main()
