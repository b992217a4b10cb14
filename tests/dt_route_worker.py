"""Date-part group keys under PLX_PART_V=1 (the first-generation partition kernels; the variable is read once per process: tests/test_gpu_dt_parts.py starts this
script in a fresh child).  Runs the packed (year, month) ids and -- with the key ranges of date parts switched off -- the raw year key at 2^24 rows, checks the route
markers of the plan and every group against the reference of tests/test_gpu_dt_parts.py, prints the plans and OK."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import polars_amd as pl  # noqa: E402
from tests import test_gpu_dt_parts as T  # noqa: E402

V1 = (["partitioned(P=", "lds_hash_table(slots="], ["partitioned(v2", "partitioned(v3", "lds-overflow"])
CASES = [("v1_packed_year_month", 3000, "ym", True, *V1), ("v1_raw_year", 6000, "y", False, *V1)]


def main():
    assert os.environ.get("PLX_PART_V") == "1"
    pl.init(0)
    for name, span, keys, ranges, want, never in CASES:
        os.environ["PLX_TEMPORAL_KEY_RANGES"] = "1" if ranges else "0"
        df, block = T.route_frame(pl, 1 << 24, span)
        out = T.route_query(pl, df, keys).collect()
        plan = pl.last_plan()
        print(f"plan[{name}]: {plan}")
        for w in want:
            assert w in plan, (w, plan)
        for w in never:
            assert w not in plan, (w, plan)
        T.assert_groups(T.rows_by_key(out, list(keys)), T.route_reference(block, keys), name)
    print("OK")


if __name__ == "__main__":
    main()
