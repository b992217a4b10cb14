#!/usr/bin/env python3
"""What median / quantile cost.

(1) per_node    Series.median() over --rows Float64 rows (the radix select: encode, one round per digit on which the valid rows differ, one min pass) next to
                Series.sort() of the same column in the same process (arg-sort + gather).  The select reads 8 B per row and round; the sort moves 32 B per row and
                pass.  `median_below_sort_min`: the median of the select's kernel times lies below the MINIMUM of the sort's.
(2) group_by    group_by(k).agg(x.median()) over --group-rows rows with --keys-small and --keys-large keys, against arg_sort_by([k, x]) alone (the route cannot be
                faster than its sort: `median_over_sort` says what the group frame, the heads, the compaction, the pick and the alignment add) and against the
                identical query with x.mean() (`median_over_mean`: what the order statistic costs a user).
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/quantile_timing.py [--rows 268435456] [--group-rows 67108864] [--steps 10] [--warmup 2] [--keys-small 1000] [--keys-large 1000000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from when_then_timing import timed  # noqa: E402  (the step timer: HIP-event kernel times + wall)

SEED = 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--group-rows", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keys-small", type=int, default=1000)
    ap.add_argument("--keys-large", type=int, default=1_000_000)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    c = pl.col
    out = {"rows": args.rows, "group_rows": args.group_rows, "steps": args.steps, "per_node": {}, "group_by": {}}

    n = args.rows
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)      # uniform in [0, 100)
    res = {}
    for name, fn in (("median", lambda: x.median()), ("sort", lambda: x.sort())):
        def step(name=name, fn=fn):
            res[name] = fn()
        out["per_node"][name] = timed(F, step, args.steps, args.warmup)
        if name == "median":
            out["per_node"]["plan"] = pl.last_plan()
    pn = out["per_node"]
    pn["median_over_sort"] = round(pn["median"]["kernel"]["median_ms"] / pn["sort"]["kernel"]["median_ms"], 4)
    pn["median_below_sort_min"] = pn["median"]["kernel"]["median_ms"] < pn["sort"]["kernel"]["min_ms"]
    pn["value"] = res["median"]
    assert abs(res["median"] - 50.0) < 0.1, res["median"]
    del res, x

    n = args.group_rows
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    for label, keys in (("small", args.keys_small), ("large", args.keys_large)):
        k = datagen.uniform_native(pl, "k", pl.Int64, n, SEED, 1 + keys % 7, 0, keys)
        df = pl.DataFrame([k, x])
        g, got = {}, {}
        for name, agg in (("median", c("x").median().alias("a")), ("mean", c("x").mean().alias("a"))):
            q = df.lazy().group_by("k").agg(agg)
            def step(name=name, q=q):
                got[name] = q.collect()
            g[name] = timed(F, step, args.steps, args.warmup)
            g[name]["plan"] = pl.last_plan()[:400]
        def sort_step():
            got["sort"] = pl.arg_sort_by([k, x], nulls_last=True)
        g["sort"] = timed(F, sort_step, args.steps, args.warmup)
        assert got["median"].height == got["mean"].height
        g["groups"] = got["median"].height
        g["median_over_sort"] = round(g["median"]["kernel"]["median_ms"] / g["sort"]["kernel"]["median_ms"], 4)
        g["median_over_mean"] = round(g["median"]["kernel"]["median_ms"] / g["mean"]["kernel"]["median_ms"], 4)
        g["median_over_sort_wall"] = round(g["median"]["wall"]["median_ms"] / g["sort"]["wall"]["median_ms"], 4)
        g["median_over_mean_wall"] = round(g["median"]["wall"]["median_ms"] / g["mean"]["wall"]["median_ms"], 4)
        out["group_by"][label] = g
        del df, k, got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
