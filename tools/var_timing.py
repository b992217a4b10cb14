#!/usr/bin/env python3
"""What var / std cost.

(1) per_node    Series.var() over --rows Float64 rows (var_pivot_kernel + var_kernel + var_finish_kernel) next to Series.sum() on the same column (reduce_all: the
                same bytes through reduce_kernel) and next to a device copy that moves the same number of bytes (torch's copy kernel, HIP events, same process).
                `var_over_sum` at the medians of the kernel times; the expectation is "HBM-bound like reduce_kernel".
(2) group_by    group_by(k).agg(x.var()) against the identical query with x.mean(), with --keys-small keys (the LDS table) and with --keys-large keys (partitioned):
                var adds one f64 cell and two register ops per row.  `var_over_mean` at the medians of the kernel times and of the wall times.  The wall time of
                the var query holds the pivot pre-pass (one small launch and one synchronisation per var source, every query: nothing is cached); `pivot_prepass`
                times that pre-pass alone, as the whole-column var of the first 4096 rows' worth of work: a fused select over a 4096-row frame.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/var_timing.py [--rows 268435456] [--steps 10] [--warmup 2] [--keys-small 1000] [--keys-large 1000000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dt_part_timing import copy_ms  # noqa: E402  (a device copy of a given number of bytes, by HIP events)
from when_then_timing import timed  # noqa: E402  (the step timer: HIP-event kernel times + wall)

SEED = 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keys-small", type=int, default=1000)
    ap.add_argument("--keys-large", type=int, default=1_000_000)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    n, c = args.rows, pl.col
    out = {"rows": n, "steps": args.steps, "per_node": {}, "group_by": {}}

    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)      # uniform in [0, 100)
    res = {}
    for name, fn in (("var", lambda: x.var()), ("sum", lambda: x.sum())):
        def step(name=name, fn=fn):
            res[name] = fn()
        out["per_node"][name] = timed(F, step, args.steps, args.warmup)
    pn = out["per_node"]
    pn["copy_same_bytes"] = copy_ms(n * 8, args.steps, args.warmup)
    pn["var_over_sum"] = round(pn["var"]["kernel"]["median_ms"] / pn["sum"]["kernel"]["median_ms"], 4)
    pn["var_of_copy"] = round(pn["copy_same_bytes"]["median_ms"] / pn["var"]["kernel"]["median_ms"], 4)
    pn["var_TBps"] = round(n * 8 / (pn["var"]["kernel"]["median_ms"] * 1e-3) / 1e12, 3)
    pn["value"] = res["var"]
    assert abs(res["var"] - 100.0 ** 2 / 12) < 1.0, res

    for label, keys in (("small", args.keys_small), ("large", args.keys_large)):
        k = datagen.uniform_native(pl, "k", pl.Int64, n, SEED, 1 + keys % 7, 0, keys)
        df = pl.DataFrame([k, x])
        g = {}
        got = {}
        for name, agg in (("var", c("x").var().alias("a")), ("mean", c("x").mean().alias("a"))):
            q = df.lazy().group_by("k").agg(agg)
            def step(name=name, q=q):
                got[name] = q.collect()
            g[name] = timed(F, step, args.steps, args.warmup)
            g[name]["plan"] = pl.last_plan()[:300]
        assert got["var"].height == got["mean"].height
        g["groups"] = got["var"].height
        g["var_over_mean"] = round(g["var"]["kernel"]["median_ms"] / g["mean"]["kernel"]["median_ms"], 4)
        g["var_over_mean_wall"] = round(g["var"]["wall"]["median_ms"] / g["mean"]["wall"]["median_ms"], 4)
        out["group_by"][label] = g
        del df, k, got

    # the pivot pre-pass alone: the same throw-away select (sum, count of the source over 4096 rows), as a query of its own
    head = pl.DataFrame([datagen.uniform_native(pl, "x", pl.Float64, 4096, SEED, 0, 0, 10 ** 9, 1e-7)])
    q = head.lazy().select(c("x").sum().alias("s"), c("x").count().alias("n"))
    out["pivot_prepass"] = timed(F, lambda: q.collect(), args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
