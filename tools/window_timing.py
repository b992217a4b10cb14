#!/usr/bin/env python3
"""What a window expression costs.

(1) routes      with_columns(x.sum().over(k), x.mean().over(k)) over --rows rows, k an Int32 key with --keys dense values: the direct route (the default rule) next to
                the sorted route (PLX_WINDOW_ROUTE=sort) on the same frame, and next to the same question asked the only way there was before: group_by(k).agg(sum,
                mean) and a left join of the rows with the result on k (non-null keys, so the two agree).
(2) bound       the same two windows over --bound-rows rows whose key spans the largest range the rule admits for that many rows (4 R <= max(8 n, 4 MiB), i.e.
                R = max(2 n, 2^20)), direct next to sorted: the comparison the rule's bound stands on.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/window_timing.py [--rows 268435456] [--keys 1000000] [--bound-rows 16777216] [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from when_then_timing import timed  # noqa: E402  (the step timer: HIP-event kernel times + wall)

SEED = 29


def ratio(a, b):
    return round(a["kernel"]["median_ms"] / b["kernel"]["median_ms"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--bound-rows", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    c = pl.col
    out = {"rows": args.rows, "keys": args.keys, "bound_rows": args.bound_rows, "steps": args.steps, "routes": {}, "bound": {}}
    os.environ.pop("PLX_WINDOW_ROUTE", None)
    windows = [c("x").sum().over("k").alias("s"), c("x").mean().over("k").alias("m")]

    def both_routes(df, into):
        got = {}
        for name, route in (("direct", None), ("sorted", "sort")):
            if route:
                os.environ["PLX_WINDOW_ROUTE"] = route
            q = df.lazy().with_columns(*windows)
            def step(name=name, q=q):
                got[name] = q.collect()
            into[name] = timed(F, step, args.steps, args.warmup)
            into[name]["plan"] = pl.last_plan()[:600]
            os.environ.pop("PLX_WINDOW_ROUTE", None)
        assert "window[direct range=" in into["direct"]["plan"] and "window[sorted rows:" in into["sorted"]["plan"], into
        assert got["direct"].height == got["sorted"].height == df.height
        into["direct_over_sorted"] = ratio(into["direct"], into["sorted"])
        return got

    n = args.rows
    k = datagen.uniform_native(pl, "k", pl.UInt32, n, SEED, 1, 0, args.keys).cast(pl.Int32)
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    df = pl.DataFrame([k, x])
    r = out["routes"]
    got = both_routes(df, r)
    del got
    q = df.lazy().join(df.lazy().group_by("k").agg(c("x").sum().alias("s"), c("x").mean().alias("m")), on="k", how="left")
    res = {}
    def join_step():
        res["join"] = q.collect()
    r["group_by_left_join"] = timed(F, join_step, args.steps, args.warmup)
    r["group_by_left_join"]["plan"] = pl.last_plan()[:600]
    assert res["join"].height == n
    r["direct_over_join"] = ratio(r["direct"], r["group_by_left_join"])
    del res, df, k, x

    n = args.bound_rows
    R = max(2 * n, 1 << 20)
    k = datagen.uniform_native(pl, "k", pl.UInt32, n, SEED, 2, 0, R).cast(pl.Int32)
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    out["bound"]["range_asked"] = R
    both_routes(pl.DataFrame([k, x]), out["bound"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
