#!/usr/bin/env python3
"""What n_unique / unique() cost.

(1) per_node    Series.n_unique() over --rows Float64 rows (the sorted-codes route: encode, a key-only radix sort, a count of the run heads) next to Series.sort() of
                the same column (arg-sort + gather); and over --rows Int32 rows of range --int-range on the bitmap route next to the forced sort route
                (PLX_NUNIQUE_ROUTE=sort) on the same column.
(2) group_by    group_by(k).agg(x.n_unique()) over --group-rows rows with --keys-small and --keys-large keys, against arg_sort_by([k, x]) alone, against the same
                query with x.median(), against x.median() alone next to the list median + n_unique of the one source (one sort: the second aggregate should be nearly
                free).
(3) unique      unique(subset=[k], keep="first") of the two-column frame with --keys-large keys against arg_sort_by([k]) alone.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/distinct_timing.py [--rows 268435456] [--group-rows 67108864] [--steps 10] [--warmup 2] [--keys-small 1000] [--keys-large 1000000] [--int-range 1000000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from when_then_timing import timed  # noqa: E402  (the step timer: HIP-event kernel times + wall)

SEED = 23


def ratio(a, b):
    return round(a["kernel"]["median_ms"] / b["kernel"]["median_ms"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--group-rows", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keys-small", type=int, default=1000)
    ap.add_argument("--keys-large", type=int, default=1_000_000)
    ap.add_argument("--int-range", type=int, default=1_000_000)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    c = pl.col
    out = {"rows": args.rows, "group_rows": args.group_rows, "steps": args.steps, "per_node": {}, "group_by": {}, "unique": {}}
    os.environ.pop("PLX_NUNIQUE_ROUTE", None)

    n = args.rows
    pn, res = out["per_node"], {}
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    for name, fn in (("n_unique_f64", lambda: x.n_unique()), ("sort_f64", lambda: x.sort())):
        def step(name=name, fn=fn):
            res[name] = fn()
        pn[name] = timed(F, step, args.steps, args.warmup)
        if name == "n_unique_f64":
            pn["plan_f64"] = pl.last_plan()
    pn["n_unique_over_sort"] = ratio(pn["n_unique_f64"], pn["sort_f64"])
    pn["value_f64"] = res["n_unique_f64"]
    del res, x
    i = datagen.uniform_native(pl, "i", pl.UInt32, n, SEED, 1, 0, args.int_range).cast(pl.Int32)
    res = {}
    for name, route in (("n_unique_i32_bitmap", None), ("n_unique_i32_sort", "sort")):
        if route:
            os.environ["PLX_NUNIQUE_ROUTE"] = route
        def step(name=name):
            res[name] = i.n_unique()
        pn[name] = timed(F, step, args.steps, args.warmup)
        pn["plan_" + name] = pl.last_plan()
        os.environ.pop("PLX_NUNIQUE_ROUTE", None)
    assert res["n_unique_i32_bitmap"] == res["n_unique_i32_sort"] and "bitmap" in pn["plan_n_unique_i32_bitmap"] and "sorted codes" in pn["plan_n_unique_i32_sort"], (res, pn)
    pn["bitmap_over_sort_route"] = ratio(pn["n_unique_i32_bitmap"], pn["n_unique_i32_sort"])
    pn["value_i32"] = res["n_unique_i32_bitmap"]
    del res, i

    n = args.group_rows
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    for label, keys in (("small", args.keys_small), ("large", args.keys_large)):
        k = datagen.uniform_native(pl, "k", pl.Int64, n, SEED, 1 + keys % 7, 0, keys)
        df = pl.DataFrame([k, x])
        g, got = {}, {}
        for name, aggs in (("n_unique", [c("x").n_unique().alias("a")]), ("median", [c("x").median().alias("a")]), ("median_and_n_unique", [c("x").median().alias("a"), c("x").n_unique().alias("b")])):
            q = df.lazy().group_by("k").agg(*aggs)
            def step(name=name, q=q):
                got[name] = q.collect()
            g[name] = timed(F, step, args.steps, args.warmup)
            g[name]["plan"] = pl.last_plan()[:500]
        def sort_step():
            got["sort"] = pl.arg_sort_by([k, x], nulls_last=True)
        g["sort"] = timed(F, sort_step, args.steps, args.warmup)
        assert got["n_unique"].height == got["median"].height
        g["groups"] = got["n_unique"].height
        g["n_unique_over_sort"] = ratio(g["n_unique"], g["sort"])
        g["n_unique_over_median"] = ratio(g["n_unique"], g["median"])
        g["list_over_median"] = ratio(g["median_and_n_unique"], g["median"])
        out["group_by"][label] = g
        if label == "large":
            u, got = out["unique"], {}
            q = df.lazy().unique("k", keep="first")
            def ustep():
                got["unique"] = q.collect()
            u["unique"] = timed(F, ustep, args.steps, args.warmup)
            u["plan"] = pl.last_plan()[:400]
            def ksort_step():
                got["sort"] = pl.arg_sort_by([k], nulls_last=True)
            u["sort"] = timed(F, ksort_step, args.steps, args.warmup)
            u["kept"] = got["unique"].height
            u["unique_over_sort"] = ratio(u["unique"], u["sort"])
        del df, k, got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
