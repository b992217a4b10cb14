#!/usr/bin/env python3
"""What the string predicates cost.

(a) raw_inline   Series.str.starts_with / contains over --rows inline views ("id%010d": 12 bytes, the view is the string; plx_datagen_id_views).  The kernel streams
                 16 B per row in and 2 bits per row out: the figure to hold against the copy ceiling is 16 B x rows / time.
(b) raw_long     Series.str.ends_with over --rows views of 20-byte strings ("id%010d-longkey", plx_datagen_long_id_views) whose bytes sit in a pool of --pool-keys
                 distinct strings: every row reads its view (streamed) and up to two 128-byte lines of the pool at a random place -- expect the pool's lines, not the
                 views, to set the time (`pool_line_bytes` = rows x 128 B x lines touched is the arithmetic to hold the time against).
(c) plan         filter(pred) -> group_by(k).agg(sum(x), len) over --rows rows where pred is a string predicate on a Categorical column (str_pred: one bit out of
                 an L2-resident bitmap per row, inside the fused scan), next to the SAME selection written as a comparison of the codes (code_cmp: existing code, the
                 reference).  `ratio` = str_pred / code_cmp at the medians.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/str_match_timing.py [--rows 268435456] [--steps 10] [--warmup 2] [--pool-keys 16777216]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from when_then_timing import timed  # noqa: E402  (the same step timer: HIP-event kernel times + wall)

SEED = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pool-keys", type=int, default=1 << 24)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    n, c = args.rows, pl.col
    out = {"rows": n, "steps": args.steps, "raw_inline": {}, "raw_long": {}, "plan": {}}

    def per_row(res, bytes_per_row):
        res["TBps_on_%dB_x_rows" % bytes_per_row] = round(n * bytes_per_row / (res["kernel"]["median_ms"] * 1e-3) / 1e12, 3)
        return res

    # (a) inline views
    views = datagen.id_views_native(pl, "v", n, SEED, 0, 0, 10 ** 9)
    s = pl.Series.from_device_views("s", views, None, encode="deferred")
    keep = {}
    for name, fn in (("starts_with", lambda: s.str.starts_with("id00000")), ("contains", lambda: s.str.contains("123"))):
        def step(name=name, fn=fn):
            keep[name] = fn()
        out["raw_inline"][name] = per_row(timed(F, step, args.steps, args.warmup), 16)
        out["raw_inline"][name]["true_rows"] = int(keep[name]._download()[0].sum())
    assert s._is_raw_views()
    del s, views
    keep.clear()

    # (b) long views: 20-byte strings in a pool
    lviews, ldata = datagen.long_id_views_native(pl, n, SEED, 1, 0, args.pool_keys)
    ls = pl.Series.from_device_views("s", lviews, ldata, encode="deferred")
    def step_long():
        keep["ends_with"] = ls.str.ends_with("7-longkey")
    r = per_row(timed(F, step_long, args.steps, args.warmup), 16)
    r["true_rows"] = int(keep["ends_with"]._download()[0].sum())
    r["pool_bytes"] = args.pool_keys * 20
    # a 20-byte string at offset 20 i lies in one 128-byte line unless it crosses a boundary: (20 i mod 128) > 108, 4 of every 32 strings
    r["pool_line_bytes"] = int(n * 128 * (1 + 4 / 32))
    r["TBps_of_pool_lines"] = round(r["pool_line_bytes"] / (r["kernel"]["median_ms"] * 1e-3) / 1e12, 3)
    out["raw_long"]["ends_with"] = r
    del ls, lviews, ldata
    keep.clear()

    # (c) filter -> group-by: the predicate on the strings against the same selection on the codes
    types = sorted(a + " " + b + " " + m for a in ("STANDARD", "SMALL", "MEDIUM", "LARGE", "ECONOMY", "PROMO") for b in ("ANODIZED", "BURNISHED", "PLATED", "POLISHED", "BRUSHED")
                   for m in ("TIN", "NICKEL", "BRASS", "STEEL", "COPPER"))
    lo, hi = min(i for i, t in enumerate(types) if t.startswith("PROMO")), 1 + max(i for i, t in enumerate(types) if t.startswith("PROMO"))
    assert all(t.startswith("PROMO") == (lo <= i < hi) for i, t in enumerate(types))            # sorted: the PROMO types are one code range
    code = datagen.uniform_native(pl, "code", pl.UInt32, n, SEED, 2, 0, len(types))
    F.check(F.lib().plx_column_retain(code._h))
    t = pl.Series._from_handle("t", code._h, pl.Categorical(types, pl.UInt32))                   # the same buffer, seen as a dictionary column
    k = datagen.uniform_native(pl, "k", pl.Int64, n, SEED, 3, 0, 8)
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 4, 0, 10 ** 9, 1e-7)
    df = pl.DataFrame([t, code, k, x])
    aggs = (c("x").sum().alias("s"), pl.len().alias("n"))
    results = {}
    for name, lf in (("code_cmp", df.lazy().filter((c("code") >= lo) & (c("code") < hi)).group_by("k").agg(*aggs)),
                     ("str_pred", df.lazy().filter(c("t").str.starts_with("PROMO")).group_by("k").agg(*aggs))):
        def step(name=name, lf=lf):
            results[name] = lf.collect().sort_host("k")
        out["plan"][name] = timed(F, step, args.steps, args.warmup)
        out["plan"][name]["plan"] = pl.last_plan()[:200]
    assert results["code_cmp"]["n"] == results["str_pred"]["n"] and results["code_cmp"]["k"] == results["str_pred"]["k"], "the two forms select different rows"
    out["plan"]["selected_rows"] = int(sum(results["str_pred"]["n"]))
    out["plan"]["ratio"] = round(out["plan"]["str_pred"]["kernel"]["median_ms"] / out["plan"]["code_cmp"]["kernel"]["median_ms"], 4)
    out["plan"]["ratio_wall"] = round(out["plan"]["str_pred"]["wall"]["median_ms"] / out["plan"]["code_cmp"]["wall"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
