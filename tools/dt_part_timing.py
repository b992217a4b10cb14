#!/usr/bin/env python3
"""What the date parts cost.

(1) per_node    Series.dt.year() / dt.weekday() over --rows rows of a Date (4 B in) and of a Datetime[us] (8 B in) column, 1 or 4 B out per row, next to a plain device
                copy that moves the SAME number of bytes (half in, half out; torch's copy kernel, timed with HIP events in the same run).  `of_copy` = copy time /
                kernel time: 1.0 is a kernel that streams as fast as a copy of its bytes.
(2) group_by    filter(d <= cutoff).group_by(year, month).agg(sum(x), len) over --rows rows in three forms:
                  (a) fused      group_by(d.dt.year(), d.dt.month()): both parts computed inside the scan
                  (b) columns    the identical query over precomputed Int32 year / Int8 month columns (code that predates the dt namespace: the baseline)
                  (c) per_node   with_columns(year, month) materialised by the per-node kernel, then (b)'s query
                `a_over_b`, `a_over_c` at the medians of the kernel times (a_over_c < 1 is the requirement: (c) moves at least 10 more bytes per row).
(3) raw_keys    (a) with PLX_TEMPORAL_KEY_RANGES=0: the parts are raw 64-bit keys (a wide hash key) instead of a 7-bit packed id: what the dense routes are worth.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/dt_part_timing.py [--rows 268435456] [--steps 10] [--warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from when_then_timing import timed  # noqa: E402  (the same step timer: HIP-event kernel times + wall)

SEED = 13
DAY_LO, DAY_HI = 8035, 10592          # 1992-01-01 .. 1998-12-31
DAY_US = 86_400_000_000


def copy_ms(nbytes_total, steps, warmup):
    """A device copy that reads nbytes_total / 2 and writes nbytes_total / 2: [median, min, max] ms by HIP events."""
    import numpy as np
    import torch
    src = torch.empty(nbytes_total // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.fill_(1)
    for _ in range(warmup):
        dst.copy_(src)
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    n, c = args.rows, pl.col
    out = {"rows": n, "steps": args.steps, "per_node": {}, "group_by": {}, "raw_keys": {}}

    def relabel(s, name, dtype):
        F.check(F.lib().plx_column_retain(s._h))
        return pl.Series._from_handle(name, s._h, dtype)

    days = datagen.uniform_native(pl, "days", pl.UInt32, n, SEED, 0, DAY_LO, DAY_HI).cast(pl.Int32)
    d = relabel(days, "d", pl.Date)
    t = relabel(datagen.uniform_native(pl, "ticks", pl.Int64, n, SEED, 1, DAY_LO * DAY_US, DAY_HI * DAY_US), "t", pl.Datetime)
    del days

    # (1) the per-node kernel against a copy of its bytes
    keep = {}
    for col, width_in in ((d, 4), (t, 8)):
        for part, width_out in (("year", 4), ("weekday", 1)):
            name = f"{part}_{'date' if width_in == 4 else 'datetime_us'}"
            def step(col=col, part=part, name=name):
                keep[name] = getattr(col.dt, part)()
            r = timed(F, step, args.steps, args.warmup)
            r["bytes_per_row"] = width_in + width_out
            r["copy_same_bytes"] = copy_ms(n * (width_in + width_out), args.steps, args.warmup)
            r["of_copy"] = round(r["copy_same_bytes"]["median_ms"] / r["kernel"]["median_ms"], 3)
            r["TBps"] = round(n * (width_in + width_out) / (r["kernel"]["median_ms"] * 1e-3) / 1e12, 3)
            out["per_node"][name] = r
            keep.clear()
    del t

    # (2) the group-by in three forms
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 2, 0, 10 ** 9, 1e-7)
    year, month = d.dt.year().rename("year"), d.dt.month().rename("month")
    df = pl.DataFrame([d, x, year, month])
    cutoff = __import__("datetime").date(1998, 9, 2)
    aggs = (c("x").sum().alias("s"), pl.len().alias("n"))
    forms = {
        "a_fused": df.lazy().filter(c("d") <= cutoff).group_by(c("d").dt.year().alias("year"), c("d").dt.month().alias("month")).agg(*aggs),
        "b_columns": df.lazy().filter(c("d") <= cutoff).group_by("year", "month").agg(*aggs),
        "c_per_node": None,
    }
    results = {}
    def run(name, fn, into):
        def step():
            results[name] = fn()
        into[name] = timed(F, step, args.steps, args.warmup)
        into[name]["plan"] = pl.last_plan()[:260]
    for name in ("a_fused", "b_columns"):
        run(name, lambda lf=forms[name]: lf.collect().sort_host(["year", "month"]), out["group_by"])
    base = pl.DataFrame([d, x])
    def per_node():
        mat = base.lazy().with_columns(c("d").dt.year().alias("year"), c("d").dt.month().alias("month")).collect(no_fusion=True)
        return mat.lazy().filter(c("d") <= cutoff).group_by("year", "month").agg(*aggs).collect().sort_host(["year", "month"])
    run("c_per_node", per_node, out["group_by"])
    for other in ("b_columns", "c_per_node"):
        assert all(results["a_fused"][k] == results[other][k] for k in ("year", "month", "n")), f"a_fused and {other} differ"
    g = out["group_by"]
    g["groups"] = len(results["a_fused"]["n"])
    g["a_over_b"] = round(g["a_fused"]["kernel"]["median_ms"] / g["b_columns"]["kernel"]["median_ms"], 4)
    g["a_over_c"] = round(g["a_fused"]["kernel"]["median_ms"] / g["c_per_node"]["kernel"]["median_ms"], 4)
    g["a_over_b_wall"] = round(g["a_fused"]["wall"]["median_ms"] / g["b_columns"]["wall"]["median_ms"], 4)
    g["a_over_c_wall"] = round(g["a_fused"]["wall"]["median_ms"] / g["c_per_node"]["wall"]["median_ms"], 4)

    # (3) the same fused query with the parts as raw 64-bit keys
    os.environ["PLX_TEMPORAL_KEY_RANGES"] = "0"
    try:
        run("a_fused_raw_keys", lambda: forms["a_fused"].collect().sort_host(["year", "month"]), out["raw_keys"])
    finally:
        del os.environ["PLX_TEMPORAL_KEY_RANGES"]
    assert all(results["a_fused"][k] == results["a_fused_raw_keys"][k] for k in ("year", "month", "n")), "raw keys give other groups"
    out["raw_keys"]["raw_over_packed"] = round(out["raw_keys"]["a_fused_raw_keys"]["kernel"]["median_ms"] / g["a_fused"]["kernel"]["median_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
