#!/usr/bin/env python3
"""What a cumulative or ranking function costs.

(1) whole       Series.cum_sum() over --rows rows, a Float64 and an Int32 column: the three launches of the segmented scan (tile aggregates, their scan, the tiles
                with their carry) against the algorithmic bytes N (2 w_in + w_out) and the HBM peak, next to torch.cumsum on the same data on the same device (a
                single-pass scan reads the input once: the byte model gives this scan up to about 1.5 times its time).
(2) over        with_columns(x.cum_sum().over(k)) and with_columns(x.rank("ordinal").over(k)) over --rows rows, k an Int32 key with --keys dense values, split by
                kernel name into sort, heads and the scan / rank kernel: what stands beside the sorted route of a window over the same keys.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call.  One JSON line on stdout.

    python tools/cumulative_timing.py [--rows 268435456] [--keys 1000000] [--steps 5] [--warmup 1] [--no-torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from when_then_timing import kernel_records, timed  # noqa: E402  (the step timer: HIP-event kernel times + wall)

SEED = 31
HBM_PEAK_TBPS = 8.0          # MI355X datasheet


def split_by_kernel(F, step):
    """one more profiled step: kernel time in ms per kernel name"""
    F.check(F.lib().plx_synchronize())
    F.check(F.lib().plx_profile_enable(1))
    kernel_records(F)
    step()
    F.check(F.lib().plx_synchronize())
    recs = kernel_records(F)
    F.check(F.lib().plx_profile_enable(0))
    out = {}
    for r in recs:
        out[r[0]] = round(out.get(r[0], 0.0) + r[1] / 1e3, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    c = pl.col
    n = args.rows
    out = {"rows": n, "keys": args.keys, "steps": args.steps, "whole": {}, "over": {}}

    for name, dt, w_in, w_out in (("Float64", pl.Float64, 8, 8), ("Int32", pl.Int32, 4, 4)):
        if dt == pl.Float64:
            s = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
        else:
            s = datagen.uniform_native(pl, "x", pl.UInt32, n, SEED, 3, 0, 1000).cast(pl.Int32)
        keep = {}
        def step(s=s, keep=keep):
            keep["out"] = s.cum_sum()
        r = timed(F, step, args.steps, args.warmup)
        r["plan"] = pl.last_plan()[:300]
        algo = n * (2 * w_in + w_out)
        r["algorithmic_bytes"] = algo
        r["fraction_of_hbm_peak"] = round(algo / (r["kernel"]["median_ms"] * 1e-3) / (HBM_PEAK_TBPS * 1e12), 4)
        if not args.no_torch:
            import torch
            t = s.to_torch()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = []
            for i in range(args.warmup + args.steps):
                ev[0].record()
                y = torch.cumsum(t, 0)
                ev[1].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ms.append(ev[0].elapsed_time(ev[1]))
            r["torch_cumsum"] = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
                                 "out_dtype": str(y.dtype)}
            r["ours_over_torch"] = round(r["kernel"]["median_ms"] / r["torch_cumsum"]["median_ms"], 4)
            del t, y
        out["whole"][name] = r
        del s, keep

    k = datagen.uniform_native(pl, "k", pl.UInt32, n, SEED, 1, 0, args.keys).cast(pl.Int32)
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    df = pl.DataFrame([k, x])
    for name, e, word in (("cum_sum", c("x").cum_sum().over("k").alias("s"), "cumulative[sorted rows:"), ("rank_ordinal", c("x").rank("ordinal").over("k").alias("r"), "rank[sorted segments:")):
        q = df.lazy().with_columns(e)
        got = {}
        def step(q=q, got=got):
            got["out"] = q.collect()
        r = timed(F, step, args.steps, args.warmup)
        r["plan"] = pl.last_plan()[:600]
        assert word in r["plan"], r["plan"]
        assert got["out"].height == n
        r["by_kernel_ms"] = split_by_kernel(F, step)
        out["over"][name] = r
        del got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
