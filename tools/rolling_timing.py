#!/usr/bin/env python3
"""What shift and a rolling function cost.

Over --rows Float64 rows, plain (the whole column) and `.over(k)` with k an Int32 key of --keys dense values:
(1) rolling_sum at w = 7, 256 and 2048 on the tile-halo route (one launch: the operand read once plus its halo, the result written once);
(2) the same three forced onto the two-scan route (PLX_ROLLING_ROUTE=scans: seven launches, P and S through memory);
(3) shift(1) (one launch: a copy at an offset and the shifted bitmap);
(4) cum_sum of the same column (three launches, two reads and one write): the yardstick the tile route's one read and one write are explained against.
Per case: warm-up, then --steps timed steps; median / minimum / maximum of the per-step sum of the library's HIP-event kernel times and of the host wall time around
the call, the kernels' declared bytes and their names; for the `.over` cases one more profiled step split by kernel name.  One JSON line on stdout.

    python tools/rolling_timing.py [--rows 268435456] [--keys 1000] [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cumulative_timing import split_by_kernel  # noqa: E402
from when_then_timing import timed  # noqa: E402  (the step timer: HIP-event kernel times + wall)

SEED = 37
HBM_PEAK_TBPS = 8.0          # MI355X datasheet
WINDOWS = (7, 256, 2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    c = pl.col
    n = args.rows
    out = {"rows": n, "keys": args.keys, "steps": args.steps, "whole": {}, "over": {}}
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 0, 0, 10 ** 9, 1e-7)
    k = datagen.uniform_native(pl, "k", pl.UInt32, n, SEED, 1, 0, args.keys).cast(pl.Int32)
    df = pl.DataFrame([k, x])

    cases = [(f"rolling_sum_w{w}_{route}", route, lambda e, w=w: e.rolling_sum(w), "rolling[tile halo:" if route == "tile" else "rolling[two scans:") for route in ("tile", "scans")
             for w in WINDOWS]
    cases += [("shift_1", "tile", lambda e: e.shift(1), "shift["), ("cum_sum", "tile", lambda e: e.cum_sum(), "cumulative[")]
    for name, route, fn, word in cases:
        os.environ["PLX_ROLLING_ROUTE"] = route                      # read per call
        for where, q in (("whole", df.lazy().select(fn(c("x")).alias("y"))), ("over", df.lazy().select(fn(c("x")).over("k").alias("y")))):
            got = {}
            def step(q=q, got=got):
                got["out"] = q.collect()
            r = timed(F, step, args.steps, args.warmup)
            r["plan"] = pl.last_plan()[:400]
            assert word in r["plan"], r["plan"]
            assert got["out"].height == n
            # one read of the operand and one write of the result (shift and the tile route), against what the route's kernels declare
            r["one_read_one_write_bytes"] = n * 16
            r["fraction_of_hbm_peak_on_those"] = round(n * 16 / (r["kernel"]["median_ms"] * 1e-3) / (HBM_PEAK_TBPS * 1e12), 4)
            if where == "over":
                r["by_kernel_ms"] = split_by_kernel(F, step)
            out[where][name] = r
            del got
    os.environ.pop("PLX_ROLLING_ROUTE", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
