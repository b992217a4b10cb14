#!/usr/bin/env python3
"""What when / then / otherwise costs, fused and per node, next to the existing kernels with the same traffic.

Fused, over bench.py's config-2 columns (a Int64, x / y Float64; same generator call and seed):
    filter_sum   filter(a > c).select(sum(x * y))                              the existing shape: three columns read once
    when_sum     select(sum(when(a > c).then(x * y).otherwise(0.0)))           the same bytes through OP_SELECT
Per node, on Int64 and Float64 columns:
    arith        a + b                    (arith_kernel: two inputs, one output)
    select       mask ? a : b             (select_kernel; `select_nullable`: the then side carries a validity bitmap, so does the result)
Per case: warm-up, then --steps timed steps; the median, minimum and maximum of the per-step sum of the library's HIP-event kernel times and of the host wall
time around the call (which ends in a synchronise), and the bytes the kernels declared (ProfileScope).  Cases the imported package lacks are skipped, so the same
file times an older checkout.  One JSON line on stdout.

    python tools/when_then_timing.py [--rows 1000000000] [--steps 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 10


def kernel_records(F):
    cap = 4096
    recs = (F.ProfileRecord * cap)()
    n = C.c_int32()
    F.check(F.lib().plx_profile_fetch(recs, cap, C.byref(n)))
    out = [(recs[i].name.decode(), recs[i].end_us - recs[i].start_us, int(recs[i].algo_bytes)) for i in range(n.value)]
    F.check(F.lib().plx_profile_clear())
    return out


def timed(F, step, steps, warmup):
    for _ in range(warmup):
        step()
    F.check(F.lib().plx_synchronize())
    F.check(F.lib().plx_profile_enable(1))
    kernel_records(F)
    wall, kern, names, nbytes = [], [], {}, 0
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        F.check(F.lib().plx_synchronize())
        wall.append((time.perf_counter() - t0) * 1e3)
        recs = kernel_records(F)
        kern.append(sum(r[1] for r in recs) / 1e3)
        names = {r[0]: r[2] for r in recs}
        nbytes = sum(r[2] for r in recs)
    F.check(F.lib().plx_profile_enable(0))
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}
    k = stat(kern)
    return {"kernel": k, "wall": stat(wall), "declared_bytes": nbytes, "kernels": names,
            "declared_TBps_at_median": round(nbytes / (k["median_ms"] * 1e-3) / 1e12, 3) if k["median_ms"] > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    F = pl._ffi
    pl.init(0)
    n, c = args.rows, pl.col
    a = datagen.uniform_native(pl, "a", pl.Int64, n, SEED, 0, 0, 2 ** 31)
    x = datagen.uniform_native(pl, "x", pl.Float64, n, SEED, 1, 0, 10 ** 9, 1e-7)
    y = datagen.uniform_native(pl, "y", pl.Float64, n, SEED, 2, 0, 10 ** 9, 1e-9)
    df = pl.DataFrame([a, x, y])
    cut = 2 ** 30
    out = {"rows": n, "steps": args.steps, "has_when": hasattr(pl, "when"), "fused": {}, "per_node": {}}

    results = {}
    def fused(name, lf):
        def step():
            results[name] = lf.collect().to_dict()
        out["fused"][name] = timed(F, step, args.steps, args.warmup)
        out["fused"][name]["plan"] = pl.last_plan()[:160]
        out["fused"][name]["result"] = results[name]
    fused("filter_sum", df.lazy().filter(c("a") > cut).select((c("x") * c("y")).sum().alias("s")))
    if hasattr(pl, "when"):
        fused("when_sum", df.lazy().select(pl.when(c("a") > cut).then(c("x") * c("y")).otherwise(0.0).sum().alias("s")))

    def call(fn, *handles):
        h = C.c_uint64()
        F.check(fn(*handles, C.byref(h)))
        F.check(F.lib().plx_column_free(h.value))
    mask = a > cut
    a2 = datagen.uniform_native(pl, "a2", pl.Int64, n, SEED, 3, 0, 2 ** 31)
    valid = datagen.uniform_native(pl, "v", pl.Int64, n, SEED, 4, 0, 10) > 0          # a Boolean column: its bitmap serves as a validity bitmap below
    for tag, p, q, dt in (("Int64", a, a2, pl.Int64), ("Float64", x, y, pl.Float64)):
        out["per_node"][f"arith_{tag}"] = timed(F, lambda: call(F.lib().plx_arith, F.ADD, p._h, q._h), args.steps, args.warmup)
        if hasattr(F.lib(), "plx_if_then_else"):
            out["per_node"][f"select_{tag}"] = timed(F, lambda: call(F.lib().plx_if_then_else, mask._h, p._h, q._h), args.steps, args.warmup)
            pv, vv = p.device_ptrs()[0], valid.device_ptrs()[0]
            pn = pl.Series.from_device("pn", dt, pv, n, vv, keepalive=(p, valid))
            out["per_node"][f"select_nullable_{tag}"] = timed(F, lambda: call(F.lib().plx_if_then_else, mask._h, pn._h, q._h), args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
