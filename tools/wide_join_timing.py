#!/usr/bin/env python3
"""What the wide-key join route (kernels_join_wide.hip) costs: an inner join of 2^24 probe rows with 2^20 build rows (unique build keys, half of the probe rows match) on
  1. three key columns (Int32, Int64, Boolean) that DO pack into one Int64: the packed route (the yardstick, default) and the wide route (PLX_JOIN_WIDE_KEYS=2) on the
     same frames, steps interleaved in one process; the two results are checked equal over all rows;
  2. two full-range Int64 key columns: the wide route only (these keys do not pack); the result is checked against the build-side ids the generator knows.
Per case: warm-up, then --steps timed steps -- the median / min / max of the per-step sum of the library's HIP-event kernel times and of the host wall time around
collect() -- and the kernels of the last step with their time and declared bytes (ProfileScope).  One JSON line per case on stdout.

    python tools/wide_join_timing.py [--probe 16777216] [--build 1048576] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 31
MULT_A, MULT_B = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F)


def kernel_stats(pl):
    import ctypes as C
    F = pl._ffi
    cap = 65536
    recs = (F.ProfileRecord * cap)()
    n = C.c_int32()
    F.check(F.lib().plx_profile_fetch(recs, cap, C.byref(n)))
    out = {}
    for i in range(n.value):
        r = recs[i]
        e = out.setdefault(r.name.decode(), [0, 0.0, 0])
        e[0] += 1; e[1] += r.end_us - r.start_us; e[2] += int(r.algo_bytes)
    return out


def timed_step(pl, q, env):
    F = pl._ffi
    for k, v in env.items():
        os.environ[k] = v
    try:
        F.check(F.lib().plx_profile_clear()); F.check(F.lib().plx_profile_enable(1))
        t0 = time.perf_counter()
        out = q.collect(no_fusion=True)
        F.check(F.lib().plx_synchronize())
        wall = (time.perf_counter() - t0) * 1e3
        stats = kernel_stats(pl)
        F.check(F.lib().plx_profile_enable(0))
    finally:
        for k in env:
            del os.environ[k]
    return out, wall, stats, pl.last_plan()


def summary(dev_ms, wall_ms, stats, plan):
    i0 = plan.find("Join{")
    return {"kernel_ms_median": round(float(np.median(dev_ms)), 4), "kernel_ms_min": round(float(np.min(dev_ms)), 4), "kernel_ms_max": round(float(np.max(dev_ms)), 4),
            "wall_ms_median": round(float(np.median(wall_ms)), 4),
            "kernels": {k: {"launches": v[0], "ms": round(v[1] / 1e3, 4), "bytes": v[2]} for k, v in sorted(stats.items())}, "plan": plan[i0:] if i0 >= 0 else plan}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", type=int, default=1 << 24)
    ap.add_argument("--build", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import polars_amd as pl
    pl.init(0)
    rng = np.random.default_rng(SEED)
    nb, npr = args.build, args.probe
    bid = rng.permutation(2 * nb)[:nb].astype(np.int64)             # unique build ids out of 2 * nb: about half of the probe rows match
    pid = rng.integers(0, 2 * nb, npr).astype(np.int64)
    matched = np.isin(pid, bid)
    row_of = np.full(2 * nb, -1, np.int64); row_of[bid] = np.arange(nb)
    want_l, want_r = np.nonzero(matched)[0], row_of[pid[matched]]

    def packable(i):        # id -> (Int32, Int64, Boolean), injective, spans 2^11 * (2 * nb / 2^12 + 1) * 2
        return [pl.Series("a", ((i >> 1) & 2047).astype(np.int32) - 1000), pl.Series("b", (i >> 12) * 1_000_003), pl.Series("c", (i & 1).astype(bool))]

    def full_range(i):      # id -> two full-range Int64 words
        u = i.astype(np.uint64)
        return [pl.Series("a", (u * MULT_A).view(np.int64)), pl.Series("b", ((u ^ np.uint64(0x5555)) * MULT_B).view(np.int64))]

    ok_all = True
    for case, enc, on, variants in (("packable_i32_i64_bool", packable, ["a", "b", "c"], (("packed", {}), ("wide", {"PLX_JOIN_WIDE_KEYS": "2"}))),
                                    ("two_full_range_i64", full_range, ["a", "b"], (("wide", {}),))):
        L = pl.DataFrame(enc(pid) + [pl.Series("lrow", np.arange(npr, dtype=np.uint32))])
        R = pl.DataFrame(enc(bid) + [pl.Series("rrow", np.arange(nb, dtype=np.uint32))])
        q = L.lazy().join(R.lazy(), on=on, maintain_order="left")
        for _, env in variants:
            for _ in range(args.warmup):
                timed_step(pl, q, env)
        dev = {v: [] for v, _ in variants}; wall = {v: [] for v, _ in variants}; last = {}
        for _ in range(args.steps):                                 # variants interleaved: one process, one device, the same clocks
            for v, env in variants:
                out, w, stats, plan = timed_step(pl, q, env)
                dev[v].append(sum(s[1] for s in stats.values()) / 1e3); wall[v].append(w)
                last[v] = (out, stats, plan)
        rec = {"tool": "wide_join_timing", "case": case, "probe_rows": npr, "build_rows": nb, "seed": SEED, "steps": args.steps, "warmup": args.warmup, "pairs": int(matched.sum())}
        for v, _ in variants:
            out, stats, plan = last[v]
            lrow, rrow = out["lrow"].to_numpy().astype(np.int64), out["rrow"].to_numpy().astype(np.int64)
            good = bool(len(lrow) == len(want_l) and np.array_equal(lrow, want_l) and np.array_equal(rrow, want_r))      # maintain_order=left + unique build keys: one order
            route_ok = ("wide_hash_join[" in plan) == (v == "wide") and ("packed " in plan) == (v == "packed")
            rec[v] = dict(summary(dev[v], wall[v], stats, plan), rows_equal_expected=good, route_ok=route_ok)
            ok_all = ok_all and good and route_ok
        if "packed" in rec and "wide" in rec:
            rec["wide_over_packed_kernel_ms"] = round(rec["wide"]["kernel_ms_median"] / max(rec["packed"]["kernel_ms_median"], 1e-9), 3)
        print(json.dumps(rec), flush=True)
        del L, R, q, last
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
