#!/usr/bin/env python3
"""What a full join costs next to the left join on the same inputs: --left rows x --right rows of hashed Int64 keys (unique on the right, about half of the right rows
matched by some left row), a row-number column per side, joined through the per-node route (no_fusion=True, so every case runs join_indices) as
    a left join, then a full join with maintain_order none / left_right / right.
--cases picks a subset (a tree without full joins runs --cases left).  Per case: warm-up, then --steps timed steps -- the median of the per-step sum of the library's
HIP-event kernel times and of the host wall time around collect() -- the kernels that ran with their declared bytes (ProfileScope), and a check of the LAST step's
result over all rows: the number of rows of each kind against numpy (np.isin over the keys) and the order on the host in O(n).  One JSON line on stdout.

    python tools/join_full_timing.py [--left 67108864] [--right 4194304] [--steps 20] [--warmup 3] [--cases left,full_none,full_left_right,full_right]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 10
HASH_MULT = np.uint64(0x9E3779B97F4A7C15)
NO_ROW = np.int64(1) << 40
CASES = {"left": ("left", "none"), "full_none": ("full", "none"), "full_left_right": ("full", "left_right"), "full_right": ("full", "right")}
FULL_KERNELS = ("join_unmatched_mask", "filter_tile_count", "filter_rowids", "join_append_unmatched")


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


def idx(col):
    v, valid = col._download()
    return v.astype(np.int64) if valid is None else np.where(valid, v.astype(np.int64), NO_ROW)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--left", type=int, default=1 << 26)
    ap.add_argument("--right", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    cases = [c for c in args.cases.split(",") if c]
    assert all(c in CASES for c in cases), cases

    import polars_amd as pl
    F = pl._ffi
    pl.init(0)
    rng = np.random.default_rng(SEED)
    nl, nr = args.left, args.right
    rid = rng.permutation(2 * nr).astype(np.uint64)[:nr]                   # unique right ids out of 2 * nr
    draw = rng.integers(0, nr, nl)                                         # a left row draws one of the first nr / 2 right rows, or an id no right row has:
    lid = np.where(draw < nr // 2, rid[np.minimum(draw, nr - 1)], (2 * nr + draw).astype(np.uint64))
    matched_right = int(np.isin(rid, lid).sum())                           # about half of the right rows are matched, by about half of the left rows
    matched_left = int(np.isin(lid, rid).sum())
    lk, rk = (lid * HASH_MULT).astype(np.int64), (rid * HASH_MULT).astype(np.int64)
    L = pl.DataFrame([pl.Series("k", lk), pl.Series("lrow", np.arange(nl, dtype=np.uint32)), pl.Series("x", rng.integers(0, 100, nl).astype(np.int32))])
    R = pl.DataFrame([pl.Series("k", rk), pl.Series("rrow", np.arange(nr, dtype=np.uint32)), pl.Series("y", rng.integers(0, 50, nr).astype(np.int32))])
    del lid, rid, lk, rk

    rows = []
    for case in cases:
        how, order = CASES[case]
        q = L.lazy().join(R.lazy(), on="k", how=how, maintain_order=order)
        for _ in range(args.warmup):
            q.collect(no_fusion=True)
        F.check(F.lib().plx_synchronize())
        dev_ms, wall_ms, stats, out = [], [], {}, None
        for _ in range(args.steps):
            out = None
            F.check(F.lib().plx_profile_clear()); F.check(F.lib().plx_profile_enable(1))
            t0 = time.perf_counter()
            out = q.collect(no_fusion=True)
            F.check(F.lib().plx_synchronize())
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            stats = kernel_stats(pl)
            F.check(F.lib().plx_profile_enable(0))
            dev_ms.append(sum(v[1] for v in stats.values()) / 1e3)
        plan = pl.last_plan()
        lrow, rrow = idx(out["lrow"]), idx(out["rrow"])
        both, left_only, right_only = int(np.sum((lrow != NO_ROW) & (rrow != NO_ROW))), int(np.sum(rrow == NO_ROW)), int(np.sum(lrow == NO_ROW))
        counts_ok = both == matched_left and left_only == nl - matched_left and right_only == (nr - matched_right if how == "full" else 0)
        if order == "left_right":
            in_order = bool(np.all((lrow[1:] > lrow[:-1]) | ((lrow[1:] == lrow[:-1]) & (rrow[1:] > rrow[:-1]))))
        elif order == "right":
            tail = rrow == NO_ROW
            in_order = bool(np.all(rrow[1:] >= rrow[:-1]) and np.all(np.diff(lrow[tail]) > 0))
        else:
            in_order = True
        i0 = plan.find("Join{")
        rows.append({"case": case, "how": how, "maintain_order": order, "kernel_ms_median": round(float(np.median(dev_ms)), 4), "kernel_ms_min": round(float(np.min(dev_ms)), 4),
                     "kernel_ms_max": round(float(np.max(dev_ms)), 4), "wall_ms_median": round(float(np.median(wall_ms)), 4), "rows_out": int(len(lrow)),
                     "pairs": both, "left_only": left_only, "right_only": right_only,
                     "kernels": {k: {"launches": v[0], "ms": round(v[1] / 1e3, 4), "bytes": v[2]} for k, v in sorted(stats.items())},
                     "full_join_kernels_ms": round(sum(v[1] for k, v in stats.items() if k in FULL_KERNELS) / 1e3, 4) if how == "full" else 0.0,
                     "plan": plan[i0:] if i0 >= 0 else plan, "in_order": in_order, "counts_match_numpy": bool(counts_ok), "ok": bool(in_order and counts_ok)})
        del out, lrow, rrow
    base = next((r["kernel_ms_median"] for r in rows if r["case"] == "left"), None)
    for r in rows:
        r["x_left_join"] = round(r["kernel_ms_median"] / base, 3) if base else None
    print(json.dumps({"tool": "join_full_timing", "left": nl, "right": nr, "matched_right_rows": matched_right, "seed": SEED, "steps": args.steps, "warmup": args.warmup, "rows": rows}))
    return 0 if all(r["ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
