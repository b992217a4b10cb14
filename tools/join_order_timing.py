#!/usr/bin/env python3
"""What join(maintain_order=...) costs: TPC-H Q3's two filtered tables (the inputs of bench.py's join_materialise_sf100 extra: same generator call, sizes and seed)
plus a row-number column per side, joined into a frame with maintain_order none / left / left_right / right, on the direct-address route and on the hashed-key
route.  Per case: warm-up, then --steps timed steps -- the median of the per-step sum of the library's HIP-event kernel times, and of the host wall time around
collect() -- the kernels that ran with their declared bytes (ProfileScope), and a check of the LAST step's result over all rows: the order on the host in O(n) and
the row set against the CPU oracle's pairs.  One JSON line on stdout.

    python tools/join_order_timing.py [--orders 150000000] [--steps 20] [--warmup 3] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SF100_ORDERS = 150_000_000
SEED = 10
HASHED_KEY_MULT = 0x9E3779B97F4A7C15 - (1 << 64)
ORDER_KERNELS = ("join_order_pack", "join_order_unpack", "join_order_runs", "sort_radix_count", "sort_radix_scatter_keys")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", type=int, default=SF100_ORDERS)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true", help="skip the row-set check against the CPU oracle (the order is still checked over all rows)")
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen, queries
    F = pl._ffi
    pl.init(0)
    date = queries.Q3_DATE
    c = pl.col
    O, L = datagen.orders_lineitem_native(pl, args.orders, SEED)
    nl, no = L.height, O.height
    L = pl.DataFrame([L[n] for n in L.columns] + [pl.Series("lrow", np.arange(nl, dtype=np.uint32))])
    O = pl.DataFrame([O[n] for n in O.columns] + [pl.Series("rrow", np.arange(no, dtype=np.uint32))])

    def host_pairs(Lf, Of):
        """the oracle's pair set over the filtered host columns, as original row numbers sorted by (lrow, rrow)"""
        from oracle import pyoracle as orc
        date_us = datagen.us(1995, 3, 15)                                   # queries.Q3_DATE in the columns' unit
        lmask = Lf["l_shipdate"].to_numpy().astype(np.int64) > date_us
        omask = (Of["o_orderdate"].to_numpy().astype(np.int64) < date_us) & ((Of["o_custkey"].to_numpy() % 5) == 0)
        lsel, osel = np.nonzero(lmask)[0], np.nonzero(omask)[0]
        li, ri, _ = orc.join(0, Lf["l_orderkey"].to_numpy()[lsel], None, Of["o_orderkey"].to_numpy()[osel], None)
        lrow, rrow = lsel[li].astype(np.int64), osel[ri].astype(np.int64)
        o = np.lexsort((rrow, lrow))
        return lrow[o], rrow[o]

    rows = []
    for route in ("direct", "hashed"):
        Lr, Or = L, O
        if route == "hashed":
            Or = O.with_columns((c("o_orderkey") * HASHED_KEY_MULT).alias("o_orderkey"))
            Lr = L.with_columns((c("l_orderkey") * HASHED_KEY_MULT).alias("l_orderkey"))
        want = None if args.no_oracle else host_pairs(Lr, Or)
        for order in ("none", "left", "left_right", "right"):
            o = Or.lazy().filter((c("o_orderdate") < date) & ((c("o_custkey") % 5) == 0))
            li = Lr.lazy().filter(c("l_shipdate") > date)
            q = li.join(o, left_on="l_orderkey", right_on="o_orderkey", maintain_order=order).select("l_orderkey", "o_orderdate", "o_shippriority", "l_extendedprice", "l_discount", "lrow", "rrow")
            for _ in range(args.warmup):
                q.collect()
            F.check(F.lib().plx_synchronize())
            dev_ms, wall_ms, stats, out = [], [], {}, None
            for _ in range(args.steps):
                out = None
                F.check(F.lib().plx_profile_clear()); F.check(F.lib().plx_profile_enable(1))
                t0 = time.perf_counter()
                out = q.collect()
                F.check(F.lib().plx_synchronize())
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                stats = kernel_stats(pl)
                F.check(F.lib().plx_profile_enable(0))
                dev_ms.append(sum(v[1] for v in stats.values()) / 1e3)
            plan = pl.last_plan()
            lrow, rrow = out["lrow"].to_numpy().astype(np.int64), out["rrow"].to_numpy().astype(np.int64)
            pairs = len(lrow)
            if order == "left":
                in_order = bool(np.all(lrow[1:] >= lrow[:-1]))
            elif order == "right":
                in_order = bool(np.all(rrow[1:] >= rrow[:-1]))
            elif order == "left_right":
                in_order = bool(np.all((lrow[1:] > lrow[:-1]) | ((lrow[1:] == lrow[:-1]) & (rrow[1:] > rrow[:-1]))))
            else:
                in_order = True
            same_set = None
            if want is not None:
                og = np.lexsort((rrow, lrow))
                same_set = bool(len(lrow) == len(want[0]) and np.array_equal(lrow[og], want[0]) and np.array_equal(rrow[og], want[1]))
            ordering = {k: {"launches": v[0], "ms": round(v[1] / 1e3, 4), "bytes": v[2]} for k, v in stats.items() if k in ORDER_KERNELS}
            ord_bytes = sum(v["bytes"] for v in ordering.values())
            i0, i1 = plan.find("order="), plan.find(", gather")
            rows.append({"route": route, "maintain_order": order, "kernel_ms_median": round(float(np.median(dev_ms)), 4), "wall_ms_median": round(float(np.median(wall_ms)), 4),
                         "kernel_ms_min": round(float(np.min(dev_ms)), 4), "kernel_ms_max": round(float(np.max(dev_ms)), 4), "pairs": pairs,
                         "ordering_kernels": ordering, "ordering_ms": round(sum(v["ms"] for v in ordering.values()), 4),
                         "ordering_bytes_per_pair": round(ord_bytes / max(pairs, 1), 2), "branch": plan[i0:i1] if i0 >= 0 else "",
                         "kernels": sorted(stats), "in_order": in_order, "same_rows_as_oracle": same_set, "ok": bool(in_order and same_set is not False)})
            del out
    print(json.dumps({"tool": "join_order_timing", "orders": no, "lineitem": nl, "seed": SEED, "steps": args.steps, "warmup": args.warmup,
                      "oracle_row_set_check": not args.no_oracle, "rows": rows}))
    return 0 if all(r["ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
