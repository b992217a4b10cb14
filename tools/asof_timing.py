#!/usr/bin/env python3
"""What join_asof costs, and whether the LDS sample stage of its search pays.

--left left rows against each of --right right rows; no `by`, and one Int32 `by` of --groups values; the right side in (by, on) order and shuffled; the left side
sorted and shuffled; `on` Int64.  Every shape runs on the default route (the samples in LDS) and with PLX_ASOF_ROUTE=global (the whole search in global memory),
the two interleaved step by step in one process.  Per shape and route: median / minimum / maximum over --steps steps of the library's HIP-event kernel times and
of the wall time of plx_join_asof_indices, the kernel times of one more step split by kernel name (the sort's share when the right side is unordered), the plan
text.  The two routes' index columns must be equal, and --check sampled left rows are held against tests/asof_ref.py's loop over their group.  One JSON line.

    python tools/asof_timing.py [--left 100000000] [--right 1000000,100000000] [--groups 10000] [--steps 5] [--warmup 1] [--check 12]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cumulative_timing import split_by_kernel  # noqa: E402
from when_then_timing import timed  # noqa: E402

SEED = 41


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--left", type=int, default=100_000_000)
    ap.add_argument("--right", type=str, default="1000000,100000000")
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=12)
    args = ap.parse_args()

    import polars_amd as pl
    from polars_amd import datagen
    from tests import asof_ref as A
    F = pl._ffi
    pl.init(0)
    n = args.left
    span = 1 << 40
    out = {"left_rows": n, "groups": args.groups, "steps": args.steps, "shapes": []}
    rng = np.random.default_rng(SEED)

    def side(rows, stream, ordered, with_by):
        on = datagen.uniform_native(pl, "on", pl.Int64, rows, SEED, stream, 0, span)
        by = datagen.uniform_native(pl, "by", pl.UInt32, rows, SEED, stream + 1, 0, args.groups).cast(pl.Int32).rename("by") if with_by else None
        df = pl.DataFrame([on] if by is None else [by, on])
        if ordered:
            df = df.sort("on") if by is None else df.sort("by", "on")
        return df

    def call(L, R, with_by):
        h = C.c_uint64()
        lb = (C.c_uint64 * 1)(L["by"]._h if with_by else 0)
        rb = (C.c_uint64 * 1)(R["by"]._h if with_by else 0)
        F.check(F.lib().plx_join_asof_indices(F.ASOF_BACKWARD, lb, rb, 1 if with_by else 0, L["on"]._h, R["on"]._h, None, C.byref(h)))
        return pl.Series._from_handle("idx", h.value)

    for m in [int(x) for x in args.right.split(",")]:
        for with_by in (False, True):
            for right_ordered in (True, False):
                R = side(m, 0, right_ordered, with_by)
                ro = R["on"].to_numpy()
                rb = R["by"].to_numpy() if with_by else None
                whole = None if with_by else (np.arange(m) if right_ordered else np.argsort(ro, kind="stable"))      # candidate order without `by`: (on, right row)
                whole_on = None if with_by else ro[whole]
                for left_ordered in (True, False):
                    L = side(n, 2, left_ordered, with_by)
                    shape = {"right_rows": m, "by": int(with_by), "right": "in order" if right_ordered else "shuffled", "left": "sorted" if left_ordered else "shuffled", "routes": {}}
                    got, steps = {}, {}
                    for route in ("lds", "global"):
                        def step(route=route):
                            os.environ["PLX_ASOF_ROUTE"] = route                  # read per call
                            got[route] = call(L, R, with_by)
                        steps[route] = step
                    # interleaved: one step of each route in turn, so that both see the same clocks and the same cache history
                    def both():
                        steps["lds"](); steps["global"]()
                    for _ in range(args.warmup):
                        both()
                    per = {"lds": [], "global": []}
                    for _ in range(args.steps):
                        for route in ("lds", "global"):
                            r = timed(F, steps[route], 1, 0)
                            per[route].append((r["kernel"]["median_ms"], r["wall"]["median_ms"]))
                    for route in ("lds", "global"):
                        k, w = np.array([p[0] for p in per[route]]), np.array([p[1] for p in per[route]])
                        by_kernel = split_by_kernel(F, steps[route])
                        search = sum(v for name, v in by_kernel.items() if name.startswith("asof_search"))
                        shape["routes"][route] = {"kernel_ms": {"median": round(float(np.median(k)), 4), "min": round(float(k.min()), 4), "max": round(float(k.max()), 4)},
                                                  "wall_ms": {"median": round(float(np.median(w)), 4), "min": round(float(w.min()), 4), "max": round(float(w.max()), 4)},
                                                  "by_kernel_ms": by_kernel, "search_ms": round(search, 4), "sort_share": round(1.0 - (search + by_kernel.get("asof_encode", 0.0) +
                                                  by_kernel.get("asof_order_check", 0.0)) / max(sum(by_kernel.values()), 1e-9), 4), "plan": pl.last_plan()[:300]}
                    a, av = got["lds"]._download()
                    b, bv = got["global"]._download()
                    assert np.array_equal(a if av is None else a[av], b if bv is None else b[bv]) and ((av is None) == (bv is None)) and (av is None or np.array_equal(av, bv)), "the two routes differ"
                    # a sample of left rows against the loop over their group
                    lo = L["on"].to_numpy()
                    lb = L["by"].to_numpy() if with_by else None
                    for i in rng.integers(0, n, args.check).tolist():
                        rows, vals = whole, whole_on
                        if with_by:
                            rows = np.flatnonzero(rb == lb[i])
                            rows = rows[np.argsort(ro[rows], kind="stable")]
                            vals = ro[rows]
                        k = int(np.searchsorted(vals, lo[i], "right"))
                        near = [(int(ro[j]), int(j)) for j in rows[max(k - 3, 0):k + 3]]
                        want = A.match_row(int(lo[i]), near, "backward")
                        have = int(a[i]) if (av is None or av[i]) else None
                        assert have == want, (shape, i, have, want)
                    shape["checked_rows"] = args.check
                    out["shapes"].append(shape)
                    del L, got
                del R, ro, rb, whole, whole_on
    os.environ.pop("PLX_ASOF_ROUTE", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
