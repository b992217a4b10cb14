"""One case of tests/test_gpu_shared_cells.py in a process of its own.  argv: the case name.

Every case is a filter + group_by on a u8 key through the LDS-table sink -- len, sum and mean of an integer column v, sum of an f64 column x -- at each of its row
counts, run-time compiled from 0 rows on.  The query runs three times with shared cells (plain, building the shadows, reading them), every result checked against
numpy, then once more with the switch off (pl._ffi.set_shared_cells(False)): integer outputs and the integer mean equal bit for bit between the two and equal numpy's,
f64 sums within RTOL, and pl._ffi.last_lds_cells() says how many cells a group held each time.  Prints OK."""
import os
import re
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polars_amd as pl  # noqa: E402
import test_gpu_encoded_inputs as T  # noqa: E402

ROWS = [511, 512, 513, 1025]
COLS = [("v", ("sum", "mean")), ("x", ("sum",))]
SHARED, PACKED_ONLY, UNSHARED = "count, sum and mean in one cell", "count and sum in one cell, the mean in its own", "one cell per aggregate"


def lds_copies(n_groups, cells):
    """csrc/kernels_fused.hip lds_agg_copies"""
    c = 16
    while c > 1 and n_groups * cells * c * 8 > 60 * 1024:
        c >>= 1
    return c


def base_table(n, seed):
    rng = np.random.default_rng(seed + n)
    return rng, {"g": (rng.integers(0, 6, n).astype(np.uint8), None), "p": (rng.integers(-50, 1000, n).astype(np.int16), None),
                 "v": (rng.integers(0, 256, n).astype(np.uint8), None), "x": (900.0 + 100000.0 * rng.random(n), None)}


def both_ends(rng, n, top, dtype=np.int64):
    code = rng.integers(0, top + 1, n).astype(dtype)
    code[:2] = 0, top
    return code


def case_table(case, n):
    rng, d = base_table(n, 9100)
    if case == "one_group":
        d["g"] = (np.full(n, 4, np.uint8), None)
    elif case == "row_mod_6":
        d["g"] = ((np.arange(n) % 6).astype(np.uint8), None)
    elif case == "group_fails_predicate":      # every row of group 3 fails p > 3: the group must be absent
        p = d["p"][0].copy()
        p[d["g"][0] == 3] = -7
        d["p"] = (p, None)
    elif case == "group_of_zeros":
        v = d["v"][0].copy()
        v[d["g"][0] == 2] = 0
        d["v"] = (v, None)
    elif case == "hundred_groups":             # G = 128 > 64: the table is added to the result with device atomics
        g = rng.integers(0, 100, n).astype(np.uint8)
        g[:100] = np.arange(100)
        d["g"] = (g, None)
    elif case == "eight_copies":               # G = 256 groups of two cells: eight copies fit the budget, sixteen do not
        g = rng.integers(0, 200, n).astype(np.uint8)
        g[:200] = np.arange(200)
        d["g"] = (g, None)
    elif case == "u8_all_255":
        d["v"] = (np.full(n, 255, np.uint8), None)
    elif case == "u16_all_65535":
        d["v"] = (np.full(n, 65535, np.uint16), None)
    elif case == "affine_base_5_stride_3":     # span > 65535: the shadow is u16 codes with stride gcd = 3
        d["v"] = (5 + 3 * both_ends(rng, n, 65535), None)
    elif case == "negative_base":
        d["v"] = (-7 + both_ends(rng, n, 255), None)
    elif case == "nullable_source":
        d["v"] = (d["v"][0], rng.random(n) < 0.9)
    elif case == "base_2_45":
        # (even offsets: every partial sum of up to 511 such values is an even number below 2^54, which a double holds exactly -- the f64 cell this case keeps is
        # then exact in any order of its atomics, and the mean can still be compared bit for bit)
        d["v"] = ((1 << 45) + 2 * both_ends(rng, n, 127), None)
    else:
        raise KeyError(case)
    return d


# case -> (row counts, what the last shared run holds, the encoding of v it reads or None)
CASES = {
    "one_group": (ROWS, SHARED, None), "row_mod_6": (ROWS, SHARED, None), "group_fails_predicate": (ROWS, SHARED, None), "group_of_zeros": (ROWS, SHARED, None),
    "hundred_groups": (ROWS, SHARED, None), "eight_copies": (ROWS, SHARED, None),
    "u8_all_255": (ROWS, SHARED, None), "u16_all_65535": (ROWS, SHARED, None), "affine_base_5_stride_3": (ROWS, SHARED, "affine16"),
    "negative_base": (ROWS, UNSHARED, "affine8"), "nullable_source": (ROWS, UNSHARED, None),
    # 511 rows in one workgroup: bits(511) + bits(511 * (2^45 + 255)) = 9 + 54 <= 64 packs, 511 * 2^45 >= 2^53 keeps the mean's f64 cell.  (From 512 rows on rule A
    # declines too -- 10 + 55 bits -- which is the unshared case above.)
    "base_2_45": ([511], PACKED_ONLY, "affine8"),
}


def bits_of(x):
    return struct.pack("<d", x) if isinstance(x, float) else x


def groups_of(out):
    d = out.to_dict()
    return {int(d["g"][i]): {k: d[k][i] for k in d if k != "g"} for i in range(len(d["n"]))}


def run_case(case, n):
    F = pl._ffi
    rows, holds, enc = CASES[case]
    data = case_table(case, n)
    df = T.frame_of(pl, data)
    keep = data["p"][0] > 3
    ref = T.reference(data, COLS, keep, data["g"][0])

    def query(what):
        out = df.lazy().filter(pl.col("p") > 3).group_by("g").agg(*T.aggs_of(pl, COLS)).collect()
        plan = pl.last_plan()
        assert "lds_table" in plan and "fused_scan[jit]" in plan, plan
        T.check(out, ref, True, (case, n, what))
        got = groups_of(out)
        for (key,), r in ref.items():      # the integer mean is exact: numpy's own bits
            if r["n"] and r["v_mean"] is not None:
                assert bits_of(got[key]["v_mean"]) == bits_of(r["v_mean"]), (case, n, what, key)
        return got, plan

    F.set_shared_cells(True)
    for run in range(3):
        shared, plan = query(("shared", run))
    assert T.encodings_in(pl.last_plan_encodings()).get("v") == enc, (case, n, pl.last_plan_encodings())
    G, n_aggs = (int(x) for x in re.search(r"lds_table\(G=(\d+),copies=\d+\).*?aggs=(\d+)", plan).groups())
    want = {SHARED: n_aggs - 2, PACKED_ONLY: n_aggs - 1, UNSHARED: n_aggs}[holds]
    assert F.last_lds_cells() == want, (case, n, holds, F.last_lds_cells(), n_aggs)
    if case == "eight_copies":
        assert (G, lds_copies(G, want), lds_copies(G, n_aggs)) == (256, 8, 4), (G, want, n_aggs)
    if case == "hundred_groups":
        assert G == 128
    F.set_shared_cells(False)
    plain, _ = query(("switched off", 0))
    assert F.last_lds_cells() == n_aggs, (case, n, F.last_lds_cells(), n_aggs)
    assert set(plain) == set(shared)
    for key in shared:
        for name in ("n", "v_sum", "v_mean"):
            assert bits_of(shared[key][name]) == bits_of(plain[key][name]), (case, n, key, name, shared[key][name], plain[key][name])
    if case == "group_fails_predicate":
        assert 3 not in shared and 3 in set(int(k) for k in data["g"][0])
    print(f"{case} n={n}: G={G} aggs={n_aggs} cells={want} ({holds}), off: {n_aggs}")


# ---- TPC-H Q1 through its two ahead-of-time shapes ----------------------------------------------------------------------------------------------
def run_q1(shape):
    from oracle import pyoracle as orc
    from polars_amd import datagen, queries
    F = pl._ffi
    n = 1025
    li = datagen.lineitem_host(n, seed=43)
    want = orc.q1({k: li[k] for k in datagen.LINEITEM_Q1_COLS}, datagen.us(1998, 9, 2))
    flags = pl.datagen_categories("l_returnflag")
    F.encoded_set_decimal_min_rows(0 if shape == 16 else 1 << 40)
    df = datagen.to_frame(pl, li, datagen.LINEITEM_Q1_COLS)

    def query(what):
        g = queries.q1(df.lazy()).collect().sort_host(["l_returnflag", "l_linestatus"])
        assert "fused_scan[aot]" in pl.last_plan(), pl.last_plan()
        assert [flags.index(x) for x in g["l_returnflag"]] == want["l_returnflag"].tolist(), what
        for k in ("sum_qty", "count_order"):
            assert g[k] == want[k].tolist(), (what, k)
        for k in ("sum_base_price", "sum_disc_price", "sum_charge", "avg_qty", "avg_price", "avg_disc"):
            assert np.allclose(np.array(g[k]), want[k], rtol=T.RTOL, atol=0), (what, k)
        return g

    F.set_shared_cells(True)
    for run in range(3):
        shared = query(("shared", run))
    ok, sid, why, _ = queries.q1(df.lazy()).describe_fusion()
    assert ok and sid == shape, (ok, sid, why)
    assert F.last_lds_cells() == 5 and F.last_scan_tile_rows() == 512, (F.last_lds_cells(), F.last_scan_tile_rows())
    F.set_shared_cells(False)
    plain = query(("switched off", 0))
    assert F.last_lds_cells() == 7, F.last_lds_cells()
    for k in ("sum_qty", "count_order", "avg_qty"):
        assert [bits_of(x) for x in shared[k]] == [bits_of(x) for x in plain[k]], k
    print(f"q1 shape {shape}: 5 cells, off: 7")


def main():
    case = sys.argv[1]
    pl.init(0)
    if case in ("q1_shape_15", "q1_shape_16"):
        run_q1(int(case[-2:]))
    else:
        pl._ffi.jit_set_min_rows(0)
        for n in CASES[case][0]:
            run_case(case, n)
    print("OK")


if __name__ == "__main__":
    main()
