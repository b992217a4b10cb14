"""The 512-row wide tiles of the compiled aggregate scans over narrow rows (csrc/fused_sinks.hpp fused_scan_body<P, Sink, true>; csrc/kernels_fused.hip
wide_tiles_choice; DESIGN.md "Encoded shadows") -- against numpy.

Built like tests/test_gpu_scan_tiles.py, whose table and helpers it uses: every query runs three times (plain, building the shadows, reading them), all three results
are compared with numpy -- integers, counts and min / max exactly, f64 sums within RTOL = 1e-6 -- and the run-time compilation threshold is lowered to 0 rows for the
small sizes.  pl._ffi.last_scan_tile_rows() says which tile size the last aggregate scan ran with: the third run reads rows of at most 16 bytes without a nullable
input, so it takes 512-row tiles from 512 rows on (a wave then finishes the rows past the last whole wide tile in 128-row tiles, in the same kernel)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_encoded_inputs as T
import test_gpu_scan_tiles as S
from test_gpu_scan_tiles import compile_every_size  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
WIDE, NARROW = 512, 128
# no wide tile; exactly one; one and a full 128-row tile; one and a partial 128-row tile (one row short of / one row past a 128-row boundary); two; three less one row
AROUND = [0, 1, 511, 512, 513, 639, 640, 641, 1023, 1024, 1025, 1535]
# every wave runs at least three wide iterations at any number of workgroups per CU up to 8, and the tail is three full 128-row tiles and one row
LARGE = 3 * S.CUS * S.MAX_WG_PER_CU * S.WAVES_PER_WG * WIDE + 385
assert LARGE % WIDE == 385 and LARGE % NARROW == 1 and LARGE >= 1 << 22


def tile_rows(pl):
    return pl._ffi.last_scan_tile_rows()


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", AROUND)
def test_row_counts_around_the_wide_tile(pl, compile_every_size, n, keyed):
    S.run_three(pl, n, keyed)
    if n:
        assert tile_rows(pl) == (WIDE if n >= WIDE else NARROW), (n, tile_rows(pl))


@pytest.mark.parametrize("keyed", [True, False])
def test_every_wave_runs_three_wide_iterations_and_the_tail_ends_in_one_row(pl, keyed):
    S.run_three(pl, LARGE, keyed)
    assert tile_rows(pl) == WIDE, tile_rows(pl)


def test_switched_off_128_row_tiles_and_the_same_results_in_a_fresh_process():
    """PLX_WIDE_TILES=0 is read once: a process of its own.  The large table keyed, a small one without the key."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport polars_amd as pl\nimport test_gpu_scan_tiles as S\nimport test_gpu_wide_tiles as W\n"
            "pl.init(0)\nS.run_three(pl, W.LARGE, True)\nassert W.tile_rows(pl) == 128, W.tile_rows(pl)\n"
            "pl._ffi.jit_set_min_rows(0)\nS.run_three(pl, 1025, False)\nassert W.tile_rows(pl) == 128, W.tile_rows(pl)\nprint('narrow tiles every time')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLX_WIDE_TILES="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "narrow tiles every time" in r.stdout, r.stdout + r.stderr


# ---- the two ahead-of-time encoded Q1 shapes ----------------------------------------------------------------------------------------------
SHAPE_Q1_ENCODED, SHAPE_Q1_ENCODED_PRICE = 15, 16


@pytest.mark.parametrize("n", [513, 1025, 3 * (1 << 20) + 385])
@pytest.mark.parametrize("shape", [SHAPE_Q1_ENCODED, SHAPE_Q1_ENCODED_PRICE])
def test_encoded_q1_ahead_of_time_shapes(pl, shape, n):
    """15: the price stays an f64 column (15-byte rows); 16: the price is read through its four-byte decimal shadow (11-byte rows)"""
    from oracle import pyoracle as orc
    from polars_amd import datagen, queries
    F = pl._ffi
    li = datagen.lineitem_host(n, seed=41)
    want = orc.q1({k: li[k] for k in datagen.LINEITEM_Q1_COLS}, datagen.us(1998, 9, 2))
    flags = pl.datagen_categories("l_returnflag")
    before = F.encoded_decimal_min_rows()
    F.encoded_set_decimal_min_rows(0 if shape == SHAPE_Q1_ENCODED_PRICE else 1 << 40)
    try:
        df = datagen.to_frame(pl, li, datagen.LINEITEM_Q1_COLS)
        for run in range(3):
            g = queries.q1(df.lazy()).collect().sort_host(["l_returnflag", "l_linestatus"])
            assert "fused_scan[aot]" in pl.last_plan(), pl.last_plan()
            assert [flags.index(x) for x in g["l_returnflag"]] == want["l_returnflag"].tolist(), run
            for k in ("sum_qty", "count_order"):
                assert g[k] == want[k].tolist(), (run, k)
            for k in ("sum_base_price", "sum_disc_price", "sum_charge", "avg_qty", "avg_price", "avg_disc"):
                assert np.allclose(np.array(g[k]), want[k], rtol=T.RTOL, atol=0), (run, k)
        enc = T.encodings_in(pl.last_plan_encodings())
        assert ("l_extendedprice" in enc) == (shape == SHAPE_Q1_ENCODED_PRICE) and enc.get("l_shipdate") == "affine16", enc
        ok, sid, why, _ = queries.q1(df.lazy()).describe_fusion()
        assert ok and sid == shape, (ok, sid, why)
        assert tile_rows(pl) == WIDE, tile_rows(pl)
    finally:
        F.encoded_set_decimal_min_rows(before)


# ---- groups and lanes -----------------------------------------------------------------------------------------------------------------------
def keyed_three(pl, data, cols, what, tiles=WIDE):
    df = T.frame_of(pl, data)
    keep = data["day"][0] <= S.CUTOFF
    used = {"day"} | {name for name, _ in cols}
    T.three_runs(pl, df, data, cols, pl.col("day") <= S.CUTOFF, keep, True, {k: v for k, v in S.expected(data).items() if k in used}, what)
    assert "fused_scan[jit]" in pl.last_plan(), pl.last_plan()
    if tiles:
        assert tile_rows(pl) == tiles, (what, tile_rows(pl))
    return df


def test_every_group_in_every_lane_position(pl, compile_every_size):
    """key = row % 6 over a row count that is no multiple of 6: each of a lane's eight row positions meets every group, tile after tile at a different phase"""
    n = 5 * WIDE + 131
    assert n % 6 != 0 and WIDE % 6 != 0
    data = dict(S.table(n))
    data["g"] = ((np.arange(n) % 6).astype(np.uint8), None)
    keyed_three(pl, data, S.COLS, ("row % 6", n))


def test_every_row_in_one_group(pl, compile_every_size):
    """the hot cell: all 64 lanes of every LDS atomic of a pass add into one group's cells (16 copies of each)"""
    n = 5 * WIDE + 131
    data = dict(S.table(n))
    data["g"] = (np.full(n, 4, np.uint8), None)
    keyed_three(pl, data, S.COLS, ("one group", n))


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", [1025, 4 * WIDE + 129])
def test_a_nullable_input_keeps_the_128_row_tiles(pl, compile_every_size, n, keyed):
    cols = [("q", ("sum", "min", "max", "count")), ("d", ("sum",)), ("x", ("sum",))]
    S.run_three(pl, n, keyed, nulls=True, cols=cols)
    assert tile_rows(pl) == NARROW, tile_rows(pl)


# ---- pointers that are not aligned to eight rows ---------------------------------------------------------------------------------------------------
# (LazyFrame.slice always copies -- engine.cpp exec_slice -- so a sliced library column is aligned again; a column that borrows a torch tensor viewed from row
# `offset` on is read where it lies.)  The table is narrow as stored: u8 key, i16 predicate column, i32 and u8 values, 8 bytes a row, nothing to encode.
NARROW_N = 5 * WIDE + 131


def narrow_table(n):
    rng = np.random.default_rng(7000 + n)
    return {"g": rng.integers(0, 6, n).astype(np.uint8), "a": rng.integers(-50, 1000, n).astype(np.int16), "b": rng.integers(-100000, 100000, n).astype(np.int32),
            "c": rng.integers(0, 200, n).astype(np.uint8)}


def narrow_query(pl, df, keyed):
    c = pl.col
    aggs = [c("b").sum().alias("sb"), c("b").min().alias("nb"), c("c").max().alias("mc"), pl.len().alias("n")]
    lf = df.lazy().filter(c("a") > 3)
    return (lf.group_by("g").agg(*aggs) if keyed else lf.select(*aggs)).collect()


def narrow_check(out, host, keyed, what):
    keep = host["a"] > 3
    d = out.to_dict()
    got = {(int(d["g"][i]) if keyed else None): (int(d["sb"][i]), int(d["nb"][i]), int(d["mc"][i]), int(d["n"][i])) for i in range(len(d["n"]))}
    want = {}
    for k in (np.unique(host["g"][keep]) if keyed else [None]):
        rows = keep if k is None else keep & (host["g"] == k)
        want[None if k is None else int(k)] = (int(host["b"][rows].sum(dtype=np.int64)), int(host["b"][rows].min()), int(host["c"][rows].max()), int(rows.sum()))
    assert got == want, (what, got, want)


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("offset", [0, 1, 3, 7, 8])
def test_borrowed_columns_viewed_from_an_odd_row(pl, compile_every_size, offset, keyed):
    """Every column starts `offset` rows into its tensor (whose own start is aligned to 64 bytes or more): at 1, 3 and 7 no column pointer is aligned to eight rows
    and the launcher must take the 128-row kernel; at 0 and 8 every pointer is and the same query takes wide tiles.  The result is numpy's either way."""
    import torch
    full = narrow_table(NARROW_N + offset)
    tensors = {k: torch.from_numpy(v).cuda() for k, v in full.items()}
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 64 == 0 for t in tensors.values())
    host = {k: v[offset:] for k, v in full.items()}
    df = pl.DataFrame([pl.Series.from_torch(k, t[offset:]) for k, t in tensors.items()])
    for run in range(2):
        out = narrow_query(pl, df, keyed)
        assert "fused_scan[jit]" in pl.last_plan() and ("lds_table" if keyed else "register_sink") in pl.last_plan(), pl.last_plan()
        assert pl.last_plan_encodings() == "", pl.last_plan_encodings()      # borrowed buffers never encode: the rows are narrow as stored
        assert tile_rows(pl) == (WIDE if offset % 8 == 0 else NARROW), (offset, run, tile_rows(pl))
        narrow_check(out, host, keyed, ("borrowed", offset, keyed, run))


@pytest.mark.parametrize("keyed", [True, False])
def test_a_sliced_frame_is_a_copy_and_reads_plain_rows(pl, compile_every_size, keyed):
    """rows 3 .. of the shared table through LazyFrame.slice: the slice is materialised (aligned, eight-byte columns, no shadows), so the encoded path is never
    reached -- asserted from last_plan_encodings() -- rows are wider than 16 bytes and the scan keeps 128-row tiles; the alignment rule itself is the test above and
    tests/test_wide_tiles_cpu.py"""
    offset, n = 3, 3 * WIDE + 200
    full = S.table(n + offset)
    data = {k: (v[offset:], None) for k, (v, _) in full.items()}
    df = T.frame_of(pl, full)
    keep = data["day"][0] <= S.CUTOFF
    ref = T.reference(data, S.COLS, keep, data["g"][0] if keyed else None)
    for run in range(3):
        lf = df.lazy().slice(offset, n).filter(pl.col("day") <= S.CUTOFF)
        out = (lf.group_by("g").agg(*T.aggs_of(pl, S.COLS)) if keyed else lf.select(*T.aggs_of(pl, S.COLS))).collect()
        T.check(out, ref, keyed, ("slice", offset, keyed, run))
        assert pl.last_plan_encodings() == "", (run, pl.last_plan_encodings())
        assert tile_rows(pl) == NARROW, (run, tile_rows(pl))


# ---- copies of the LDS table (Params::copies): sixteen, or what fits --------------------------------------------------------------------------
def lds_copies(n_groups, n_aggs):
    """csrc/kernels_fused.hip lds_agg_copies"""
    c = 16
    while c > 1 and n_groups * n_aggs * c * 8 > 60 * 1024:
        c >>= 1
    return c


def plan_table(plan):
    """(G, copies, aggs) of the LDS table as the plan text names them: "lds_table(G=8,copies=16), inputs=7, ops=18, aggs=7" """
    import re
    m = re.search(r"lds_table\(G=(\d+),copies=(\d+)\).*?aggs=(\d+)", plan)
    assert m, plan
    return tuple(int(x) for x in m.groups())


COPIES_COLS = [("q", ("sum",)), ("d", ("sum",))]
COPIES_GROUPS = 200


@pytest.mark.parametrize("groups,copies", [(6, 16), (COPIES_GROUPS, 8)])
def test_sixteen_copies_or_eight(pl, compile_every_size, groups, copies):
    """Same query, same table but for the key.  Few groups: sixteen copies of every cell.  Many groups: the table the plan names fits the 60 KiB budget eight times,
    not sixteen times, and is added to the result with device atomics (more than 64 groups).  Every pass of a wide tile addresses its cells by the copy count, which
    is read back from the plan text and checked against the budget rule for the G and the aggregate count the plan names."""
    n = 7 * WIDE + 77
    rng = np.random.default_rng(groups)
    data = dict(S.table(n))
    g = rng.integers(0, groups, n).astype(np.uint8)
    g[:groups] = np.arange(groups)
    data["g"] = (g, None)
    keyed_three(pl, data, COPIES_COLS, ("copies", groups))
    G, got, n_aggs = plan_table(pl.last_plan())
    assert G >= groups and got == lds_copies(G, n_aggs), (G, got, n_aggs)
    assert got == copies, (G, got, n_aggs)
