"""The tail of the LDS-table group-by on the device (kernels_fused.hip groupby_tail_kernel, engine.cpp groupby_tail_finish; DESIGN.md 4.11 "One tail kernel").

Every case runs its query twice, with the switch on (pl._ffi.set_groupby_tail) and off, downloads every column with DataFrame._download_all (plx_frame_to_host: the
raw value and validity arrays) and compares the two results as rows sorted by key BIT FOR BIT, then with a numpy reference.  Switch on: plx_last_groupby_tail() == 1
and the download was served from the host mirrors (plx_last_download_mirrored() == 1); off: both 0.  pl.last_plan() is the same text in both runs.

Bit for bit between two runs asks that the f64 cells do not depend on the order of the scan's atomics, which changes from run to run with or without the tail: the
f64 inputs here are multiples of 1/8 below 128, so every sum of up to 8193 values or of their squares is exact in a double in any order (var / std sum differences
from a pivot, the mean of the first rows, which is no multiple of 1/8: the var / std case keeps a valid NaN among those rows, which makes the pivot 0).
TPC-H Q1 reads generated prices, whose sums are not exact: there the integer columns and avg_qty are compared bit for bit and the f64 sums against the oracle.

Tolerances of the numpy comparison (eps = 2^-52): sums are exact by construction (asserted equal); a mean is one division of two exact numbers (equal to numpy's);
var / std go through sums of d and d * d that are exact as well, leaving the few roundings of the finalisation (variance.hpp) against numpy's two-pass formula over
<= 8193 values with a condition number 1 + mean^2 / var < 5: a relative 8193 * 5 * eps < 1e-11 bounds both; the tests ask for 1e-10.

Not here: FIN_NARROW and an f32 mean -- the fused group-by compiler produces neither (narrow integers sum into Int64, Float32 columns are not read by fused scans);
the 1- and 2-byte element writes are covered by max of a UInt8 and min of a UInt16 column (FIN_MINMAX_I).  A table of one slot does not exist either: a key column
takes at least one bit, so the smallest table has two slots (the constant-key case below)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [1, 127, 128, 129, 511, 512, 513, 1025]
AGGS_A = [("vi", "sum"), ("x", "sum"), ("x", "mean"), ("vi", "mean"), ("vi", "min"), ("vi", "max")]
AGGS_B = [("x", "min"), ("x", "max"), ("x", "var"), ("x", "std"), ("b", "max"), ("w", "min")]


@pytest.fixture()
def F(pl):
    f = pl._ffi
    yield f
    f.set_groupby_tail(True)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def table(n, n_keys, seed=0, key_dtype=np.uint16):
    """key `g` cycles through 0 .. n_keys - 1 (every code present when n >= n_keys); vi: nullable i64; x: nullable f64, multiples of 1/8, one NaN; b: u8; w: u16.
    Group 1 (when there is one) has all of vi and x null."""
    rng = np.random.default_rng(7700 + seed + n)
    g = (np.arange(n) % n_keys).astype(key_dtype)
    vi = rng.integers(-1000, 1000, n).astype(np.int64)
    x = rng.integers(0, 1024, n).astype(np.float64) / 8.0
    if n > 5:
        x[5] = np.nan
    vi_valid = rng.random(n) < 0.9
    x_valid = rng.random(n) < 0.9
    vi_valid[g == 1] = False
    x_valid[g == 1] = False
    if n > 5 and g[5] != 1:
        x_valid[5] = True      # the NaN counts: the mean of the first rows is not finite, so var / std take the pivot 0 (Compiler::var_pivot) and d = x is exact
    return {"g": (g, None), "p": (np.full(n, 10, np.int16), None), "vi": (vi, vi_valid), "x": (x, x_valid),
            "b": (rng.integers(0, 256, n).astype(np.uint8), None), "w": (rng.integers(0, 65536, n).astype(np.uint16), None)}


def frame_of(pl, data):
    return pl.DataFrame([pl.Series(name, v, validity=valid) if valid is not None else pl.Series(name, v) for name, (v, valid) in data.items()])


def agg_exprs(pl, aggs):
    return [pl.len().alias("n")] + [getattr(pl.col(c), kind)().alias(f"{c}_{kind}") for c, kind in aggs]


# ---- the two runs -----------------------------------------------------------------------------------------------------------------------------------
def sorted_rows(out, cols, keys):
    """{column: (values, validity or None)} with the rows ordered by the key columns (a null key first)"""
    names = out.columns
    d = dict(zip(names, cols))
    n = out.height
    def key_of(i):
        return tuple((0, 0) if (d[k][1] is not None and not d[k][1][i]) else (1, d[k][0][i].item()) for k in keys)
    order = np.array(sorted(range(n), key=key_of), dtype=np.int64)
    return {c: (v[order], None if m is None else m[order]) for c, (v, m) in d.items()}


def run_both(pl, F, make_query, keys, tail_expected=True, mirrored_expected=True):
    res = {}
    for on in (True, False):
        F.set_groupby_tail(on)
        out = make_query().collect()
        plan = pl.last_plan()
        tail = F.last_groupby_tail()
        cols = out._download_all()
        mirrored = F.last_download_mirrored()
        res[on] = (out, plan, sorted_rows(out, cols, keys))
        assert tail == int(on and tail_expected), (on, tail, plan)
        assert mirrored == int(on and tail_expected and mirrored_expected), (on, mirrored, plan)
    (out1, plan1, rows1), (out0, plan0, rows0) = res[True], res[False]
    assert plan1 == plan0, (plan1, plan0)
    assert out1.columns == out0.columns and out1.height == out0.height and out1.schema == out0.schema, (out1, out0)
    for c in rows1:
        (v1, m1), (v0, m0) = rows1[c], rows0[c]
        assert v1.dtype == v0.dtype and v1.tobytes() == v0.tobytes(), (c, v1, v0)
        assert (m1 is None) == (m0 is None) and (m1 is None or np.array_equal(m1, m0)), (c, m1, m0)
    return out1, plan1, rows1


def table_slots(plan):
    return int(re.search(r"lds_table\(G=(\d+),", plan).group(1))


# ---- the numpy reference ----------------------------------------------------------------------------------------------------------------------------
def reference(data, keys, keep, aggs):
    """{key tuple (None = null): {name: value or None}}"""
    kcols = [data[k] for k in keys]
    members = {}
    for i in np.nonzero(keep)[0].tolist():
        members.setdefault(tuple(None if (m is not None and not m[i]) else v[i].item() for v, m in kcols), []).append(i)
    ref = {}
    for t, ii in members.items():
        ii = np.array(ii, dtype=np.int64)
        r = {"n": len(ii)}
        for c, kind in aggs:
            v, m = data[c]
            x = v[ii] if m is None else v[ii][m[ii]]
            name = f"{c}_{kind}"
            if kind == "sum":
                r[name] = float(x.sum()) if v.dtype == np.float64 else int(x.sum(dtype=np.int64))
            elif len(x) == 0:
                r[name] = None
            elif kind == "mean":
                r[name] = float(x.astype(np.float64).sum() / len(x))
            elif kind in ("min", "max"):
                if v.dtype == np.float64:      # NaN is ignored; all NaN -> NaN
                    o = x[~np.isnan(x)]
                    r[name] = float("nan") if len(o) == 0 else float(getattr(o, kind)())
                else:
                    r[name] = int(getattr(x, kind)())
            else:      # var / std, ddof = 1
                r[name] = None if len(x) < 2 else float(np.var(x, ddof=1) if kind == "var" else np.std(x, ddof=1))
        ref[t] = r
    return ref


def check_reference(rows, ref, keys, what):
    n = len(rows["n"][0])
    got = {}
    for i in range(n):
        t = tuple(None if (rows[k][1] is not None and not rows[k][1][i]) else rows[k][0][i].item() for k in keys)
        got[t] = {c: (None if (m is not None and not m[i]) else v[i].item()) for c, (v, m) in rows.items() if c not in keys}
    assert set(got) == set(ref), (what, sorted(got, key=str), sorted(ref, key=str))
    for t, r in ref.items():
        for name, want in r.items():
            g = got[t][name]
            if want is None:
                assert g is None, (what, t, name, g)
            elif isinstance(want, float) and np.isnan(want):
                assert g is not None and np.isnan(g), (what, t, name, g)
            elif name.endswith(("_var", "_std")):
                assert g is not None and abs(g - want) <= 1e-10 * abs(want), (what, t, name, g, want)
            else:
                assert g == want, (what, t, name, g, want)


def nan_sum_fix(data):
    """x sums and means with the NaN row in them are NaN in both; keep the reference simple: the NaN row is null for the sum / mean / var set"""
    x, m = data["x"]
    m = m.copy()
    m[np.isnan(x)] = False
    return {**data, "x": (x, m)}


# ---- row counts at the tile edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_row_counts_at_the_tile_edges(pl, F, n):
    """eight key codes, every final kind (two queries: a program holds 16 cells); 128- and 512-row tile edges.  The second set keeps the NaN row: min / max pass
    over it, var / std of its group are NaN on the device as in numpy."""
    for aggs, with_nan in ((AGGS_A, False), (AGGS_B, True)):
        data = table(n, 8) if with_nan else nan_sum_fix(table(n, 8))
        df = frame_of(pl, data)
        q = lambda: df.lazy().filter(pl.col("p") > 3).group_by("g").agg(*agg_exprs(pl, aggs))
        out, plan, rows = run_both(pl, F, q, ["g"])
        assert "lds_table(G=" in plan and table_slots(plan) <= 64, plan
        check_reference(rows, reference(data, ["g"], np.ones(n, bool), aggs), ["g"], (n, aggs[0]))


# ---- table sizes and occupancies ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 2, 8, 64, 128, 4096])
@pytest.mark.parametrize("occupancy", ["all", "slot0", "last", "every_other", "none"])
def test_table_sizes_and_occupancies(pl, F, n_keys, occupancy):
    """<= 64 slots: per-workgroup partials + partials_finish_kernel in front of the tail; more: the scan's atomics into the table.  4096 slots hold one cell (len)."""
    n = max(1025, 2 * n_keys + 1)
    data = nan_sum_fix(table(n, n_keys, seed=n_keys))
    g = data["g"][0]
    occ = {"all": np.ones(n, bool), "slot0": g == 0, "last": g == n_keys - 1, "every_other": g % 2 == 0, "none": np.zeros(n, bool)}[occupancy]
    data["p"] = (np.where(occ, 10, -7).astype(np.int16), None)
    df = frame_of(pl, data)
    aggs = [] if n_keys == 4096 else AGGS_A
    q = lambda: df.lazy().filter(pl.col("p") > 3).group_by("g").agg(*agg_exprs(pl, aggs))
    out, plan, rows = run_both(pl, F, q, ["g"])
    G = table_slots(plan)
    print(f"n_keys={n_keys} {occupancy}: G={G} groups={out.height}")
    assert G >= n_keys and (n_keys > 8 or G <= 64) and (n_keys < 128 or G > 64), plan
    assert out.height == len(np.unique(g[occ]))
    if occupancy == "none":      # (run_both compared the schema with the other path's)
        assert out.height == 0 and out.columns == ["g", "n"] + [f"{c}_{k}" for c, k in aggs]
    check_reference(rows, reference(data, ["g"], occ, aggs), ["g"], (n_keys, occupancy))


# ---- key forms ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_key_columns_a_nullable_key_and_a_boolean_key(pl, F):
    n = 1025
    data = nan_sum_fix(table(n, 5))
    rng = np.random.default_rng(5)
    data["h"] = (rng.integers(-3, 4, n).astype(np.int32), rng.random(n) < 0.8)      # nullable: the null group
    data["t"] = (rng.random(n) < 0.4, None)                                         # Boolean: values written through a ballot
    df = frame_of(pl, data)
    for keys in (["g", "h"], ["h"], ["t"], ["t", "h", "g"]):
        q = lambda: df.lazy().filter(pl.col("p") > 3).group_by(*keys).agg(*agg_exprs(pl, AGGS_A))
        out, plan, rows = run_both(pl, F, q, keys)
        assert "lds_table(G=" in plan, plan
        check_reference(rows, reference(data, keys, np.ones(n, bool), AGGS_A), keys, keys)
        if "h" in keys:
            assert rows["h"][1] is not None and not rows["h"][1].all(), "the null group"


# ---- Q1 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["plain", "encoded_15", "encoded_16"])
def test_q1_against_the_oracle(pl, F, orc, shape):
    from polars_amd import datagen, queries
    n = 1025
    li = datagen.lineitem_host(n, seed=43)
    want = orc.q1({k: li[k] for k in datagen.LINEITEM_Q1_COLS}, datagen.us(1998, 9, 2))
    flags = pl.datagen_categories("l_returnflag")
    old = F.encoded_decimal_min_rows()
    try:
        F.encoded_set_decimal_min_rows(0 if shape == "encoded_16" else 1 << 40)
        df = datagen.to_frame(pl, li, datagen.LINEITEM_Q1_COLS)
        results = {}
        for on in (True, False):
            F.set_groupby_tail(on)
            for run in range(1 if shape == "plain" else 3):      # plain, building the shadows, reading them
                out = queries.q1(df.lazy()).collect()
                plan, tail = pl.last_plan(), F.last_groupby_tail()
                g = out.sort_host(["l_returnflag", "l_linestatus"])
                assert tail == int(on) and F.last_download_mirrored() == int(on), (on, tail, plan)
                assert "fused_scan[aot]" in plan and "lds_table" in plan, plan
                assert [flags.index(x) for x in g["l_returnflag"]] == want["l_returnflag"].tolist()
                for k in ("sum_qty", "count_order"):
                    assert g[k] == want[k].tolist(), (on, k)
                for k in ("sum_base_price", "sum_disc_price", "sum_charge", "avg_qty", "avg_price", "avg_disc"):
                    assert np.allclose(np.array(g[k]), want[k], rtol=1e-6, atol=0), (on, k)
            results[on] = (g, plan, pl.last_plan_encodings())
        if shape != "plain":
            ok, sid, why, _ = queries.q1(df.lazy()).describe_fusion()
            assert ok and sid == int(shape[-2:]), (ok, sid, why)
            assert results[True][2] != "" and results[True][2] == results[False][2]
        assert results[True][1] == results[False][1]
        for k in ("l_returnflag", "l_linestatus", "sum_qty", "count_order", "avg_qty"):
            assert [np.float64(x).tobytes() if isinstance(x, float) else x for x in results[True][0][k]] == \
                   [np.float64(x).tobytes() if isinstance(x, float) else x for x in results[False][0][k]], k
    finally:
        F.encoded_set_decimal_min_rows(old)


# ---- conditions that decline -----------------------------------------------------------------------------------------------------------------------------
def test_maintain_order_takes_the_old_path_and_keeps_first_occurrence_order(pl, F):
    n = 1025
    data = nan_sum_fix(table(n, 8))
    rng = np.random.default_rng(3)
    g = rng.permutation(np.arange(n) % 8).astype(np.uint16)
    data["g"] = (g, None)
    data["vi"][1][:] = rng.random(n) < 0.9
    data["x"][1][:] = ~np.isnan(data["x"][0]) & (rng.random(n) < 0.9)
    df = frame_of(pl, data)
    q = lambda: df.lazy().filter(pl.col("p") > 3).group_by("g", maintain_order=True).agg(*agg_exprs(pl, AGGS_A))
    out, plan, rows = run_both(pl, F, q, ["g"], tail_expected=False)
    assert "lds_table(G=" in plan, plan
    first = [int(k) for k in g[np.sort(np.unique(g, return_index=True)[1])]]
    F.set_groupby_tail(True)
    assert q().collect()["g"].to_numpy().tolist() == first and F.last_groupby_tail() == 0
    check_reference(rows, reference(data, ["g"], np.ones(n, bool), AGGS_A), ["g"], "maintain_order")


def test_an_expression_over_two_aggregates_has_no_mirror(pl, F):
    n = 1025
    data = nan_sum_fix(table(n, 8))
    data["vi"] = (data["vi"][0], None)
    df = frame_of(pl, data)
    c = pl.col
    q = lambda: df.lazy().filter(c("p") > 3).group_by("g").agg((c("x").sum() / c("b").sum()).alias("ratio"), c("vi").sum().alias("vi_sum"))
    out, plan, rows = run_both(pl, F, q, ["g"], mirrored_expected=False)
    x, m = data["x"]
    for i, k in enumerate(rows["g"][0].tolist()):
        sel = data["g"][0] == k
        assert rows["ratio"][0][i] == x[sel & m].sum() / float(data["b"][0][sel].sum(dtype=np.int64)), k      # exact sums, one division
        assert rows["vi_sum"][0][i] == data["vi"][0][sel].sum()
    # the columns that ARE aggregates keep their mirrors: a download of those alone is served from them
    F.set_groupby_tail(True)
    out = q().collect()
    assert np.array_equal(np.sort(out["vi_sum"].to_numpy()), np.sort(rows["vi_sum"][0])) and F.last_download_mirrored() == 1
    out["ratio"].to_numpy()
    assert F.last_download_mirrored() == 0


# ---- mirror coherence --------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_equals_device_and_derived_columns_have_none(pl, F):
    n = 1025
    data = nan_sum_fix(table(n, 64))
    data["vi"] = (data["vi"][0], None)
    data["x"] = (np.where(np.isnan(data["x"][0]), 1.0, data["x"][0]), None)
    df = frame_of(pl, data)
    aggs = [("vi", "sum"), ("x", "sum"), ("b", "max"), ("w", "min"), ("x", "mean")]
    F.set_groupby_tail(True)
    out = df.lazy().filter(pl.col("p") > 3).group_by("g").agg(*agg_exprs(pl, aggs)).collect()
    assert F.last_groupby_tail() == 1 and out.height == 64
    host = {}
    for name in out.columns:
        s = out[name]
        assert s.null_count() == 0, name
        host[name] = s.to_numpy()
        assert F.last_download_mirrored() == 1, name
        dev = s.to_torch().cpu().numpy()
        assert host[name].tobytes() == dev.tobytes(), name      # (to_torch reinterprets unsigned as signed: the bytes are what is compared)
    assert host["g"].tolist() == list(range(64))                # ascending slot order
    # derived frames: correct values, no mirror
    idx = pl.Series("i", np.array([63, 0, 7, 7], dtype=np.uint32))
    assert out["vi_sum"].gather(idx).to_numpy().tolist() == host["vi_sum"][[63, 0, 7, 7]].tolist() and F.last_download_mirrored() == 0
    sl = out.slice(5, 9)
    assert sl["g"].to_numpy().tolist() == list(range(5, 14)) and F.last_download_mirrored() == 0
    assert sl["x_sum"].to_numpy().tobytes() == host["x_sum"][5:14].tobytes()
    so = out.sort("w_min", descending=True)
    order = np.argsort(-host["w_min"].astype(np.int64), kind="stable")
    assert sorted(so["w_min"].to_numpy().tolist(), reverse=True) == so["w_min"].to_numpy().tolist() and F.last_download_mirrored() == 0
    assert so["w_min"].to_numpy().tolist() == host["w_min"][order].tolist()
    d = so._download_all()
    assert F.last_download_mirrored() == 0 and sorted(d[0][0].tolist()) == list(range(64))
    # the source frame is untouched by all of that
    assert out["g"].to_numpy().tolist() == list(range(64)) and F.last_download_mirrored() == 1


# ---- bounds nobody measured -----------------------------------------------------------------------------------------------------------------------------------
def test_declared_key_bounds_violated_by_one_row(pl, F):
    """plx_column_set_bounds declares 0 .. 7 for the key (tests/test_gpu_queries.py declares bounds the same way); one row holds 200: the table sink raises its flag,
    which the tail kernel carries in the block's header -- an error return, the same class and message either way"""
    n = 1025
    data = nan_sum_fix(table(n, 8))
    g = data["g"][0].astype(np.int64)
    g[700] = 200
    messages = []
    for on in (True, False):
        F.set_groupby_tail(on)
        key = pl.Series("g", g)
        F.check(F.lib().plx_column_set_bounds(key._h, 0, 7))
        df = pl.DataFrame([key] + [pl.Series(name, v, validity=m) if m is not None else pl.Series(name, v) for name, (v, m) in data.items() if name != "g"])
        with pytest.raises(pl.PlxError) as e:
            df.lazy().filter(pl.col("p") > 3).group_by("g").agg(*agg_exprs(pl, AGGS_A)).collect()
        messages.append((type(e.value), str(e.value)))
        # the same frame without the stray row's lie: bounds that hold
        key2 = pl.Series("g", np.where(g == 200, 3, g))
        F.check(F.lib().plx_column_set_bounds(key2._h, 0, 7))
        df2 = pl.DataFrame([key2] + [df[c] for c in df.columns if c != "g"])
        out = df2.lazy().filter(pl.col("p") > 3).group_by("g").agg(*agg_exprs(pl, AGGS_A)).collect()
        assert out.height == 8 and F.last_groupby_tail() == int(on) and "lds_table" in pl.last_plan()
    assert messages[0] == messages[1] and "group key outside the bounds declared or assumed for its column" in messages[0][1], messages


def test_assumed_key_bounds_violated_run_again(pl, F):
    """2^24 rows and more: the planner assumes the key's bounds from a strided sample (tests/test_gpu_datagen.py builds the same input); six rows the sample does not
    look at lie outside them, the flag comes back through the block's header and the query runs again from exact statistics -- the note is in the plan either way"""
    from test_gpu_datagen import _outside_the_sample
    rng = np.random.default_rng(13)
    n = 17_000_000
    ids = rng.integers(0, 3000, n).astype(np.int64)
    ids[_outside_the_sample(n)] = 5000 + np.arange(6)
    keys, counts = np.unique(ids, return_counts=True)
    plans = []
    for on in (True, False):
        F.set_groupby_tail(on)
        df = pl.DataFrame({"key": ids})      # a fresh column: nothing is known or remembered about it
        out = df.lazy().group_by("key").agg(pl.len().alias("n")).collect()
        plan = pl.last_plan()
        plans.append(plan)
        assert "AssumedBoundsViolated{" in plan, plan      # (the text of the attempt that raised is not kept; the second run's range needs 13 bits: another route)
        k = out["key"].to_numpy()
        o = np.argsort(k)
        assert np.array_equal(k[o], keys) and np.array_equal(out["n"].to_numpy()[o], counts)
    assert plans[0] == plans[1]
