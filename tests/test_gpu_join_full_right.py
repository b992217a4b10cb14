"""Full and right joins and the coalesce option through the hash-join routes (kernels_join.hip / kernels_join_wide.hip: the count pass flags the build rows it
walks over, the unflagged rows are compacted and appended; kernels_join_order.hip orders the pair list; contract in include/polars_amd.h).
Ground truth, in the manner of test_gpu_join_order.py: both frames carry a row number (lrow, rrow) and outputs are compared UNSORTED.  The pair set is the CPU
oracle's LEFT join (orc.join(1, ...)) plus, for a full join, np.setdiff1d(all right rows, matched right rows); a right join is the oracle's left join with the
sides exchanged.  The set is put into the requested order with np.lexsort and a sentinel above any row number for "no row", which is exactly the contract (rows
without a row of the leading side last, in the other side's row order).  none / left / right: the row set plus the monotonicity the order promises; left_right /
right_left: row for row.  Every case runs through collect() and collect(no_fusion=True) and asserts its route through pl.last_plan()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASH_MULT = np.uint64(0x9E3779B97F4A7C15)
ORDERS = ("none", "left", "right", "left_right", "right_left")
NO_ROW = np.int64(1) << 40              # "no row" in the reference's sort keys: above any row number
BIG = (1 << 18) + 5                     # more than one block's scan carry, more than one 2048-row compaction tile
BLOCK_ROWS = 512                        # rows one workgroup of the build / count / emit kernels takes per grid step (kBlock * 2)
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def _hashed(v):
    return (np.asarray(v).astype(np.uint64) * HASH_MULT).astype(np.int64)


def _orders_for(how):
    return ORDERS if how == "full" else ("none", "right", "right_left")


# ------------------------------------------------------------------------------------------------------------------ inputs ---
def _sides(rng, n_left, n_right, matching="random", nulls=True):
    """hashed Int64 keys over a shared id space + payloads + validity (2-3 % null keys on both sides).  matching: "random" (about half of the shorter side's
    keys occur on the other), "all" (every row of the shorter side is matched), "disjoint" (no key in common), "dup_build" / "dup_probe" (about three rows per key on
    the shorter / longer side), "heavy" (one key holds a few per cent of both sides)."""
    nb, npr = min(n_left, n_right), max(n_left, n_right)
    ids = max(npr, 1) * 2
    if matching == "random":
        bid, pid = rng.permutation(ids)[:nb], rng.integers(0, ids, npr)
    elif matching == "all":
        bid = rng.permutation(ids)[:nb]
        pid = np.concatenate([bid, rng.integers(0, ids, npr - nb)])[rng.permutation(npr)] if npr else bid[:0]
    elif matching == "disjoint":
        bid, pid = rng.integers(0, ids, nb) * 2, rng.integers(0, ids, npr) * 2 + 1
    elif matching == "dup_build":
        bid, pid = rng.integers(0, max(nb // 3, 1), nb), rng.permutation(ids)[:npr] % max(nb, 1)
    elif matching == "dup_probe":
        bid, pid = rng.permutation(ids)[:nb] % max(npr // 3, 1), rng.integers(0, max(npr // 3, 1), npr)
    else:
        assert matching == "heavy"
        bid, pid = rng.permutation(ids)[:nb], rng.integers(0, ids, npr)
        bid[rng.random(nb) < 0.04] = 7
        pid[rng.random(npr) < 0.02] = 7
    lid, rid = (bid, pid) if n_left <= n_right else (pid, bid)          # (a tie builds on the left: join_indices)
    assert len(lid) == n_left and len(rid) == n_right
    return dict(lk=_hashed(lid), rk=_hashed(rid), lv=(rng.random(n_left) > 0.03) if nulls else None, rv=(rng.random(n_right) > 0.02) if nulls else None,
                lx=rng.integers(0, 100, n_left).astype(np.int32), ry=rng.integers(0, 50, n_right).astype(np.int32))


def _series(pl, name, v, valid):
    return pl.Series(name, v, validity=valid) if valid is not None else pl.Series(name, v)


def _frames(pl, h):
    L = pl.DataFrame([_series(pl, "k", h["lk"], h["lv"]), pl.Series("lrow", np.arange(len(h["lk"]), dtype=np.int64)), pl.Series("x", h["lx"])])
    R = pl.DataFrame([_series(pl, "k", h["rk"], h["rv"]), pl.Series("rrow", np.arange(len(h["rk"]), dtype=np.int64)), pl.Series("y", h["ry"])])
    return L, R


# --------------------------------------------------------------------------------------------------------------- reference ---
def _pairs(orc, how, lk, lv, rk, rv):
    """the pair set as (lrow or NO_ROW, rrow or NO_ROW), in no particular order"""
    if how == "right":
        ri, li, lvalid = orc.join(1, rk, rv, lk, lv)                    # the left join with the sides exchanged
        return np.where(lvalid, li.astype(np.int64), NO_ROW), ri.astype(np.int64)
    li, ri, rvalid = orc.join(1, lk, lv, rk, rv)
    l, r = li.astype(np.int64), np.where(rvalid, ri.astype(np.int64), NO_ROW)
    if how == "left":
        return l, r
    if how == "inner":
        return l[rvalid], r[rvalid]
    assert how == "full"
    extra = np.setdiff1d(np.arange(len(rk), dtype=np.int64), ri[rvalid].astype(np.int64))       # right rows no left row matched, null keys among them
    return np.concatenate([l, np.full(len(extra), NO_ROW)]), np.concatenate([r, extra])


def _idx(col):
    v, valid = col._download()
    return v.astype(np.int64) if valid is None else np.where(valid, v.astype(np.int64), NO_ROW)


def _check_rows(out, ref, h, order):
    lrow, rrow = ref
    g_l, g_r = _idx(out["lrow"]), _idx(out["rrow"])
    assert len(g_l) == len(lrow), (len(g_l), len(lrow))
    if order in ("left_right", "right_left"):
        o = np.lexsort((rrow, lrow)) if order == "left_right" else np.lexsort((lrow, rrow))
        assert np.array_equal(g_l, lrow[o]) and np.array_equal(g_r, rrow[o]), order         # row for row; "no row" of the leading side last
    else:
        if order in ("left", "right"):
            prim, sec = (g_l, g_r) if order == "left" else (g_r, g_l)
            assert np.all(np.diff(prim) >= 0), order + " row numbers are not non-decreasing (rows without one last)"
            assert np.all(np.diff(sec[prim == NO_ROW]) > 0), "the rows without a " + order + " row are not in the other side's row order"
        og, ow = np.lexsort((g_r, g_l)), np.lexsort((rrow, lrow))                              # the same row SET
        assert np.array_equal(g_l[og], lrow[ow]) and np.array_equal(g_r[og], rrow[ow]), order
    # the payload columns travelled with their rows, null where the side has no row
    for name, src, g in (("x", h["lx"], g_l), ("y", h["ry"], g_r)):
        v, valid = out[name]._download()
        has = g != NO_ROW
        assert np.array_equal(valid if valid is not None else np.ones(len(g), bool), has), name
        assert np.array_equal(v[has], src[g[has]]), name
    return g_l, g_r


def _check_key(col, want, want_valid):
    v, valid = col._download()
    valid = valid if valid is not None else np.ones(len(v), bool)
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(v[valid], want[valid])


def _side_key(k, kv, g):
    """(values, validity) of a side's key column gathered at the row numbers g (NO_ROW: null)"""
    has = g != NO_ROW
    at = np.where(has, g, 0)
    if len(k) == 0:
        return np.zeros(len(g), k.dtype), np.zeros(len(g), bool)
    return k[at], has & (kv[at] if kv is not None else True)


def _check_columns(out, h, how, coalesce, g_l, g_r, key="k"):
    """names and key values per the column rules of plx_ir.coalesce"""
    merge = (how != "full") if coalesce is None else coalesce
    lkv, lkm = _side_key(h["lk"], h["lv"], g_l)
    rkv, rkm = _side_key(h["rk"], h["rv"], g_r)
    if not merge:
        assert out.columns == [key, "lrow", "x", key + "_right", "rrow", "y"], out.columns
        _check_key(out[key], lkv, lkm)
        _check_key(out[key + "_right"], rkv, rkm)
    elif how == "right":
        assert out.columns == ["lrow", "x", key, "rrow", "y"], out.columns
        _check_key(out[key], rkv, rkm)
    else:
        assert out.columns == [key, "lrow", "x", "rrow", "y"], out.columns
        has_left = g_l != NO_ROW
        _check_key(out[key], np.where(has_left, lkv, rkv), np.where(has_left, lkm, rkm))


def _route(pl, how, build=None, wide=False):
    plan = pl.last_plan()
    assert "FusedJoinFrame{" not in plan and "FusedJoinGroupBy" not in plan and "Join{" in plan and "how=" + how in plan, plan
    name = ("wide_hash_full_join[" if wide else "hash_full_join[") if how == "full" else ("wide_hash_join[" if wide else "hash_join[")
    assert name in plan, plan
    assert ("unmatched build rows=" in plan) == (how == "full"), plan
    if build:
        assert "build=" + build + " rows=" in plan, plan
    return plan


def _run(pl, orc, h, hows=("full", "right"), orders=None, coalesce=None, build=None):
    L, R = _frames(pl, h)
    for how in hows:
        ref = _pairs(orc, how, h["lk"], h["lv"], h["rk"], h["rv"])
        for order in [o for o in (orders or ORDERS) if o in _orders_for(how)]:
            q = L.lazy().join(R.lazy(), on="k", how=how, maintain_order=order, coalesce=coalesce)
            for kw in ({}, {"no_fusion": True}):
                out = q.collect(**kw)
                plan = _route(pl, how, "left" if how == "right" else build)
                if not kw:
                    assert "(join not fused: full and right joins take the per-node route)" in plan, plan
                assert ("order=" in plan) == (order != "none") and (order == "none" or f"order={order}: " in plan), plan
                g_l, g_r = _check_rows(out, ref, h, order)
                _check_columns(out, h, how, coalesce, g_l, g_r)
                if how == "full":
                    tail = int(plan.split("unmatched build rows=")[1].split("]")[0])
                    built_left = "build=left rows=" in plan
                    assert tail == int(np.sum((g_r if built_left else g_l) == NO_ROW)), plan


# -------------------------------------------------------------------------------------------------------------------- sizes ---
@pytest.mark.parametrize("n_build", [0, 1, 63, 64, 65, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 2047, 2049, BIG])
def test_every_build_and_probe_size_on_both_build_sides(pl, orc, n_build):
    """the flag / ballot / compaction / append passes at the sizes where they can go wrong: empty sides, one row, around a wave, around a block, around a compaction
    tile, several blocks; the shorter side is the build side, so both "probe is left" and "probe is right" occur"""
    rng = np.random.default_rng(100 + n_build % 997)
    for n_probe in (0, 1, 65, BIG):
        if n_probe < n_build:
            continue
        for build in ("left", "right"):
            nl, nr = (n_build, n_probe) if build == "left" else (n_probe + (1 if n_probe == n_build else 0), n_build)      # the right side is built only when it is strictly shorter
            h = _sides(rng, nl, nr)
            _run(pl, orc, h, orders=("left_right", "right", "right_left"), build=build)


# ----------------------------------------------------------------------------------------------------------------- matching ---
@pytest.mark.parametrize("build", ["left", "right"])
@pytest.mark.parametrize("matching", ["all", "disjoint", "dup_build", "dup_probe", "heavy"])
def test_matching_shapes_in_every_order(pl, orc, matching, build):
    """empty tail, empty head, chains on the build side (flags set repeatedly), repeats on the probe side (several probe rows flag one build row), one heavy key (runs
    beyond the in-place run ordering): all five orders of a full join, the three of a right join"""
    rng = np.random.default_rng(7)
    nl, nr = (3_001, 20_003) if build == "left" else (20_003, 3_001)
    h = _sides(rng, nl, nr, matching, nulls=matching != "all")
    lrow, rrow = _pairs(orc, "full", h["lk"], h["lv"], h["rk"], h["rv"])
    both = int(np.sum((lrow != NO_ROW) & (rrow != NO_ROW)))
    if matching == "disjoint":
        assert both == 0 and len(lrow) == nl + nr
    if matching == "all":                                                              # (no null keys here: a null key would leave its build row unmatched)
        assert int(np.sum((lrow if build == "left" else rrow) == NO_ROW)) > 0          # unmatched probe rows exist (no row of the build side),
        assert int(np.sum((rrow if build == "left" else lrow) == NO_ROW)) == 0         # the tail of unmatched build rows is empty
    if matching == "heavy":
        assert both > 40 * 100
    _run(pl, orc, h, build=build)


def test_right_join_refuses_the_left_orders_and_names_the_option(pl):
    h = _sides(np.random.default_rng(12), 1000, 500)
    L, R = _frames(pl, h)
    for order in ("left", "left_right"):
        for kw in ({}, {"no_fusion": True}):
            with pytest.raises(pl.PlxError, match="maintain_order=" + order) as e:
                L.lazy().join(R.lazy(), on="k", how="right", maintain_order=order).collect(**kw)
            assert e.value.code == 3                                       # PLX_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------------------------------- coalesce ---
@pytest.mark.parametrize("how", ["full", "right", "inner", "left"])
@pytest.mark.parametrize("coalesce", [None, True, False])
def test_coalesce_column_lists_and_key_values(pl, orc, how, coalesce):
    h = _sides(np.random.default_rng(21), 5_003, 1_777, "dup_build")
    L, R = _frames(pl, h)
    ref = _pairs(orc, how, h["lk"], h["lv"], h["rk"], h["rv"])
    order = "right_left" if how == "right" else "left_right"
    q = L.lazy().join(R.lazy(), on="k", how=how, maintain_order=order, coalesce=coalesce)
    for kw in ({}, {"no_fusion": True}):
        out = q.collect(**kw)
        plan = pl.last_plan()
        assert "Join{" in plan and "how=" + how in plan and "FusedJoinFrame{" not in plan, plan
        assert ("coalesce=" in plan) == (coalesce is not None) and (coalesce is None or "coalesce=" + str(coalesce).lower() in plan), plan
        if not kw and coalesce is False and how in ("inner", "left"):
            assert "(join not fused: coalesce=false (both key columns kept) takes the per-node route)" in plan, plan
        g_l, g_r = _check_rows(out, ref, h, order)
        _check_columns(out, h, how, coalesce, g_l, g_r)
        assert list(q.collect_schema()) == out.columns


def test_coalesce_false_is_served_by_the_per_node_route_at_a_size_the_fused_join_takes(pl, orc, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    h = _sides(np.random.default_rng(22), 30_000, 4_000)
    L, R = _frames(pl, h)
    fused = L.lazy().join(R.lazy(), on="k", how="left", maintain_order="left_right").collect()
    assert "FusedJoinFrame{" in pl.last_plan(), pl.last_plan()
    out = L.lazy().join(R.lazy(), on="k", how="left", maintain_order="left_right", coalesce=False).collect()
    plan = pl.last_plan()
    assert "FusedJoinFrame{" not in plan and "coalesce=false (both key columns kept) takes the per-node route" in plan and "Join{" in plan, plan
    g_l, g_r = _check_rows(out, _pairs(orc, "left", h["lk"], h["lv"], h["rk"], h["rv"]), h, "left_right")
    _check_columns(out, h, "left", False, g_l, g_r)
    assert np.array_equal(_idx(fused["rrow"]), g_r)


# --------------------------------------------------------------------------------------------------------- multi-column keys ---
def _multi_frames(pl, names, lcols, rcols):
    nl, nr = len(lcols[0][0]), len(rcols[0][0])
    L = pl.DataFrame([_series(pl, n, v, m) for n, (v, m) in zip(names, lcols)] + [pl.Series("lrow", np.arange(nl, dtype=np.int64))])
    R = pl.DataFrame([_series(pl, n, v, m) for n, (v, m) in zip(names, rcols)] + [pl.Series("rrow", np.arange(nr, dtype=np.int64))])
    return L, R


def _run_multi(pl, orc, names, lcols, rcols, route):
    """full (all five orders; keep both and coalesce) and right joins on a multi-column key; route(plan, how) asserts the key route"""
    def oc(cols):
        return [((v.astype(np.uint8) if v.dtype == np.bool_ else v), m) for v, m in cols]
    lk, lv, rk, rv = orc.encode_key_rows(oc(lcols), oc(rcols))
    L, R = _multi_frames(pl, names, lcols, rcols)
    for how in ("full", "right"):
        lrow, rrow = _pairs(orc, how, lk, lv, rk, rv)
        for order in _orders_for(how):
            for coalesce in ((None, True) if order in ("left_right", "right_left") else (None,)):
                q = L.lazy().join(R.lazy(), on=list(names), how=how, maintain_order=order, coalesce=coalesce)
                for kw in ({}, {"no_fusion": True}):
                    out = q.collect(**kw)
                    route(pl.last_plan(), how)
                    g_l, g_r = _idx(out["lrow"]), _idx(out["rrow"])
                    assert len(g_l) == len(lrow)
                    if order in ("left_right", "right_left"):
                        o = np.lexsort((rrow, lrow)) if order == "left_right" else np.lexsort((lrow, rrow))
                        assert np.array_equal(g_l, lrow[o]) and np.array_equal(g_r, rrow[o]), (how, order)
                    else:
                        if order != "none":
                            prim, sec = (g_l, g_r) if order == "left" else (g_r, g_l)
                            assert np.all(np.diff(prim) >= 0) and np.all(np.diff(sec[prim == NO_ROW]) > 0), (how, order)
                        og, ow = np.lexsort((g_r, g_l)), np.lexsort((rrow, lrow))
                        assert np.array_equal(g_l[og], lrow[ow]) and np.array_equal(g_r[og], rrow[ow]), (how, order)
                    merge = (how != "full") if coalesce is None else coalesce
                    want_cols = (list(names) + ["lrow"] + [n + "_right" for n in names] + ["rrow"] if not merge else
                                 ["lrow"] + list(names) + ["rrow"] if how == "right" else list(names) + ["lrow", "rrow"])
                    assert out.columns == want_cols and list(q.collect_schema()) == want_cols, out.columns
                    has_left = g_l != NO_ROW
                    for n, (lvals, lm), (rvals, rm) in zip(names, lcols, rcols):
                        a, am = _side_key(lvals, lm, g_l)
                        b, bm = _side_key(rvals, rm, g_r)
                        cols = ((n, a, am), (n + "_right", b, bm)) if not merge else ((n, b, bm),) if how == "right" else ((n, np.where(has_left, a, b), np.where(has_left, am, bm)),)
                        for cname, want, wm in cols:
                            v, valid = out[cname]._download()
                            valid = valid if valid is not None else np.ones(len(v), bool)
                            assert np.array_equal(valid, wm), (how, order, cname)
                            assert np.array_equal(v[valid].view(np.uint64 if v.dtype.itemsize == 8 else v.dtype), want[wm].view(np.uint64 if want.dtype.itemsize == 8 else want.dtype)), (how, order, cname)


@pytest.mark.parametrize("build", ["left", "right"])
def test_packed_two_column_key(pl, orc, build):
    rng = np.random.default_rng(31)
    nl, nr = (2_500, 9_001) if build == "left" else (9_001, 2_500)
    def cols(n):
        return [(rng.integers(-40, 40, n).astype(np.int32), rng.random(n) > 0.03), (rng.integers(0, 60, n).astype(np.int64), rng.random(n) > 0.02)]
    def route(plan, how):
        assert "packed 2 key columns" in plan and ("hash_full_join[build=" + build if how == "full" else "hash_join[build=left") in plan and "wide_hash" not in plan, plan
    _run_multi(pl, orc, ("a", "b"), cols(nl), cols(nr), route)


@pytest.mark.parametrize("build", ["left", "right"])
@pytest.mark.parametrize("words", [2, 3])
def test_wide_keys(pl, orc, words, build):
    """key parts that do not pack: a Float64 part with NaNs of both signs and zeros of both signs, a full-range Int64 part (and a small Int16 part for words=3)"""
    rng = np.random.default_rng(40 + words)
    nl, nr = (2_500, 9_001) if build == "left" else (9_001, 2_500)
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    f_pool = np.array([np.nan, neg_nan, 0.0, -0.0, np.inf, 1.5, -2.25, 1e300])
    i_pool = np.concatenate([np.array([-1, 0, I64_MIN, I64_MAX], np.int64), rng.integers(I64_MIN, I64_MAX, 12, dtype=np.int64, endpoint=True)])
    def cols(n):
        c = [(f_pool[rng.integers(0, len(f_pool), n)], rng.random(n) > 0.03), (i_pool[rng.integers(0, len(i_pool), n)], rng.random(n) > 0.02)]
        if words == 3:
            c.append((rng.integers(-3, 3, n).astype(np.int16), None))
        return c
    def route(plan, how):
        assert ("wide_hash_full_join[words=%d" % words if how == "full" else "wide_hash_join[words=%d" % words) in plan and "packed" not in plan, plan
        assert ("build=" + (build if how == "full" else "left") + " rows=") in plan, plan
    _run_multi(pl, orc, ("f", "i", "s")[:words], cols(nl), cols(nr), route)


def test_wide_key_coalesce_reads_the_side_that_has_the_row(pl, orc):
    """-0.0 on the left and +0.0 on the right are one key: the coalesced column shows the LEFT bits where a left row exists"""
    L = pl.DataFrame([pl.Series("f", np.array([-0.0, 1.0, 5.0])), pl.Series("i", np.array([I64_MIN, 2, 3], np.int64)), pl.Series("lrow", np.arange(3, dtype=np.int64))])
    R = pl.DataFrame([pl.Series("f", np.array([0.0, 7.0])), pl.Series("i", np.array([I64_MIN, I64_MAX], np.int64)), pl.Series("rrow", np.arange(2, dtype=np.int64))])
    out = L.lazy().join(R.lazy(), on=["f", "i"], how="full", coalesce=True, maintain_order="left_right").collect()
    assert "wide_hash_full_join[words=2" in pl.last_plan(), pl.last_plan()
    assert _idx(out["lrow"]).tolist() == [0, 1, 2, NO_ROW] and _idx(out["rrow"]).tolist() == [0, NO_ROW, NO_ROW, 1]
    f = out["f"].to_numpy()
    assert f.tolist() == [0.0, 1.0, 5.0, 7.0] and np.signbit(f[0])
    assert out["i"].to_numpy().tolist() == [I64_MIN, 2, 3, I64_MAX]


# ------------------------------------------------------------------------------------------------------------------ queries ---
def test_head_over_an_ordered_full_join(pl, orc):
    h = _sides(np.random.default_rng(51), 4_000, 30_000, "dup_build")
    L, R = _frames(pl, h)
    lrow, rrow = _pairs(orc, "full", h["lk"], h["lv"], h["rk"], h["rv"])
    for order, o in (("left_right", np.lexsort((rrow, lrow))), ("right_left", np.lexsort((lrow, rrow)))):
        for kw in ({}, {"no_fusion": True}):
            out = L.lazy().join(R.lazy(), on="k", how="full", maintain_order=order).head(50).collect(**kw)
            assert "hash_full_join[" in pl.last_plan() and out.height == 50
            assert _idx(out["lrow"]).tolist() == lrow[o][:50].tolist() and _idx(out["rrow"]).tolist() == rrow[o][:50].tolist()


def test_group_by_over_a_full_join_is_not_fused_and_equals_numpy(pl, orc):
    h = _sides(np.random.default_rng(52), 40_000, 6_000, "dup_probe", nulls=True)
    L, R = _frames(pl, h)
    lrow, rrow = _pairs(orc, "full", h["lk"], h["lv"], h["rk"], h["rv"])
    has_l, has_r = lrow != NO_ROW, rrow != NO_ROW
    y = np.where(has_r, h["ry"][np.where(has_r, rrow, 0)], -1)                   # the group key: the right payload, null (-1 here) on left-only rows
    x = np.where(has_l, h["lx"][np.where(has_l, lrow, 0)], 0).astype(np.int64)
    for kw in ({}, {"no_fusion": True}):
        out = L.lazy().join(R.lazy(), on="k", how="full").group_by("y").agg(pl.col("x").sum().alias("sx"), pl.col("x").count().alias("cx"), pl.len().alias("n")).collect(**kw)
        plan = pl.last_plan()
        assert "FusedJoinGroupBy" not in plan and "hash_full_join[" in plan, plan
        if not kw:
            assert "full and right joins take the per-node route" in plan, plan
        gy, gv = out["y"]._download()
        gkey = np.where(gv, gy, -1) if gv is not None else gy
        o = np.argsort(gkey)
        keys = np.unique(y)
        assert gkey[o].tolist() == keys.tolist()
        assert out["n"].to_numpy()[o].tolist() == [int(np.sum(y == k)) for k in keys]
        assert out["cx"].to_numpy()[o].tolist() == [int(np.sum((y == k) & has_l)) for k in keys]
        sx, sv = out["sx"]._download()
        want_sx = np.array([int(np.sum(x[(y == k) & has_l])) for k in keys])
        assert np.array_equal((np.where(sv, sx, 0) if sv is not None else sx)[o], want_sx)


def test_keys_of_different_dtypes_keep_both_columns_and_the_schema_says_so(pl, orc):
    """Int32 against Int64 keys: lowering casts the left key, nothing coalesces on a right join or a coalescing full join, and collect_schema() names what comes out"""
    rng = np.random.default_rng(61)
    lk32, rk64 = rng.integers(0, 400, 900).astype(np.int32), rng.integers(0, 400, 300).astype(np.int64)
    L = pl.DataFrame([pl.Series("k", lk32), pl.Series("lrow", np.arange(900, dtype=np.int64))])
    R = pl.DataFrame([pl.Series("k", rk64), pl.Series("rrow", np.arange(300, dtype=np.int64))])
    for how, coalesce, order in (("right", None, "right_left"), ("full", True, "left_right")):
        lrow, rrow = _pairs(orc, how, lk32.astype(np.int64), None, rk64, None)
        o = np.lexsort((rrow, lrow)) if order == "left_right" else np.lexsort((lrow, rrow))
        q = L.lazy().join(R.lazy(), on="k", how=how, coalesce=coalesce, maintain_order=order)
        out = q.collect()
        assert out.columns == ["k", "lrow", "k_right", "rrow"] and list(q.collect_schema()) == out.columns, out.columns
        g_l, g_r = _idx(out["lrow"]), _idx(out["rrow"])
        assert np.array_equal(g_l, lrow[o]) and np.array_equal(g_r, rrow[o])
        _check_key(out["k"], *_side_key(lk32, None, g_l))
        _check_key(out["k_right"], *_side_key(rk64, None, g_r))


def test_a_boolean_key_column_coalesced_on_a_full_join_is_refused_by_name(pl):
    """the limit written at plx_ir.coalesce: the coalesced full-join key is built for 1 / 2 / 4 / 8-byte values; keeping both keys works"""
    L = pl.DataFrame([pl.Series("b", np.array([True, False, True])), pl.Series("i", np.array([1, 2, 3], np.int64)), pl.Series("lrow", np.arange(3, dtype=np.int64))])
    R = pl.DataFrame([pl.Series("b", np.array([True, True])), pl.Series("i", np.array([1, 9], np.int64)), pl.Series("rrow", np.arange(2, dtype=np.int64))])
    with pytest.raises(pl.PlxError, match="full join with coalesce") as e:
        L.lazy().join(R.lazy(), on=["b", "i"], how="full", coalesce=True).collect()
    assert e.value.code == 3                                               # PLX_ERR_UNSUPPORTED
    out = L.lazy().join(R.lazy(), on=["b", "i"], how="full", maintain_order="left_right").collect()
    assert out.columns == ["b", "i", "lrow", "b_right", "i_right", "rrow"] and _idx(out["lrow"]).tolist() == [0, 1, 2, NO_ROW] and _idx(out["rrow"]).tolist() == [0, NO_ROW, NO_ROW, 1]


def test_a_select_over_a_full_join_names_the_decline_reason_once(pl, orc):
    h = _sides(np.random.default_rng(71), 700, 2_000)
    L, R = _frames(pl, h)
    out = L.lazy().join(R.lazy(), on="k", how="full", maintain_order="left_right").select("lrow", "rrow", "y").collect()
    plan = pl.last_plan()
    assert plan.count("full and right joins take the per-node route") == 1 and "hash_full_join[" in plan, plan
    lrow, rrow = _pairs(orc, "full", h["lk"], h["lv"], h["rk"], h["rv"])
    o = np.lexsort((rrow, lrow))
    assert np.array_equal(_idx(out["lrow"]), lrow[o]) and np.array_equal(_idx(out["rrow"]), rrow[o])
