"""Joins honour maintain_order (plx_join_order, include/polars_amd.h; JoinArgs::maintain_order of the reference): the pair list is put into the requested order on
the device (kernels_join_order.hip) before the gathers.  Ground truth: the PAIR SET of the CPU oracle (orc.join), put into the requested order by numpy
(np.lexsort((secondary, primary)); the oracle's own order depends on the side it builds on and is not relied on).  Both frames carry a row-number column (lrow,
rrow), so the order is visible in the output, and outputs are compared UNSORTED.  Every route is asserted through pl.last_plan()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASH_MULT = np.uint64(0x9E3779B97F4A7C15)
ORDERS = ("none", "left", "right", "left_right", "right_left")
NO_RIGHT = np.int64(1) << 40            # stands for "no right row" in the reference's sort key: one pair per unmatched left row, so it never ties


def _hashed(v):
    return (v.astype(np.uint64) * HASH_MULT).astype(np.int64)


def _dense(v):
    return v.astype(np.int64) * 3 + 11


def _sides(rng, n_left, n_right, enc, dup_right=False, left="random", nulls=True):
    """left / right key columns over a shared id space, payloads, validity.  The right keys are unique (half of the id space) or, dup_right, about three rows per key;
    left = "random" (any id, repeats), "unique" or "dup" (about three rows per key)."""
    ids = max(n_left, n_right, 1) * 2
    def keys(n, dup):
        return rng.integers(0, max(n // 3, 1), n) if dup else rng.permutation(ids)[:n]
    lid = rng.integers(0, ids, n_left) if left == "random" else keys(n_left, left == "dup")
    rid = keys(n_right, dup_right)
    return dict(lk=enc(lid), rk=enc(rid), lv=(rng.random(n_left) > 0.03) if nulls else None, rv=(rng.random(n_right) > 0.02) if nulls else None,
                lx=rng.integers(0, 100, n_left).astype(np.int32), ry=rng.integers(0, 50, n_right).astype(np.int32))


def _frames(pl, h):
    def key(name, v, valid):
        return pl.Series(name, v, validity=valid) if valid is not None else pl.Series(name, v)
    L = pl.DataFrame([key("k", h["lk"], h["lv"]), pl.Series("lrow", np.arange(len(h["lk"]), dtype=np.int64)), pl.Series("x", h["lx"])])
    R = pl.DataFrame([key("k", h["rk"], h["rv"]), pl.Series("rrow", np.arange(len(h["rk"]), dtype=np.int64)), pl.Series("y", h["ry"])])
    return L, R


def _reference(orc, h, how, lmask=None, rmask=None, lk=None, rk=None):
    """the oracle's pair set as (lrow, rrow, rvalid) over the ORIGINAL row numbers, in no particular order"""
    lk = h["lk"] if lk is None else lk
    rk = h["rk"] if rk is None else rk
    lsel = np.nonzero(lmask)[0] if lmask is not None else np.arange(len(lk))
    rsel = np.nonzero(rmask)[0] if rmask is not None else np.arange(len(rk))
    lv = h["lv"][lsel] if h["lv"] is not None else None
    rv = h["rv"][rsel] if h["rv"] is not None else None
    li, ri, rvalid = orc.join(1 if how == "left" else 0, lk[lsel], lv, rk[rsel], rv)
    if rvalid is None:
        rvalid = np.ones(len(li), bool)
    lrow = lsel[li].astype(np.int64)
    rrow = np.where(rvalid, rsel[np.where(rvalid, ri, 0)] if len(rsel) else 0, NO_RIGHT).astype(np.int64)
    return lrow, rrow, rvalid


def _got(out):
    lrow = out["lrow"].to_numpy().astype(np.int64)
    rrow, rv = out["rrow"]._download()
    y, yv = out["y"]._download()
    n = out.height
    rv = rv if rv is not None else np.ones(n, bool)
    yv = yv if yv is not None else np.ones(n, bool)
    assert np.array_equal(rv, yv)
    return lrow, np.where(rv, rrow.astype(np.int64), NO_RIGHT), rv, out["x"].to_numpy(), np.where(yv, y, 0)


def _check(out, ref, h, order):
    lrow, rrow, rvalid = ref
    g_l, g_r, g_v, g_x, g_y = _got(out)
    assert len(g_l) == len(lrow), (len(g_l), len(lrow))
    if order in ("left_right", "right_left"):
        o = np.lexsort((rrow, lrow)) if order == "left_right" else np.lexsort((lrow, rrow))
        assert np.array_equal(g_l, lrow[o]), order                         # row for row, nulls of a left join at their left position
        assert np.array_equal(g_v, rvalid[o]) and np.array_equal(g_r, rrow[o]), order
    else:
        if order == "left":
            assert np.all(np.diff(g_l) >= 0), "left row numbers are not non-decreasing"
        if order == "right":
            assert np.all(np.diff(g_r) >= 0), "right row numbers are not non-decreasing"
        og, ow = np.lexsort((g_r, g_l)), np.lexsort((rrow, lrow))             # the same row SET
        assert np.array_equal(g_l[og], lrow[ow]) and np.array_equal(g_r[og], rrow[ow]) and np.array_equal(g_v[og], rvalid[ow]), order
    # the payload columns travelled with their rows
    assert np.array_equal(g_x, h["lx"][g_l])
    assert np.array_equal(g_y, np.where(g_v, h["ry"][np.where(g_v, g_r, 0)] if len(h["ry"]) else 0, 0))


def _orders_for(how):
    return ORDERS if how == "inner" else ("none", "left", "left_right")


def _run_all(pl, orc, h, build_query, plan_checks, lmask=None, rmask=None, hows=("inner", "left"), ref_keys=None, expect_fused=True):
    """every order x inner / left x fused / no_fusion over one pair of frames; plan_checks(how, order, plan) asserts the route"""
    L, R = _frames(pl, h)
    for how in hows:
        ref = _reference(orc, h, how, lmask, rmask, *(ref_keys or (None, None)))
        for order in _orders_for(how):
            q = build_query(L, R, how, order)
            out = q.collect()
            plan = pl.last_plan()
            assert ("FusedJoinFrame{" in plan) == expect_fused, plan
            if order == "none":
                assert "order=" not in plan, plan
            else:
                assert f"order={order}: " in plan, plan
            plan_checks(how, order, plan)
            _check(out, ref, h, order)
            per_node = q.collect(no_fusion=True)
            plan = pl.last_plan()
            assert "FusedJoinFrame{" not in plan and "Join{" in plan, plan
            assert ("order=" in plan) == (order != "none") and (order == "none" or f"order={order}: " in plan), plan
            _check(per_node, ref, h, order)


def _plain(L, R, how, order):
    return L.lazy().join(R.lazy(), on="k", how=how, maintain_order=order)


def test_direct_address_table_with_ballot_candidates(pl, orc, monkeypatch):
    """dense unique build keys, the larger left side probes: candidates come out of the probe scan's ballots in row order -> left / left_right have nothing to do,
    right / right_left are the stable radix by build row"""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "0")
    h = _sides(np.random.default_rng(1), 400_003, 60_000, _dense)

    def checks(how, order, plan):
        assert "direct-address table" in plan and "build=right" in plan, plan
        if how == "inner":
            assert "direct hits (ballots" in plan, plan
        if order in ("left", "left_right"):
            assert "already ordered" in plan, plan
        if order in ("right", "right_left"):
            assert "radix by build row" in plan, plan
    _run_all(pl, orc, h, _plain, checks)


def test_hash_table_on_sparse_keys(pl, orc, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "0")
    h = _sides(np.random.default_rng(2), 300_017, 50_000, _hashed)

    def checks(how, order, plan):
        assert "hash table cap=" in plan and "unique-keys" in plan and "direct-address" not in plan, plan
        if order in ("left", "left_right"):
            assert "already ordered" in plan, plan
        if order in ("right", "right_left"):
            assert "radix by build row" in plan, plan
    _run_all(pl, orc, h, _plain, checks)


@pytest.mark.parametrize("table", ["hash", "direct"])
def test_partitioned_candidates_are_put_back_in_row_order(pl, orc, monkeypatch, table):
    """PLX_PROBE_PARTITIONED=2: the candidates of an inner join arrive in partition order; an order that can use probe order restores them before the match"""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "2")
    h = _sides(np.random.default_rng(3 + (table == "direct")), (1 << 22) + 999, 300_000, _hashed if table == "hash" else _dense)

    def checks(how, order, plan):
        if how != "inner":
            return
        assert ("partitioned_hash_probe(" if table == "hash" else "partitioned_probe(") in plan, plan
        assert ("candidates back in row order" in plan) == (order in ("left", "left_right", "right_left")), plan
        if order in ("left", "left_right"):
            assert "already ordered" in plan, plan
        if order in ("right", "right_left"):
            assert "radix by build row" in plan, plan
    _run_all(pl, orc, h, _plain, checks)


def test_duplicate_build_keys_chains_and_one_heavy_key(pl, orc, monkeypatch):
    """runs of 1..7 build rows per key are ordered in place; one key with 5 000 build rows crosses the insertion-sort bound and takes the packed radix"""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "0")
    rng = np.random.default_rng(5)
    n_keys = 40_000
    reps = rng.integers(1, 8, n_keys)
    rid = rng.permutation(np.repeat(np.arange(n_keys), reps))
    lid = rng.integers(0, 2 * n_keys, 250_001)

    def sides(heavy):
        r, l = rid.copy(), lid.copy()
        if heavy:
            r = rng.permutation(np.concatenate([r, np.full(5_000, 3 * n_keys)]))
            l[[7, 100_000, 250_000]] = 3 * n_keys
        n_l, n_r = len(l), len(r)
        return dict(lk=_hashed(l), rk=_hashed(r), lv=rng.random(n_l) > 0.03, rv=rng.random(n_r) > 0.02, lx=rng.integers(0, 100, n_l).astype(np.int32), ry=rng.integers(0, 50, n_r).astype(np.int32))

    for heavy in (False, True):
        def checks(how, order, plan):
            assert "multi-value" in plan, plan
            if order == "left":
                assert "already ordered" in plan, plan
            if order == "left_right":
                assert ("a run longer than" in plan and "radix by (probe row, build row)" in plan) if heavy else "ordered in place" in plan, plan
            if order in ("right", "right_left"):
                assert "radix by build row" in plan, plan
        _run_all(pl, orc, sides(heavy), _plain, checks)


def test_left_side_smaller_is_the_build_side(pl, orc, monkeypatch):
    """inner join with the smaller LEFT table: it becomes the build side, so left / left_right are the build-side order (radix) and right / right_left the probe side's;
    duplicate keys on the left: right_left orders chains.  A left join still probes with its left table."""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "0")
    for dup in (False, True):
        h = _sides(np.random.default_rng(6 + dup), 30_000, 200_003, _hashed, left="dup" if dup else "unique")

        def checks(how, order, plan):
            if how == "left":
                assert "build=right" in plan, plan
                return
            assert "build=left" in plan and ("multi-value" in plan) == dup, plan
            if order in ("left", "left_right"):
                assert "radix by build row" in plan, plan
            if order == "right" or (order == "right_left" and not dup):
                assert "already ordered" in plan, plan
            if order == "right_left" and dup:
                assert "ordered in place" in plan, plan
        _run_all(pl, orc, h, _plain, checks)


def test_predicates_on_both_sides(pl, orc, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "0")
    h = _sides(np.random.default_rng(8), 300_000, 80_000, _hashed, dup_right=True)

    def q(L, R, how, order):
        c = pl.col
        return L.lazy().filter(c("x") < 60).join(R.lazy().filter(c("y") != 3), on="k", how=how, maintain_order=order)
    _run_all(pl, orc, h, q, lambda how, order, plan: None, lmask=h["lx"] < 60, rmask=h["ry"] != 3)


def test_null_keys_match_nothing_and_keep_their_place_in_a_left_join(pl, orc, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    rng = np.random.default_rng(9)
    h = _sides(rng, 100_000, 20_000, _dense)
    h["lv"] = rng.random(100_000) > 0.3                    # many null left keys
    L, R = _frames(pl, h)
    out = L.lazy().join(R.lazy(), on="k", how="left", maintain_order="left_right").collect()
    assert "order=left_right" in pl.last_plan()
    g_l, g_r, g_v, _, _ = _got(out)
    null_rows = np.nonzero(~h["lv"])[0]
    assert np.array_equal(np.unique(g_l), np.arange(100_000))          # every left row is there, in place
    assert not g_v[np.isin(g_l, null_rows)].any()                      # and a null key has no right row
    _check(out, _reference(orc, h, "left"), h, "left_right")


def test_multi_column_packed_keys_through_the_per_node_join(pl, orc):
    rng = np.random.default_rng(10)
    n_l, n_r = 200_000, 70_000
    la, lb = rng.integers(0, 300, n_l).astype(np.int64), rng.integers(-20, 20, n_l).astype(np.int32)
    ra, rb = rng.integers(0, 300, n_r).astype(np.int64), rng.integers(-20, 20, n_r).astype(np.int32)
    h = dict(lk=la, rk=ra, lv=None, rv=None, lx=rng.integers(0, 100, n_l).astype(np.int32), ry=rng.integers(0, 50, n_r).astype(np.int32))
    L, R = _frames(pl, h)
    L = pl.DataFrame([L["k"], pl.Series("b", lb), L["lrow"], L["x"]])
    R = pl.DataFrame([R["k"], pl.Series("b", rb), R["rrow"], R["y"]])
    packed = (la * 64 + (lb.astype(np.int64) + 20), ra * 64 + (rb.astype(np.int64) + 20))      # any injective packing gives the oracle the same pairs
    for how in ("inner", "left"):
        ref = _reference(orc, h, how, lk=packed[0], rk=packed[1])
        for order in _orders_for(how):
            out = L.lazy().join(R.lazy(), on=["k", "b"], how=how, maintain_order=order).collect()
            plan = pl.last_plan()
            assert "packed 2 key columns" in plan and "dup-keys" in plan and (order == "none" or f"order={order}: " in plan), plan
            _check(out, ref, h, order)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, (1 << 22) + 77_777])
def test_sizes(pl, orc, monkeypatch, n):
    """wave, tile (4096 keys per workgroup and radix pass) and multi-pass boundaries of the pair list; left side = n rows with duplicate keys on the right"""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "0")
    rng = np.random.default_rng(100 + n % 97)
    n_r = max(n // 3, 1) if n else 0
    h = _sides(rng, n, n_r, _hashed, dup_right=n_r > 4, nulls=n > 0)
    if n == 0:
        h["lv"] = h["rv"] = None
    L, R = _frames(pl, h)
    for how in ("inner", "left"):
        ref = _reference(orc, h, how)
        for order in _orders_for(how):
            q = _plain(L, R, how, order)
            _check(q.collect(), ref, h, order)
            _check(q.collect(no_fusion=True), ref, h, order)


def test_head_over_an_ordered_join_is_the_first_reference_rows(pl, orc, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    h = _sides(np.random.default_rng(11), 50_000, 120_000, _hashed, left="dup")       # build = left: without the option the output is in right order
    L, R = _frames(pl, h)
    lrow, rrow, _ = _reference(orc, h, "inner")
    o = np.lexsort((rrow, lrow))[:10]
    for kw in ({}, {"no_fusion": True}):
        out = L.lazy().join(R.lazy(), on="k", maintain_order="left_right").head(10).collect(**kw)
        assert out.height == 10
        assert out["lrow"].to_numpy().tolist() == lrow[o].tolist() and out["rrow"].to_numpy().tolist() == rrow[o].tolist()


def test_left_join_refuses_the_right_orders_and_names_the_option(pl, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    h = _sides(np.random.default_rng(12), 1000, 500, _dense)
    L, R = _frames(pl, h)
    for order in ("right", "right_left"):
        for kw in ({}, {"no_fusion": True}):
            with pytest.raises(pl.PlxError, match="maintain_order=" + order) as e:
                L.lazy().join(R.lazy(), on="k", how="left", maintain_order=order).collect(**kw)
            assert e.value.code == 3                                       # PLX_ERR_UNSUPPORTED


@pytest.mark.parametrize("how", ["semi", "anti"])
def test_semi_and_anti_joins_are_unchanged_by_any_value(pl, monkeypatch, how):
    h = _sides(np.random.default_rng(13), 200_000, 30_000, _dense, dup_right=True)
    L, R = _frames(pl, h)
    for kw in ({}, {"no_fusion": True}):
        base = L.lazy().join(R.lazy(), on="k", how=how).collect(**kw)
        base_plan = pl.last_plan()
        want = base["lrow"].to_numpy()
        assert np.all(np.diff(want) > 0)                                   # left order already
        for order in ORDERS[1:]:
            out = L.lazy().join(R.lazy(), on="k", how=how, maintain_order=order).collect(**kw)
            assert pl.last_plan() == base_plan
            assert np.array_equal(out["lrow"].to_numpy(), want) and np.array_equal(out["x"].to_numpy(), base["x"].to_numpy())


def test_group_by_maintain_order_over_an_ordered_join_sees_left_order(pl, orc, monkeypatch):
    """a join feeding group_by(maintain_order=True): the groups appear in the order of their first LEFT row when the join keeps left order (build = left here)"""
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    h = _sides(np.random.default_rng(14), 20_000, 90_000, _hashed, nulls=False)
    L, R = _frames(pl, h)
    out = L.lazy().join(R.lazy(), on="k", maintain_order="left").group_by("x", maintain_order=True).agg(pl.len().alias("n")).collect(no_fusion=True)
    lrow, rrow, _ = _reference(orc, h, "inner")
    x_in_left_order = h["lx"][np.sort(lrow)]
    _, first = np.unique(x_in_left_order, return_index=True)
    assert out["x"].to_numpy().tolist() == x_in_left_order[np.sort(first)].tolist()
