"""The benchmark queries of BASELINE.json / SURVEY.md section 8(d) and Appendix A, written
in the mirror API.  Shared by bench.py, the parity tests and tools/gen_fused_shapes.py."""
from __future__ import annotations

import datetime as dt

from . import expr as E

Q1_CUTOFF = dt.datetime(1998, 9, 2)
Q3_DATE = dt.datetime(1995, 3, 15)


def cfg1(lf, k=2 ** 30):
    """filter(a > k).select(a.sum())  -- BASELINE config 1"""
    return lf.filter(E.col("a") > k).select(E.col("a").sum())


def cfg2(lf, k=2 ** 30):
    """filter(a > k).select((x*(1-y)).sum(), x.mean(), a.sum())  -- BASELINE config 2"""
    return lf.filter(E.col("a") > k).select((E.col("x") * (1 - E.col("y"))).sum().alias("xy"), E.col("x").mean().alias("x_mean"),
                                            E.col("a").sum().alias("a_sum"))


def cfg3(lf):
    """group_by(key).agg(v.sum(), v.count())  -- BASELINE config 3"""
    return lf.group_by("key").agg(E.col("v").sum().alias("v_sum"), E.col("v").count().alias("v_count"))


def cfg3w(lf):
    """group_by(k1, k2).agg(v.sum(), v.count())  -- config 3 on a two-column (wide) key: the reference row-encodes it (hash_keys.rs:334 RowEncodedKeys)"""
    return lf.group_by("k1", "k2").agg(E.col("v").sum().alias("v_sum"), E.col("v").count().alias("v_count"))


def cfg5(lf):
    """group_by(k).agg(v.sum(), v.mean()) on dictionary-encoded string keys -- BASELINE config 5"""
    return lf.group_by("k").agg(E.col("v").sum().alias("v_sum"), E.col("v").mean().alias("v_mean"))


def h2o_sd(lf):
    """group_by(id4, id5).agg(v3.std(), v3.mean()) -- the H2O group-by benchmark's `sd(v3) by id4, id5` (beside the mean: both share the count cell)"""
    return lf.group_by("id4", "id5").agg(E.col("v3").std().alias("v3_sd"), E.col("v3").mean().alias("v3_mean"))


def h2o_median_sd(lf):
    """group_by(id4, id5).agg(v3.median(), v3.std()) -- the H2O group-by benchmark's `median(v3), sd(v3) by id4, id5` as it is asked: the std runs through the fused
    scan's cells, the median over sorted segments"""
    return lf.group_by("id4", "id5").agg(E.col("v3").median().alias("v3_median"), E.col("v3").std().alias("v3_sd"))


def lineitem_distinct(lineitem):
    """group_by(l_returnflag, l_linestatus).agg(l_quantity.n_unique(), l_shipdate.n_unique(), len) -- the shape of TPC-H Q16's `count(distinct ps_suppkey)` over the
    columns the lineitem generator has: distinct quantities and ship dates per flag and status.  The count of rows runs through the fused scan's cells, each distinct
    count over the sorted segments of its source"""
    return lineitem.group_by("l_returnflag", "l_linestatus").agg(E.col("l_quantity").n_unique().alias("n_quantities"), E.col("l_shipdate").n_unique().alias("n_shipdates"),
                                                                  E.len().alias("count_order"))


def share_of_flag_total(lineitem):
    """with_columns((l_extendedprice / l_extendedprice.sum().over(l_returnflag, l_linestatus)).alias("share")).filter(l_quantity > l_quantity.median().over(l_returnflag))
    -- every line's share of the revenue of its (flag, status), kept where its quantity lies above the median quantity of its flag.  Two window expressions: each runs
    one group-by over its keys and goes back to the rows through one row -> group map and one broadcast; height and row order stay the frame's until the filter"""
    c = E.col
    return (lineitem.with_columns((c("l_extendedprice") / c("l_extendedprice").sum().over("l_returnflag", "l_linestatus")).alias("share"))
            .filter(c("l_quantity") > c("l_quantity").median().over("l_returnflag")))


def running_revenue_by_flag(lineitem):
    """with_columns((l_extendedprice * (1 - l_discount)).cum_sum().over(l_returnflag, l_linestatus).alias("running_revenue")) -- every line's revenue added to the
    revenue of the lines of its (flag, status) before it, in the frame's row order.  One stable sort of the rows by the two keys, one head mask and one segmented scan
    in three launches; height and row order stay the frame's"""
    c = E.col
    return lineitem.with_columns((c("l_extendedprice") * (1.0 - c("l_discount"))).cum_sum().over("l_returnflag", "l_linestatus").alias("running_revenue"))


def top3_price_per_flag(lineitem):
    """filter(l_extendedprice.rank("ordinal", descending=True).over(l_returnflag, l_linestatus) <= 3) -- the three most expensive lines of every (flag, status), in
    the frame's row order; ordinal ranks break ties by row order, so exactly three rows of every partition stay.  One sort by (flag, status, price descending) and one
    O(1)-per-row rank kernel"""
    c = E.col
    return lineitem.filter(c("l_extendedprice").rank("ordinal", descending=True).over("l_returnflag", "l_linestatus") <= 3)


def moving_average_revenue_by_flag(lineitem):
    """with_columns((l_extendedprice * (1 - l_discount)).rolling_mean(7, min_samples=1).over(l_returnflag).alias("revenue_ma7")) -- the mean revenue of every line
    and the up to six lines of its flag before it, in the frame's row order.  The stable sort and head mask of the cumulative functions, then one tile-halo launch:
    two segmented scans in registers and one combine per row, never a difference of prefixes"""
    c = E.col
    return lineitem.with_columns((c("l_extendedprice") * (1.0 - c("l_discount"))).rolling_mean(7, min_samples=1).over("l_returnflag").alias("revenue_ma7"))


def quantity_change_by_flag(lineitem):
    """with_columns(l_quantity.diff().over(l_returnflag).alias("quantity_change"), l_quantity.shift(1).over(l_returnflag).alias("previous_quantity")) -- every
    line's quantity against the line of its flag before it (null on the first line of a flag).  Both share one sorted order; one launch each"""
    c = E.col
    return lineitem.with_columns(c("l_quantity").diff().over("l_returnflag").alias("quantity_change"), c("l_quantity").shift(1).over("l_returnflag").alias("previous_quantity"))


def q1(lineitem, cutoff=Q1_CUTOFF):
    """TPC-H Q1; the final sort by (flag, status) happens on the host."""
    c = E.col
    disc_price = c("l_extendedprice") * (1 - c("l_discount"))
    return (lineitem.filter(c("l_shipdate") <= cutoff)
            .group_by("l_returnflag", "l_linestatus")
            .agg(c("l_quantity").sum().alias("sum_qty"),
                 c("l_extendedprice").sum().alias("sum_base_price"),
                 disc_price.sum().alias("sum_disc_price"),
                 (disc_price * (1 + c("l_tax"))).sum().alias("sum_charge"),
                 c("l_quantity").mean().alias("avg_qty"),
                 c("l_extendedprice").mean().alias("avg_price"),
                 c("l_discount").mean().alias("avg_disc"),
                 E.len().alias("count_order")))


def q6(lineitem, year: int = 1994, discount: float = 0.06, quantity: int = 24):
    """TPC-H Q6 (forecasting revenue change): one filter + one sum, the shape of BASELINE config 2 on lineitem's columns --
    sum(l_extendedprice * l_discount) over shipdate in [year, year + 1), discount within +-0.01, quantity below the bound."""
    c = E.col
    lo, hi = dt.datetime(year, 1, 1), dt.datetime(year + 1, 1, 1)
    return (lineitem.filter(c("l_shipdate").is_between(lo, hi, closed="left") & c("l_discount").is_between(round(discount - 0.01, 2), round(discount + 0.01, 2))
                            & (c("l_quantity") < quantity))
            .select((c("l_extendedprice") * c("l_discount")).sum().alias("revenue")))


def q6_year(lineitem, year: int = 1994, discount: float = 0.06, quantity: int = 24):
    """TPC-H Q6 with the year as the query states it: l_shipdate.dt.year() == year instead of q6's two date literals.  The year is computed inside the scan."""
    c = E.col
    return (lineitem.filter((c("l_shipdate").dt.year() == year) & c("l_discount").is_between(round(discount - 0.01, 2), round(discount + 0.01, 2))
                            & (c("l_quantity") < quantity))
            .select((c("l_extendedprice") * c("l_discount")).sum().alias("revenue")))


def revenue_by_ship_month(lineitem, cutoff=Q1_CUTOFF):
    """Revenue per calendar month: lineitem[l_shipdate <= cutoff] grouped by (year, month) of l_shipdate -- the grouping of TPC-H Q7 / Q8 / Q9 (extract(year from ...))
    and of every "per month" report.  Both keys are computed inside the scan; their ranges are known without a pass over the data (month) or from the column's own
    range (year), so the pair packs into a few bits and takes the dense table routes."""
    c = E.col
    return (lineitem.filter(c("l_shipdate") <= cutoff)
            .group_by(c("l_shipdate").dt.year().alias("year"), c("l_shipdate").dt.month().alias("month"))
            .agg((c("l_extendedprice") * (1 - c("l_discount"))).sum().alias("revenue"), E.len().alias("n")))


def q3(lineitem, orders, date=Q3_DATE, seg_mod=5):
    """TPC-H Q3 restated on the two big tables (SURVEY.md 8(d) cfg 4): the customer
    market-segment filter is approximated by o_custkey % seg_mod == 0."""
    c = E.col
    o = orders.filter((c("o_orderdate") < date) & ((c("o_custkey") % seg_mod) == 0))
    li = lineitem.filter(c("l_shipdate") > date)
    return (li.join(o, left_on="l_orderkey", right_on="o_orderkey")
            .group_by("l_orderkey", "o_orderdate", "o_shippriority")
            .agg((c("l_extendedprice") * (1 - c("l_discount"))).sum().alias("revenue")))


def q3_join_frame(lineitem, orders, date=Q3_DATE, seg_mod=5):
    """Q3's two filtered tables joined into a FRAME (no group-by above the join): the materialising hash join, five output columns."""
    c = E.col
    o = orders.filter((c("o_orderdate") < date) & ((c("o_custkey") % seg_mod) == 0))
    li = lineitem.filter(c("l_shipdate") > date)
    return li.join(o, left_on="l_orderkey", right_on="o_orderkey").select("l_orderkey", "o_orderdate", "o_shippriority", "l_extendedprice", "l_discount")


def q3_semi_frame(lineitem, orders, date=Q3_DATE, seg_mod=5):
    """The lineitem rows of Q3's join as a SEMI join: lineitem[l_shipdate > date] whose order is among orders[o_orderdate < date, o_custkey % seg_mod == 0] --
    left columns only, left order (single_keys_semi_anti.rs)."""
    c = E.col
    o = orders.filter((c("o_orderdate") < date) & ((c("o_custkey") % seg_mod) == 0))
    li = lineitem.filter(c("l_shipdate") > date)
    return li.join(o, left_on="l_orderkey", right_on="o_orderkey", how="semi")


def q3_partsupp(lineitem, partsupp, date=Q3_DATE, group=5):
    """A join whose BUILD side repeats its keys: lineitem[l_shipdate > date] JOIN partsupp[ps_group == group] ON partkey (dbgen's partsupp holds four rows per part;
    the shape of TPC-H Q9 / Q20's partsupp joins), grouped by (l_partkey, ps_suppkey) -- a group is a build row, every lineitem row of a part contributes to each of the
    part's suppliers.  ps_group is a property of the part (the same for all of its rows): the predicate keeps parts with ALL their partsupp rows."""
    c = E.col
    ps = partsupp.filter(c("ps_group") == group)
    li = lineitem.filter(c("l_shipdate") > date)
    return (li.join(ps, left_on="l_partkey", right_on="ps_partkey")
            .group_by("l_partkey", "ps_suppkey")
            .agg((c("l_extendedprice") * (1 - c("l_discount"))).sum().alias("revenue"), E.len().alias("n")))


def q3_full(customer, orders, lineitem, date=Q3_DATE, segment="BUILDING"):
    """TPC-H Q3 with all three tables, in the form the optimizer hands the physical planner (single-table
    predicates pushed below the joins): customer[c_mktsegment == segment] JOIN orders[o_orderdate < date] ON custkey, then
    JOIN lineitem[l_shipdate > date] ON orderkey, grouped by (o_orderkey, o_orderdate, o_shippriority)."""
    c = E.col
    cust = customer.filter(c("c_mktsegment") == segment)
    o = cust.join(orders.filter(c("o_orderdate") < date), left_on="c_custkey", right_on="o_custkey")
    j = o.join(lineitem.filter(c("l_shipdate") > date), left_on="o_orderkey", right_on="l_orderkey")
    return (j.group_by("o_orderkey", "o_orderdate", "o_shippriority")
            .agg((c("l_extendedprice") * (1 - c("l_discount"))).sum().alias("revenue")))


def q3_full_top10(customer, orders, lineitem, date=Q3_DATE, segment="BUILDING"):
    """... ORDER BY revenue DESC, o_orderdate LIMIT 10"""
    return q3_full(customer, orders, lineitem, date, segment).sort("revenue", "o_orderdate", descending=[True, False]).head(10)


def q1_sorted(lineitem, cutoff=Q1_CUTOFF):
    """TPC-H Q1 including its ORDER BY l_returnflag, l_linestatus (device radix sort of the <= 6 result rows)."""
    return q1(lineitem, cutoff).sort("l_returnflag", "l_linestatus")


def q3_top10(lineitem, orders, date=Q3_DATE, seg_mod=5):
    """TPC-H Q3 including its ORDER BY revenue DESC, o_orderdate LIMIT 10: the Slice directly above the Sort becomes a
    radix select over the ~1e6 groups."""
    return q3(lineitem, orders, date, seg_mod).sort("revenue", "o_orderdate", descending=[True, False]).head(10)


def q12(lineitem, orders, modes=(3, 5), high=(0, 1)):
    """TPC-H Q12's shape over caller-supplied frames: lineitem[l_shipmode in modes] JOIN orders ON orderkey, grouped by ship mode, with the two conditional counts
    sum(case when o_orderpriority in high then 1 else 0 end) and its complement.  Ship modes and priorities are whatever the frames hold: integer codes, or
    strings against dictionary-encoded columns."""
    c = E.col
    is_high = c("o_orderpriority").is_in(high)
    j = lineitem.filter(c("l_shipmode").is_in(modes)).join(orders, left_on="l_orderkey", right_on="o_orderkey")
    return j.group_by("l_shipmode").agg(E.when(is_high).then(1).otherwise(0).sum().alias("high_line_count"),
                                        E.when(~is_high).then(1).otherwise(0).sum().alias("low_line_count"))


def q14_sums(lineitem, part, promo_below=25):
    """The two sums of TPC-H Q14 over caller-supplied frames: lineitem JOIN part ON partkey, then sum(case when promo then revenue else 0 end) and sum(revenue) with
    promo = p_type < promo_below (dbgen's PROMO% types as a code range).  The final ratio is arithmetic over aggregates, left to the caller."""
    c = E.col
    rev = c("l_extendedprice") * (1 - c("l_discount"))
    j = lineitem.join(part, left_on="l_partkey", right_on="p_partkey")
    return j.select(E.when(c("p_type") < promo_below).then(rev).otherwise(0.0).sum().alias("promo_revenue"), rev.sum().alias("revenue"))


def q14_promo(lineitem, part, prefix="PROMO"):
    """TPC-H Q14's two sums with the predicate as the query states it: p_type LIKE 'PROMO%' is str.starts_with on the dictionary-encoded p_type column -- decided once
    per distinct type, looked up per row -- instead of q14_sums' code range, which only holds for a generator that hands the codes out in that order."""
    c = E.col
    rev = c("l_extendedprice") * (1 - c("l_discount"))
    j = lineitem.join(part, left_on="l_partkey", right_on="p_partkey")
    return j.select(E.when(c("p_type").str.starts_with(prefix)).then(rev).otherwise(0.0).sum().alias("promo_revenue"), rev.sum().alias("revenue"))


def quote_before_trade(trades, quotes, tolerance=None):
    """Every trade with the last quote of its symbol at or before it, at most `tolerance` (default one second) old, then per symbol how many trades found a quote
    and what they paid over it: join_asof(by="sym", on="ts", tolerance=...) -> group_by("sym").  trades / quotes: sym, ts (Datetime), price; neither side needs to
    be sorted."""
    c = E.col
    tol = dt.timedelta(seconds=1) if tolerance is None else tolerance
    j = trades.join_asof(quotes, by="sym", on="ts", tolerance=tol)
    return j.group_by("sym").agg(E.len().alias("trades"), c("price_right").count().alias("quoted"), (c("price") - c("price_right")).mean().alias("mean_over_quote"),
                                 c("price_right").max().alias("max_quote"))
