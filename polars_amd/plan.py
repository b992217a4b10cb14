"""Logical plan of the mirror API and its lowering to the IR / AExpr arenas that cross
the C ABI (plx_ir / plx_aexpr).

In the reference this work is done by polars-plan: DSL -> IR conversion and the
optimizer's type-coercion pass, which inserts ``AExpr::Cast`` so that every
``BinaryExpr`` reaches the physical planner with same-typed operands
(crates/polars-plan/src/plans/conversion/type_coercion/binary.rs:172-...).  polars-plan
is out of scope (kept as the API surface), so this module restates the small part the
hot path needs; the GPU engine itself only ever sees coerced arenas.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

from . import _ffi as F
from . import datatypes as T
from .expr import CUM_NAMES, ROLLING_NAMES, STR_MATCH_NAMES, Expr, dt_part_dtype, dt_unit, literal_physical, str_match_host, str_pattern_bytes

Schema = Dict[str, T.DataType]


# ---- logical plan nodes ------------------------------------------------------------------
class Node:
    def __init__(self, kind: str, **kw):
        self.kind = kind
        self.__dict__.update(kw)


# JoinArgs.maintain_order -> plx_join_order (include/polars_amd.h)
JOIN_ORDERS = {"none": F.JOIN_ORDER_NONE, "left": F.JOIN_ORDER_LEFT, "right": F.JOIN_ORDER_RIGHT, "left_right": F.JOIN_ORDER_LEFT_RIGHT, "right_left": F.JOIN_ORDER_RIGHT_LEFT}


# join kinds -> plx_join_how; JoinArgs.coalesce (None: the kind's default, True, False) -> plx_ir.coalesce
JOIN_HOWS = {"inner": F.JOIN_INNER, "left": F.JOIN_LEFT, "semi": F.JOIN_SEMI, "anti": F.JOIN_ANTI, "full": F.JOIN_FULL, "right": F.JOIN_RIGHT}
JOIN_COALESCE = {None: F.JOIN_COALESCE_DEFAULT, True: F.JOIN_COALESCE, False: F.JOIN_KEEP_BOTH}


def join_schema(how: str, coalesce, left_on, right_on, ls: Schema, rs: Schema, suffix: str) -> Schema:
    """Output columns of a join (plx_ir.coalesce in include/polars_amd.h): left columns, then right columns, the suffix on a right name that clashes.  A key pair of two
    plain columns coalesces unless told otherwise (a full join: only when told to): inner / left / full drop the right key, a right join drops the left key.
    On right and full joins a pair whose dtypes differ does not coalesce: lowering casts such keys to their supertype, and the engine merges plain columns only
    (schemas that carry dtypes, i.e. lowering and collect_schema; inner / left joins keep the rule they had)."""
    if how in ("semi", "anti"):            # left columns only (single_keys_semi_anti.rs)
        return dict(ls)
    merge = (how != "full") if coalesce is None else bool(coalesce)
    def cast_apart(a, b):
        adt, bdt = ls.get(a.name), rs.get(b.name)
        return how in ("right", "full") and adt is not None and bdt is not None and adt.physical != bdt.physical
    plain = [(a.name, b.name) for a, b in zip(left_on, right_on) if a.kind == "col" and b.kind == "col" and not cast_apart(a, b)] if merge else []
    drop_left = {a for a, _ in plain} if how == "right" else set()
    drop_right = {b for _, b in plain} if how != "right" else set()
    out = {name: dt for name, dt in ls.items() if name not in drop_left}
    for name, dt in rs.items():
        if name in drop_right:
            continue
        out[name + suffix if name in out else name] = dt
    return out


def _is_temporal(dt) -> bool:
    return dt == T.Date or isinstance(dt, T.DatetimeType)


def asof_tolerance_literal(tolerance: Any, on_dt: T.DataType) -> Tuple[Any, T.DataType]:
    """The tolerance of a join_asof as the literal of its PLX_IR_JOIN_ASOF node: (value, literal dtype) in the `on` dtype's family.  Integer and temporal `on`: an
    int in the column's own unit (Int64, UInt64 for an unsigned `on`); Date / Datetime also take a datetime.timedelta, converted exactly (one that is no whole number
    of the unit is refused); float `on`: a float (Float64).  Negative, NaN and duration strings ("2h") are ValueErrors naming the value."""
    import datetime as _dt
    import math
    import numbers
    if isinstance(tolerance, str):
        raise ValueError(f"join_asof: tolerance={tolerance!r}: duration strings are not on this path; give an int in the column's own unit, a datetime.timedelta (Date / Datetime) or a float")
    if isinstance(tolerance, bool) or not isinstance(tolerance, (numbers.Real, _dt.timedelta)):
        raise ValueError(f"join_asof: tolerance={tolerance!r} is neither a number nor a datetime.timedelta")
    if isinstance(tolerance, _dt.timedelta):
        if not _is_temporal(on_dt):
            raise ValueError(f"join_asof: tolerance={tolerance!r}: a timedelta needs a Date or Datetime `on`, this one is {on_dt}")
        us = (tolerance.days * 86_400 + tolerance.seconds) * 1_000_000 + tolerance.microseconds
        if us < 0:
            raise ValueError(f"join_asof: tolerance={tolerance!r} is negative")
        num, den = (us, 86_400_000_000) if on_dt == T.Date else (us * on_dt.ticks_per_second(), 1_000_000)
        if num % den:
            raise ValueError(f"join_asof: tolerance={tolerance!r} is no whole number of the unit of `on` ({'days' if on_dt == T.Date else on_dt.time_unit})")
        return num // den, T.Int64
    if on_dt.is_float():
        f = float(tolerance)
        if math.isnan(f) or f < 0:
            raise ValueError(f"join_asof: tolerance={tolerance!r} must be a number >= 0")
        return f, T.Float64
    if not isinstance(tolerance, numbers.Integral):
        if isinstance(tolerance, float) and (math.isnan(tolerance) or tolerance < 0):
            raise ValueError(f"join_asof: tolerance={tolerance!r} must be a number >= 0")
        raise ValueError(f"join_asof: tolerance={tolerance!r}: `on` is {on_dt}, so the tolerance is an int in the column's own unit" + (" or a datetime.timedelta" if _is_temporal(on_dt) else ""))
    v = int(tolerance)
    if v < 0:
        raise ValueError(f"join_asof: tolerance={tolerance!r} is negative")
    lit_dt = T.UInt64 if on_dt.name.startswith("UInt") else T.Int64
    if v > (2 ** 64 - 1 if lit_dt == T.UInt64 else 2 ** 63 - 1):
        raise ValueError(f"join_asof: tolerance={tolerance!r} does not fit the {lit_dt} literal of the plan node")
    return v, lit_dt


def describe_asof_joins(node: Node) -> List[str]:
    """One line per join_asof under `node` (LazyFrame.explain): the JoinAsof node as it is lowered."""
    out: List[str] = []
    for attr in ("input", "left", "right"):
        child = getattr(node, attr, None)
        if isinstance(child, Node):
            out += describe_asof_joins(child)
    if node.kind == "join_asof":
        by = ", ".join(f"{a!r} = {b!r}" for a, b in zip(node.left_on[:-1], node.right_on[:-1]))
        out.append(f"JoinAsof[strategy={node.strategy}{' strict' if node.strict else ''}, by=[{by}], on={node.left_on[-1]!r} / {node.right_on[-1]!r}, "
                   f"tolerance={node.tolerance!r}, order=left rows]")
    return out


def describe_distincts(node: Node) -> List[str]:
    """One line per unique() under `node` (LazyFrame.explain): the Distinct node as it is lowered."""
    out: List[str] = []
    for attr in ("input", "left", "right"):
        child = getattr(node, attr, None)
        if isinstance(child, Node):
            out += describe_distincts(child)
    if node.kind == "unique":
        subset = "all columns" if node.subset is None else "[" + ", ".join(node.subset) + "]"
        keep = "first (asked: any)" if node.keep == "any" else node.keep
        out.append(f"Distinct[subset={subset}, keep={keep}, order=rows]")
    return out


def describe_windows(node: Node) -> List[str]:
    """One line per window expression under `node` (LazyFrame.explain): the function and its keys as written.  The route each one took is in the physical plan
    of the last collect (`Window{... route=window[direct range=R] | window[sorted rows: ...]}`)."""
    out: List[str] = []
    for attr in ("input", "left", "right"):
        child = getattr(node, attr, None)
        if isinstance(child, Node):
            out += describe_windows(child)

    def walk(e):
        if e is None:
            return
        f = e.lhs if e.kind == "window" else None
        while f is not None and f.kind == "alias":
            f = f.lhs
        if e.kind == "window" and f.kind not in ROW_FUNCTION_KINDS:      # (a cumulative / ranking / shift / rolling function under .over has its own line: describe_cumulatives)
            out.append(f"Window[{e.lhs!r} over [{', '.join(repr(k) for k in e.value)}], mapping=group_to_rows] in {node.kind}")
        for c in e.children():
            walk(c)
    for e in list(getattr(node, "exprs", None) or []) + [getattr(node, "predicate", None)]:
        walk(e)
    return out


ROW_FUNCTION_KINDS = ("cum", "rank", "shift", "rolling")      # one value per row from the rows around it: cum_*, rank, shift / diff, rolling_*
_ROW_FUNCTION_TITLES = {"cum": "Cumulative", "rank": "Rank", "shift": "Shift", "rolling": "Rolling"}


def describe_cumulatives(node: Node) -> List[str]:
    """One line per cumulative / ranking / shift / diff / rolling expression under `node` (LazyFrame.explain): the function as written and its partition.  The route
    each one took is in the physical plan of the last collect (`Cumulative{... route=cumulative[whole column] | cumulative[sorted rows: ...]}`, `Rank{...
    route=rank[sorted segments: ...]}`, `Shift{... route=shift[whole column] | shift[sorted rows: ...]}`, `Rolling{... route=rolling[tile halo: ...] | rolling[two
    scans: ...]}`)."""
    out: List[str] = []
    for attr in ("input", "left", "right"):
        child = getattr(node, attr, None)
        if isinstance(child, Node):
            out += describe_cumulatives(child)

    def walk(e, keys):
        if e is None:
            return
        if e.kind in ROW_FUNCTION_KINDS:
            over = "the whole column" if keys is None else "[" + ", ".join(repr(k) for k in keys) + "]"
            out.append(f"{_ROW_FUNCTION_TITLES[e.kind]}[{e!r} over {over}] in {node.kind}")
        if e.kind == "window":
            f = e.lhs
            while f is not None and f.kind == "alias":
                f = f.lhs
            if f is not None and f.kind in ROW_FUNCTION_KINDS:
                walk(f, e.value)
                return
        for c in e.children():
            walk(c, None)
    for e in list(getattr(node, "exprs", None) or []) + [getattr(node, "predicate", None)]:
        walk(e, None)
    return out


def has_row_function(e: Optional[Expr]) -> bool:
    """a cumulative, ranking, shift / diff or rolling expression anywhere in `e`: like a window, it reads every row of its input"""
    return e is not None and (e.kind in ROW_FUNCTION_KINDS or any(has_row_function(c) for c in e.children()))


def row_function_name(e: Expr) -> str:
    if e.kind == "cum":
        return CUM_NAMES[e.op]
    if e.kind == "shift":
        return "diff" if e.op == F.SHIFT_DIFF else "shift"
    return ROLLING_NAMES[e.op] if e.kind == "rolling" else "rank"


def shift_result_dtype(op: int, dt) -> T.DataType:
    """shift keeps the dtype, whatever it is; diff widens unsigned operands (UInt8 -> Int16, UInt16 -> Int32, UInt32 / UInt64 -> Int64) and takes integers and floats
    only: there is no Duration dtype here for a temporal difference, and Boolean / Categorical have none."""
    if op == F.SHIFT_SHIFT:
        if not isinstance(dt, T.DataType):
            raise TypeError(f"shift() needs a column expression, got {dt}")
        return dt
    if not isinstance(dt, T.DataType) or not dt.is_numeric():
        raise TypeError(f"diff() needs an integer or float expression, got {dt}" + (" (a temporal difference would be a Duration, which is not built)" if dt in (T.Date, T.Datetime) else ""))
    return {T.UInt8: T.Int16, T.UInt16: T.Int32, T.UInt32: T.Int64, T.UInt64: T.Int64}.get(dt, dt)


def rolling_result_dtype(op: int, dt) -> T.DataType:
    """rolling_sum follows cum_sum, rolling_mean is Float64 (Float32 stays), rolling_min / rolling_max keep the dtype and are the only ones to take Date / Datetime;
    Categorical operands are refused everywhere (codes are not lexical order, and sum nothing)."""
    name = ROLLING_NAMES[op]
    temporal_ok = op in (F.ROLLING_MIN, F.ROLLING_MAX)
    if not isinstance(dt, T.DataType) or isinstance(dt, T.Categorical) or not (dt.is_numeric() or dt == T.Boolean or (temporal_ok and dt in (T.Date, T.Datetime))):
        raise TypeError(f"{name}() needs an integer, float or Boolean expression{' (or a Date / Datetime one)' if temporal_ok else ''}, got {dt}")
    if op == F.ROLLING_SUM:
        return sum_dtype(dt)
    if op == F.ROLLING_MEAN:
        return T.Float32 if dt == T.Float32 else T.Float64
    return dt


def shift_fill_literal(fill: Any, dt: T.DataType):
    """The physical value of shift's fill_value for a column of dtype `dt`; TypeError naming fill_value when the dtype cannot hold it exactly."""
    import datetime as _dt

    import numpy as np

    def bad(why: str = ""):
        return TypeError(f"shift(fill_value={fill!r}): a {dt} column cannot hold this fill_value exactly{why}")
    if isinstance(fill, np.generic):
        fill = fill.item()
    if isinstance(dt, T.Categorical):
        cats = list(dt.categories)
        if not isinstance(fill, str) or fill not in cats:
            raise bad(" (a Categorical column takes a string of its dictionary)")
        return cats.index(fill)
    if dt == T.Boolean:
        if not isinstance(fill, bool):
            raise bad()
        return fill
    if isinstance(fill, bool):
        raise bad()
    if dt == T.Date:
        if isinstance(fill, _dt.date) and not isinstance(fill, _dt.datetime):
            fill = literal_physical(fill)[0]
        if not isinstance(fill, int) or not -(2 ** 31) <= fill < 2 ** 31:
            raise bad()
        return fill
    if dt == T.Datetime:
        if isinstance(fill, _dt.datetime):
            us = literal_physical(fill)[0]
            per = dt.ticks_per_second()
            if (us * per) % 1_000_000:
                raise bad()
            fill = us * per // 1_000_000
        if not isinstance(fill, int) or not -(2 ** 63) <= fill < 2 ** 63:
            raise bad()
        return fill
    if dt.is_integer():
        if isinstance(fill, float) and fill.is_integer():
            fill = int(fill)
        ii = np.iinfo(dt.np_dtype)
        if not isinstance(fill, int) or not ii.min <= fill <= ii.max:
            raise bad()
        return fill
    if dt.is_float():
        if not isinstance(fill, (int, float)):
            raise bad()
        f = float(fill)
        if isinstance(fill, int) and int(f) != fill:
            raise bad()
        if dt == T.Float32 and f == f and float(np.float32(f)) != f:
            raise bad()
        return f
    raise bad()


def cum_result_dtype(op: int, dt) -> T.DataType:
    """Logical result dtype of a cumulative function over a `dt` operand; TypeError for an operand it does not take.  cum_sum follows the sum aggregate and takes no
    temporal or Categorical operand; cum_min / cum_max keep the dtype (Date / Datetime included) and take no Categorical (codes are not lexical order); cum_count
    takes anything."""
    name = CUM_NAMES[op]
    if op == F.CUM_COUNT:
        return T.UInt32
    if not isinstance(dt, T.DataType) or isinstance(dt, T.Categorical):
        raise TypeError(f"{name}() needs an integer, float or Boolean expression{' (or a Date / Datetime one)' if op != F.CUM_SUM else ''}, got {dt}")
    if op == F.CUM_SUM:
        if not (dt.is_numeric() or dt == T.Boolean):        # Date / Datetime
            raise TypeError(f"cum_sum() needs an integer, float or Boolean expression, got {dt}")
        return sum_dtype(dt)
    return dt


def rank_result_dtype(method: str, dt) -> T.DataType:
    """Float64 for "average", UInt32 for the other methods; TypeError for a Categorical operand (codes are not lexical order)."""
    if not isinstance(dt, T.DataType) or isinstance(dt, T.Categorical):
        raise TypeError(f"rank() needs an integer, float, Boolean, Date or Datetime expression, got {dt}")
    return T.Float64 if method == "average" else T.UInt32


def describe_join_orders(node: Node) -> List[str]:
    """One line per join under `node` that was asked to keep a row order (LazyFrame.explain)."""
    out: List[str] = []
    for attr in ("input", "left", "right"):
        child = getattr(node, attr, None)
        if isinstance(child, Node):
            out += describe_join_orders(child)
    if node.kind == "join" and getattr(node, "maintain_order", "none") != "none":
        out.append(f"Join[how={node.how}, maintain_order={node.maintain_order}]")
    return out


def sum_dtype(dt: T.DataType) -> T.DataType:
    # sum_output_dtype, crates/polars-core/src/chunked_array/ops/aggregate/mod.rs:55-64
    if dt == T.Boolean:
        return T.UInt32
    if dt in (T.Int8, T.Int16, T.UInt8, T.UInt16):
        return T.Int64
    return dt


class Lowering:
    """Builds the arenas. ``aexprs`` / ``irs`` are lists of plain dicts; ``to_c`` marshals
    them into the plx_aexpr / plx_ir structs of include/polars_amd.h."""

    def __init__(self):
        self.aexprs: List[dict] = []
        self.irs: List[dict] = []
        self.luts: List[Any] = []        # lookup bitmaps of the AE_BITMAP_LOOKUP nodes, in order of appearance: host bool arrays (None for one decided on the device)
        self.lut_columns: List[Any] = [] # ... and their Boolean columns (Series; placeholders without a device), kept alive with the arenas
        self._lut_memo: Dict[Any, Any] = {}   # (dictionary, kind, pattern) -> its column: the same predicate twice (pred and ~pred of a conditional pair) is one bitmap
        self.notes: List[str] = []       # what lowering itself decided, for pl.last_plan(): "str.starts_with('PROMO') over 150 categories [device]"

    # -- expressions ---------------------------------------------------------------------
    def _push(self, **kw) -> int:
        node = dict(kind=0, op=0, lhs=-1, rhs=-1, dtype=0, is_null=0, lit=None, name=None, cond=-1, lut=None)
        node.update(kw)
        self.aexprs.append(node)
        return len(self.aexprs) - 1

    def _cast(self, idx: int, frm, to: T.DataType) -> int:
        if frm == to or (isinstance(frm, T.DataType) and frm.physical == to.physical and frm.name == to.name):
            return idx
        return self._push(kind=F.AE_CAST, lhs=idx, dtype=to.physical)

    def _lit_node(self, value, dt: T.DataType) -> int:
        return self._push(kind=F.AE_LITERAL, dtype=dt.physical, lit=value, is_null=0)

    def _materialise_dyn(self, pending, target: Optional[T.DataType]) -> Tuple[int, T.DataType]:
        """A python int / float literal takes the dtype of what it meets."""
        value, tag = pending
        if tag == "dyn_int":
            if target is not None and target.is_integer():
                info_ok = True
                try:
                    import numpy as np
                    ii = np.iinfo(target.np_dtype)
                    info_ok = ii.min <= value <= ii.max
                except Exception:
                    info_ok = False
                if info_ok:
                    return self._lit_node(int(value), target), target
                raise OverflowError(f"literal {value} does not fit {target}")
            if target is not None and target.is_float():
                return self._lit_node(float(value), target), target
            if target is not None and target in (T.Date, T.Datetime):
                return self._lit_node(int(value), target), target
            dt = T.Int32 if -(2 ** 31) <= value < 2 ** 31 else T.Int64
            return self._lit_node(int(value), dt), dt
        # dyn_float
        if target is not None and target == T.Float32:
            return self._lit_node(float(value), T.Float32), T.Float32
        return self._lit_node(float(value), T.Float64), T.Float64

    def lower_expr(self, e: Expr, schema: Schema, want: Optional[T.DataType] = None):
        """Returns (arena index, logical dtype). Unresolved python literals return
        (('dyn', value, tag), None) through ``_lower_maybe_dyn``."""
        idx, dt = self._lower_maybe_dyn(e, schema)
        if isinstance(idx, tuple):
            return self._materialise_dyn(idx, want)
        return idx, dt

    def _lower_maybe_dyn(self, e: Expr, schema: Schema):
        k = e.kind
        if k == "col":
            if e.name not in schema:
                raise KeyError(f"column not found: {e.name}")
            return self._push(kind=F.AE_COLUMN, name=e.name), schema[e.name]
        if k == "lit":
            if e.value is None:
                dt = e.dtype or T.Int32
                return self._push(kind=F.AE_LITERAL, dtype=dt.physical, lit=0, is_null=1), dt
            value, tag = literal_physical(e.value)
            if e.dtype is not None:
                v = float(value) if e.dtype.is_float() else (bool(value) if e.dtype == T.Boolean else int(value))
                return self._lit_node(v, e.dtype), e.dtype
            if isinstance(tag, str):
                return (value, tag), None
            return self._lit_node(value, tag), tag
        if k == "alias":
            idx, dt = self.lower_expr(e.lhs, schema)
            return self._push(kind=F.AE_ALIAS, lhs=idx, name=e.name), dt
        if k == "cast":
            idx, dt = self.lower_expr(e.lhs, schema, e.dtype)
            if isinstance(dt, T.DatetimeType) and isinstance(e.dtype, T.DatetimeType) and dt.time_unit != e.dtype.time_unit:
                raise TypeError(f"cast Datetime[{dt.time_unit}] -> Datetime[{e.dtype.time_unit}] (a multiply / floor-divide of the ticks) is not on this path")
            if dt == e.dtype:
                return idx, dt
            return self._push(kind=F.AE_CAST, lhs=idx, dtype=e.dtype.physical), e.dtype
        if k == "not":
            idx, dt = self.lower_expr(e.lhs, schema)
            if dt != T.Boolean:
                raise TypeError("~ needs a boolean expression")
            return self._push(kind=F.AE_NOT, lhs=idx), T.Boolean
        if k in ("is_null", "is_not_null"):
            idx, _ = self.lower_expr(e.lhs, schema)
            return self._push(kind=F.AE_IS_NULL if k == "is_null" else F.AE_IS_NOT_NULL, lhs=idx), T.Boolean
        if k == "fill_null":
            idx, dt = self.lower_expr(e.lhs, schema)
            li, ldt = self.lower_expr(e.rhs, schema, dt)        # the literal takes the column's dtype (python ints / floats are dynamic)
            if ldt.physical != dt.physical:
                raise TypeError(f"fill_null value of type {ldt} for a {dt} column")
            return self._push(kind=F.AE_FILL_NULL, lhs=idx, rhs=li), dt
        if k == "len":
            return self._push(kind=F.AE_LEN), T.UInt32
        if k == "agg":
            idx, dt = self.lower_expr(e.lhs, schema)
            if e.op == F.AGG_SUM:
                out = sum_dtype(dt)
            elif e.op == F.AGG_MEAN:
                out = T.Float32 if dt == T.Float32 else T.Float64
            elif e.op in (F.AGG_COUNT, F.AGG_LEN, F.AGG_N_UNIQUE):      # n_unique: any operand dtype, nothing rides in the node
                out = T.UInt32
            elif e.op in (F.AGG_VAR, F.AGG_STD):
                what = "var" if e.op == F.AGG_VAR else "std"
                if not (isinstance(dt, T.DataType) and dt.is_numeric()):      # Boolean, Date / Datetime, Categorical
                    raise TypeError(f"{what}() needs a numeric expression, got {dt}")
                # ddof rides in the literal slot of the AGG node (plx_aexpr.lit.u), as a date part's unit does
                return self._push(kind=F.AE_AGG, op=e.op, lhs=idx, lit=int(e.value)), (T.Float32 if dt == T.Float32 else T.Float64)
            elif e.op == F.AGG_QUANTILE:
                q, interpolation = e.value
                if not (isinstance(dt, T.DataType) and dt.is_numeric()):      # Boolean, Date / Datetime, Categorical
                    raise TypeError(f"{'median' if e.value == (0.5, 'linear') else 'quantile'}() needs a numeric expression, got {dt}")
                # q rides in the literal slot of the AGG node (plx_aexpr.lit.f64), the interpolation in its otherwise unread dtype slot
                return (self._push(kind=F.AE_AGG, op=e.op, lhs=idx, lit=float(q), dtype=F.QUANTILE_INTERPOLATIONS[interpolation]),
                        T.Float32 if dt == T.Float32 else T.Float64)
            else:
                out = dt
            return self._push(kind=F.AE_AGG, op=e.op, lhs=idx), out
        if k == "cum":
            # x.cum_sum(reverse=...): AE_CUMULATIVE with the operand in lhs, the plx_cum_op in `op` and reverse in the literal slot (plx_aexpr.lit.u), as a date
            # part's unit rides there.  The operand is a row-level expression: the refusals are by name, here, before anything runs
            self._check_row_operand(e)
            idx, dt = self.lower_expr(e.lhs, schema)
            return self._push(kind=F.AE_CUMULATIVE, op=e.op, lhs=idx, lit=int(bool(e.value))), cum_result_dtype(e.op, dt)
        if k == "rank":
            self._check_row_operand(e)
            idx, dt = self.lower_expr(e.lhs, schema)
            method, descending = e.value
            return self._push(kind=F.AE_RANK, op=F.RANK_METHODS[method], lhs=idx, lit=int(bool(descending))), rank_result_dtype(method, dt)
        if k == "shift":
            # x.shift(n, fill_value=v) / x.diff(n): AE_SHIFT with the operand in lhs, 0 / 1 in `op`, n in the literal slot (plx_aexpr.lit.i) and the fill literal,
            # typed as the operand, in rhs
            self._check_row_operand(e)
            idx, dt = self.lower_expr(e.lhs, schema)
            out = shift_result_dtype(e.op, dt)
            n, fill = e.value
            fi = -1 if fill is None else self._lit_node(shift_fill_literal(fill, dt), dt)
            return self._push(kind=F.AE_SHIFT, op=e.op, lhs=idx, rhs=fi, lit=max(-(2 ** 63), min(2 ** 63 - 1, int(n)))), out
        if k == "rolling":
            self._check_row_operand(e)
            idx, dt = self.lower_expr(e.lhs, schema)
            w, m, c = e.value
            return self._push(kind=F.AE_ROLLING, op=e.op, lhs=idx, lit=F.rolling_pack(w, m, c)), rolling_result_dtype(e.op, dt)
        if k == "window":
            f = e.lhs
            while f.kind == "alias":
                f = f.lhs
            if f.kind not in ROW_FUNCTION_KINDS and has_row_function(e.lhs):
                raise TypeError(f"{e!r}: under .over() a function that mixes a cumulative / ranking expression (or a shift / diff / rolling expression) with anything else is not built; put "
                                ".over(keys) directly on that expression (and on each aggregate) and the arithmetic outside")
            # f.over(k1, k2, ...): AE_WINDOW with the function in lhs and the first link of the key chain in rhs; one AE_WINDOW_KEY link per key (lhs = the key,
            # rhs = the next link or -1).  The arena is topological, so the links are pushed last key first.  The engine checks that f aggregates and the keys do not
            fi, fdt = self.lower_expr(e.lhs, schema)
            key_nodes = [self.lower_expr(key, schema)[0] for key in e.value]
            link = -1
            for ki in reversed(key_nodes):
                link = self._push(kind=F.AE_WINDOW_KEY, lhs=ki, rhs=link)
            return self._push(kind=F.AE_WINDOW, lhs=fi, rhs=link), fdt
        if k == "binary":
            return self._lower_binary(e, schema)
        if k == "ternary":
            return self._lower_ternary(e, schema)
        if k == "str_match":
            return self._lower_str_match(e, schema)
        if k == "dt_part":
            return self._lower_dt_part(e, schema)
        raise TypeError(f"unsupported expression {e!r}")

    def _lower_string_compare(self, e: Expr, schema: Schema):
        """Categorical column ==/!= string literal: the string is looked up in the column's dictionary and the physical codes
        are compared -- what the reference does for a Categorical against a string scalar
        (crates/polars-core/src/chunked_array/comparison/categorical.rs: the rev-map lookup, then `equal` on the physical).
        A string that is not in the dictionary equals no row.  Returns None when `e` is not such a comparison."""
        for col_side, lit_side in ((e.lhs, e.rhs), (e.rhs, e.lhs)):
            if lit_side.kind == "lit" and isinstance(lit_side.value, str):
                ci, cdt = self._lower_maybe_dyn(col_side, schema)
                if isinstance(ci, tuple) or not isinstance(cdt, T.Categorical):
                    raise TypeError("a string literal can only be compared with a dictionary-encoded (Categorical) column on this path")
                if e.op not in (F.OP_EQ, F.OP_NE):
                    raise TypeError("only == and != are supported between a Categorical column and a string")
                cats = cdt.categories
                code = cats.index(lit_side.value) if lit_side.value in cats else len(cats)
                phys = T.PHYSICAL_TO_DTYPE[cdt.physical]
                if code > int(__import__("numpy").iinfo(phys.np_dtype).max):      # absent string and a full code space: no row can match
                    return self._lit_node(e.op == F.OP_NE, T.Boolean), T.Boolean
                lit = self._lit_node(code, phys)
                return self._push(kind=F.AE_BINARY, op=e.op, lhs=ci, rhs=lit), T.Boolean
        return None

    def _lower_str_match(self, e: Expr, schema: Schema):
        """str.starts_with / ends_with / contains(literal) on a Categorical column: the predicate is decided once per dictionary entry -- on the device for a
        dictionary that lives there (plx_strdict_match: nothing is downloaded), in Python for a host list -- and the rows look their code up in the resulting
        bitmap (AE_BITMAP_LOOKUP; null code -> null, a code beyond the dictionary -> false)."""
        from . import frame as _frame
        what = STR_MATCH_NAMES[e.op]
        pattern = str_pattern_bytes(e.value, what)
        ci, cdt = self._lower_maybe_dyn(e.lhs, schema)
        if isinstance(ci, tuple) or not isinstance(cdt, T.Categorical):
            raise TypeError(f"str.{what} needs a dictionary-encoded (Categorical) column on this path, got {'a literal' if isinstance(ci, tuple) else cdt}")
        if len(pattern) > F.STR_MATCH_MAX_PATTERN:
            raise F.UnsupportedError(F.ERR_UNSUPPORTED, f"str.{what}: a pattern of {len(pattern)} bytes; patterns of more than {F.STR_MATCH_MAX_PATTERN} bytes are not on this path")
        cats = cdt.categories
        memo, key = self._lut_memo, (id(cats), e.op, pattern)
        if key in memo:
            return self._push(kind=F.AE_BITMAP_LOOKUP, lhs=ci, lut=memo[key]), T.Boolean
        host = None
        if hasattr(cats, "_load") and getattr(cats, "_h", 0) and cats._items is None:       # a device dictionary nobody has downloaded
            h = C.c_uint64()
            F.check(F.lib().plx_strdict_match(cats._h, e.op, pattern, len(pattern), C.byref(h)))
            lut, where = _frame.Series._from_handle("", h.value, T.Boolean), "device"
        else:
            import numpy as np
            host = np.array([bool(str_match_host(e.op, c, pattern)) for c in cats], dtype=bool)
            where = "host"
            if F._initialised:
                lut = _frame.Series("", host, T.Boolean)
            else:                                   # planning without a device (explain, describe_fusion, debug_program on placeholder frames)
                h = C.c_uint64()
                F.check(F.lib().plx_column_placeholder(F.BOOL, len(host), 0, 0, 0, 0, C.byref(h)))
                lut = _frame.Series._from_handle("", h.value, T.Boolean)
        memo[key] = lut
        self.luts.append(host)
        self.lut_columns.append(lut)
        self.notes.append(f"str.{what}({e.value!r}) over {len(cats)} categories [{where}]")
        return self._push(kind=F.AE_BITMAP_LOOKUP, lhs=ci, lut=lut), T.Boolean

    def _lower_dt_part(self, e: Expr, schema: Schema):
        """dt.<part>() of a Date / Datetime expression: AE_TEMPORAL with the part in `op` and the operand's unit (plx_time_unit) in the literal slot -- the engine sees
        physical Int32 / Int64 values and cannot tell a Date from a count, or microseconds from nanoseconds, any other way."""
        ci, cdt = self._lower_maybe_dyn(e.lhs, schema)
        unit = dt_unit(None if isinstance(ci, tuple) else cdt, e.op)          # TypeError: not temporal, or the time of day / date() of a Date
        note = f"{e!r} [{'Date' if unit == F.UNIT_DATE else 'Datetime[' + cdt.time_unit + ']'}]"              # the expression as written, for pl.last_plan() / explain()
        if note not in self.notes:
            self.notes.append(note)
        return self._push(kind=F.AE_TEMPORAL, op=e.op, lhs=ci, lit=unit), dt_part_dtype(e.op)

    def _lower_mixed_time_units(self, op: int, li: int, ldt, ri: int, rdt):
        """Datetime column <cmp> Datetime literal of another time unit (a python datetime is "us").  The reference coerces both sides to
        the COARSER unit (get_time_units, crates/polars-core/src/utils/mod.rs:804-811) and casts the finer side by floor division
        (chunked_array/logical/datetime.rs:59-66: `v.div_euclid(d)`).  No cast kernel runs here: the comparison is rewritten, exactly,
        into the column's own unit.  Column coarser than the literal: the literal is floor-divided.  Column finer by the factor f:
        floor(x / f) <= L  <=>  x <= f L + f - 1;  floor(x / f) >= L  <=>  x >= f L;  < and > shift L by one; == is both bounds, != neither."""
        cmp_ops = (F.OP_EQ, F.OP_NE, F.OP_LT, F.OP_LE, F.OP_GT, F.OP_GE)
        is_lit = lambda i: self.aexprs[i]["kind"] == F.AE_LITERAL and not self.aexprs[i]["is_null"]
        if op not in cmp_ops or is_lit(li) == is_lit(ri):
            raise TypeError(f"Datetime[{ldt.time_unit}] with Datetime[{rdt.time_unit}]: only comparisons of a column with a literal cross time units on this path")
        if is_lit(li):                                              # literal <op> column  ->  column <flipped op> literal
            li, ldt, ri, rdt = ri, rdt, li, ldt
            op = {F.OP_LT: F.OP_GT, F.OP_LE: F.OP_GE, F.OP_GT: F.OP_LT, F.OP_GE: F.OP_LE}.get(op, op)
        L = int(self.aexprs[ri]["lit"])
        cu, lu = ldt.ticks_per_second(), rdt.ticks_per_second()
        cmp = lambda o, v: self._push(kind=F.AE_BINARY, op=o, lhs=li, rhs=self._lit_node(int(v), ldt))
        if cu < lu:                                                 # the column's unit is the coarser one: only the literal is cast
            return cmp(op, L // (lu // cu)), T.Boolean
        f = cu // lu
        i64_min, i64_max = -(1 << 63), (1 << 63) - 1
        # x <= hi / x >= lo with bounds that may lie outside i64: then the comparison is constant for every non-null x (and stays null for nulls)
        le = lambda hi: cmp(F.OP_LE, i64_max) if hi >= i64_max else cmp(F.OP_LT, i64_min) if hi < i64_min else cmp(F.OP_LE, hi)
        ge = lambda lo: cmp(F.OP_GE, i64_min) if lo <= i64_min else cmp(F.OP_GT, i64_max) if lo > i64_max else cmp(F.OP_GE, lo)
        gt = lambda hi: cmp(F.OP_GT, i64_max) if hi >= i64_max else cmp(F.OP_GE, i64_min) if hi < i64_min else cmp(F.OP_GT, hi)
        lt = lambda lo: cmp(F.OP_LT, i64_min) if lo <= i64_min else cmp(F.OP_LE, i64_max) if lo > i64_max else cmp(F.OP_LT, lo)
        upper = lambda l: f * l + f - 1                             # floor(x / f) <= l  <=>  x <= upper(l)
        lower = lambda l: f * l                                     # floor(x / f) >= l  <=>  x >= lower(l)
        if op == F.OP_LE:
            return le(upper(L)), T.Boolean
        if op == F.OP_LT:
            return le(upper(L - 1)), T.Boolean
        if op == F.OP_GE:
            return ge(lower(L)), T.Boolean
        if op == F.OP_GT:
            return ge(lower(L + 1)), T.Boolean
        if op == F.OP_EQ:
            return self._push(kind=F.AE_BINARY, op=F.OP_AND, lhs=ge(lower(L)), rhs=le(upper(L))), T.Boolean
        return self._push(kind=F.AE_BINARY, op=F.OP_OR, lhs=lt(lower(L)), rhs=gt(upper(L))), T.Boolean

    def _coerce_pair(self, li, ldt, ri, rdt):
        """Type coercion of two operands that must meet in one dtype (type_coercion/binary.rs): a python literal (still a (value, tag) pair)
        takes the other side's dtype, then both sides are cast to their supertype.  Returns (li, ldt, ri, rdt) with ldt == rdt."""
        ldyn, rdyn = isinstance(li, tuple), isinstance(ri, tuple)
        if ldyn and rdyn:
            li, ldt = self._materialise_dyn(li, None)
            ri, rdt = self._materialise_dyn(ri, None)
            ldyn = rdyn = False
        if ldyn or rdyn:
            other_dt = rdt if ldyn else ldt
            value, tag = li if ldyn else ri
            if tag == "dyn_float" and (other_dt.is_integer() or other_dt == T.Boolean):
                # int column vs float literal: the column is cast to Float64
                oi = ri if ldyn else li
                oi = self._cast(oi, other_dt, T.Float64)
                lit_i, _ = self._materialise_dyn((value, tag), T.Float64)
                li, ri = (lit_i, oi) if ldyn else (oi, lit_i)
                ldt = rdt = T.Float64
            else:
                try:
                    lit_i, lit_dt = self._materialise_dyn((value, tag), other_dt)
                except OverflowError:
                    lit_i, lit_dt = self._materialise_dyn((value, tag), None)
                if ldyn:
                    li, ldt = lit_i, lit_dt
                else:
                    ri, rdt = lit_i, lit_dt
        if ldt != rdt or (isinstance(ldt, T.DataType) and ldt.physical != rdt.physical):
            if {ldt.name, rdt.name} <= {"Date", "Datetime"} and ldt != rdt:
                raise TypeError("cannot compare Date with Datetime on this path")
            st = T.supertype(ldt, rdt)
            li = self._cast(li, ldt, st)
            ri = self._cast(ri, rdt, st)
            ldt = rdt = st
        return li, ldt, ri, rdt

    def _lower_binary(self, e: Expr, schema: Schema):
        op = e.op
        if (e.lhs.kind == "lit" and isinstance(e.lhs.value, str)) or (e.rhs.kind == "lit" and isinstance(e.rhs.value, str)):
            return self._lower_string_compare(e, schema)
        li, ldt = self._lower_maybe_dyn(e.lhs, schema)
        ri, rdt = self._lower_maybe_dyn(e.rhs, schema)
        ldyn, rdyn = isinstance(li, tuple), isinstance(ri, tuple)
        if not ldyn and not rdyn and isinstance(ldt, T.DatetimeType) and isinstance(rdt, T.DatetimeType) and ldt.time_unit != rdt.time_unit:
            return self._lower_mixed_time_units(op, li, ldt, ri, rdt)
        if op in (F.OP_AND, F.OP_OR, F.OP_XOR):
            if ldyn or rdyn or ldt != T.Boolean or rdt != T.Boolean:
                raise TypeError("& | ^ need boolean operands on this path")
            return self._push(kind=F.AE_BINARY, op=op, lhs=li, rhs=ri), T.Boolean
        li, ldt, ri, rdt = self._coerce_pair(li, ldt, ri, rdt)
        if op in (F.OP_EQ, F.OP_NE, F.OP_LT, F.OP_LE, F.OP_GT, F.OP_GE):
            out = T.Boolean
        elif op == F.OP_TRUE_DIVIDE:
            out = ldt if ldt.is_float() else T.Float64
        else:
            out = ldt
        return self._push(kind=F.AE_BINARY, op=op, lhs=li, rhs=ri), out

    def _lower_ternary(self, e: Expr, schema: Schema):
        """when(cond).then(lhs).otherwise(rhs) (TernaryExpr): the branches meet in their supertype by the rules of a binary expression; an open otherwise, or a
        bare None on either side, is a null of the other branch's dtype."""
        pi, pdt = self.lower_expr(e.cond, schema)
        if pdt != T.Boolean:
            raise TypeError(f"when(...) needs a Boolean predicate, got {pdt}")
        bare_null = lambda x: x is None or (x.kind == "lit" and x.value is None and x.dtype is None)
        if bare_null(e.lhs) and bare_null(e.rhs):
            ai, adt = self.lower_expr(e.lhs, schema)
            return self._push(kind=F.AE_TERNARY, lhs=ai, rhs=self._null_node(adt), cond=pi), adt
        if bare_null(e.lhs) or bare_null(e.rhs):
            oi, odt = self.lower_expr(e.rhs if bare_null(e.lhs) else e.lhs, schema)
            ni = self._null_node(odt)
            ai, bi = (ni, oi) if bare_null(e.lhs) else (oi, ni)
            return self._push(kind=F.AE_TERNARY, lhs=ai, rhs=bi, cond=pi), odt
        ai, adt = self._lower_maybe_dyn(e.lhs, schema)
        bi, bdt = self._lower_maybe_dyn(e.rhs, schema)
        dyn = isinstance(ai, tuple) or isinstance(bi, tuple)
        if not dyn and isinstance(adt, T.DatetimeType) and isinstance(bdt, T.DatetimeType) and adt.time_unit != bdt.time_unit:
            raise TypeError(f"when/then/otherwise branches Datetime[{adt.time_unit}] and Datetime[{bdt.time_unit}]: casts between time units are not on this path")
        ai, adt, bi, bdt = self._coerce_pair(ai, adt, bi, bdt)
        return self._push(kind=F.AE_TERNARY, lhs=ai, rhs=bi, cond=pi), adt

    def _check_row_operand(self, e: Expr) -> None:
        """The operand of a cumulative / ranking expression is row-level: no aggregate, no window and no other cumulative / ranking expression inside."""
        what = row_function_name(e)

        def walk(x):
            if x.kind in ("agg", "len"):
                raise TypeError(f"{what}(): an aggregate ({x!r}) inside the operand of a cumulative / ranking expression is not built; the operand is a row-level expression")
            if x.kind == "window":
                raise TypeError(f"{what}(): a window expression ({x!r}) inside the operand of a cumulative / ranking expression is not built; compute it in with_columns first")
            if x.kind in ROW_FUNCTION_KINDS:
                raise TypeError(f"{what}(): a cumulative / ranking / shift / rolling expression ({x!r}) inside the operand of another one is not built; compute the inner one in with_columns first")
            for c in x.children():
                walk(c)
        walk(e.lhs)

    def _null_node(self, dt: T.DataType) -> int:
        return self._push(kind=F.AE_LITERAL, dtype=dt.physical, lit=0, is_null=1)

    # -- IR ----------------------------------------------------------------------------------
    def lower_node(self, n: Node) -> Tuple[int, Schema]:
        def push(**kw) -> int:
            node = dict(kind=0, input=-1, input_right=-1, predicate=-1, frame=None, exprs=[], keys=[], keys_right=[], how=0,
                        maintain_order=0, suffix="_right", sort_descending=[], sort_nulls_last=[], slice_offset=0, slice_len=0, coalesce=0)
            node.update(kw)
            self.irs.append(node)
            return len(self.irs) - 1

        k = n.kind
        if k == "scan":
            return push(kind=F.IR_SCAN, frame=n.frame), dict(n.frame.schema)
        if k == "filter":
            inp, schema = self.lower_node(n.input)
            p, dt = self.lower_expr(n.predicate, schema)
            if dt != T.Boolean:
                raise TypeError("filter predicate must be boolean")
            return push(kind=F.IR_FILTER, input=inp, predicate=p), schema
        if k in ("select", "with_columns"):
            inp, schema = self.lower_node(n.input)
            exprs, out_schema = [], ({} if k == "select" else dict(schema))
            for e in n.exprs:
                idx, dt = self.lower_expr(e, schema)
                exprs.append(idx)
                out_schema[expr_output_name(e)] = dt
            return push(kind=F.IR_SELECT if k == "select" else F.IR_HSTACK, input=inp, exprs=exprs), out_schema
        if k == "group_by":
            inp, schema = self.lower_node(n.input)
            keys, aggs, out_schema = [], [], {}
            for e in list(n.keys) + list(n.aggs):
                if has_row_function(e):
                    raise TypeError(f"group_by: a cumulative / ranking expression or a shift / diff / rolling expression ({e!r}) cannot stand in the keys or aggregates of a group_by: it keeps one value per "
                                    "row; use it in select / with_columns, with .over(keys) for partitions")
            for e in n.keys:
                idx, dt = self.lower_expr(e, schema)
                keys.append(idx)
                out_schema[expr_output_name(e)] = dt
            for e in n.aggs:
                idx, dt = self.lower_expr(e, schema)
                aggs.append(idx)
                out_schema[expr_output_name(e)] = dt
            return push(kind=F.IR_GROUPBY, input=inp, keys=keys, exprs=aggs, maintain_order=int(n.maintain_order)), out_schema
        if k == "join":
            li, ls = self.lower_node(n.left)
            ri, rs = self.lower_node(n.right)
            lk, rk = [], []
            for a, b in zip(n.left_on, n.right_on):
                ai, adt = self.lower_expr(a, ls)
                bi, bdt = self.lower_expr(b, rs)
                if isinstance(adt, T.DatetimeType) and isinstance(bdt, T.DatetimeType) and adt.time_unit != bdt.time_unit:
                    raise TypeError(f"join keys Datetime[{adt.time_unit}] and Datetime[{bdt.time_unit}]: casts between time units are not on this path")
                if adt.physical != bdt.physical:
                    st = T.supertype(adt, bdt)
                    ai = self._cast(ai, adt, st)
                    bi = self._cast(bi, bdt, st)
                lk.append(ai)
                rk.append(bi)
            if n.how not in JOIN_HOWS:
                raise ValueError(f"how must be one of {list(JOIN_HOWS)}, got {n.how!r}")
            how = JOIN_HOWS[n.how]
            order = JOIN_ORDERS[getattr(n, "maintain_order", "none")]
            coalesce = getattr(n, "coalesce", None)
            out_schema = join_schema(n.how, coalesce, n.left_on, n.right_on, ls, rs, n.suffix)
            return push(kind=F.IR_JOIN, input=li, input_right=ri, keys=lk, keys_right=rk, how=how, suffix=n.suffix, maintain_order=order, coalesce=JOIN_COALESCE[coalesce]), out_schema
        if k == "join_asof":
            # keys / keys_right: the by parts first, `on` last; the Datetime-unit and supertype rules of a join; Categorical by parts and a Boolean / Categorical `on` refused
            li, ls = self.lower_node(n.left)
            ri, rs = self.lower_node(n.right)
            if n.strategy not in F.ASOF_STRATEGIES:
                raise ValueError(f"strategy must be one of {list(F.ASOF_STRATEGIES)}, got {n.strategy!r}")
            if len(n.left_on) - 1 > F.ASOF_MAX_BY:
                raise ValueError(f"join_asof: {len(n.left_on) - 1} by parts; an as-of join takes 0..{F.ASOF_MAX_BY}")
            lk, rk, on_dt = [], [], None
            for j, (a, b) in enumerate(zip(n.left_on, n.right_on)):
                is_on = j == len(n.left_on) - 1
                what = "`on`" if is_on else f"by part {j} ({a!r} = {b!r})"
                ai, adt = self.lower_expr(a, ls)
                bi, bdt = self.lower_expr(b, rs)
                for dt in (adt, bdt):
                    if isinstance(dt, T.Categorical):
                        raise TypeError(f"join_asof: {what} is Categorical: " + ("`on` may be an integer, a float, a Date or a Datetime" if is_on else
                                        "Categorical by parts are not on this path yet (the two dictionaries would have to be reconciled); join on the codes of one shared dictionary, or on an integer key"))
                    if is_on and dt == T.Boolean:
                        raise TypeError("join_asof: `on` is Boolean: `on` may be an integer, a float, a Date or a Datetime")
                if isinstance(adt, T.DatetimeType) and isinstance(bdt, T.DatetimeType) and adt.time_unit != bdt.time_unit:
                    raise TypeError(f"join keys Datetime[{adt.time_unit}] and Datetime[{bdt.time_unit}]: casts between time units are not on this path")
                if _is_temporal(adt) != _is_temporal(bdt) or (_is_temporal(adt) and isinstance(adt, T.DatetimeType) != isinstance(bdt, T.DatetimeType)):
                    raise TypeError(f"join_asof: {what} is {adt} on the left and {bdt} on the right")
                st = adt
                if adt.physical != bdt.physical:
                    st = T.supertype(adt, bdt)
                    ai = self._cast(ai, adt, st)
                    bi = self._cast(bi, bdt, st)
                lk.append(ai)
                rk.append(bi)
                on_dt = st
            tol = -1
            if n.tolerance is not None:
                value, lit_dt = asof_tolerance_literal(n.tolerance, on_dt)
                tol = self._lit_node(value, lit_dt)
            out_schema = join_schema("left", n.coalesce, n.left_on, n.right_on, ls, rs, n.suffix)
            return push(kind=F.IR_JOIN_ASOF, input=li, input_right=ri, keys=lk, keys_right=rk, how=F.ASOF_STRATEGIES[n.strategy] | (F.ASOF_STRICT if n.strict else 0),
                        predicate=tol, suffix=n.suffix, coalesce=JOIN_COALESCE[n.coalesce]), out_schema
        if k == "sort":
            inp, schema = self.lower_node(n.input)
            keys = [self.lower_expr(e, schema)[0] for e in n.by]
            return push(kind=F.IR_SORT, input=inp, keys=keys, sort_descending=[int(bool(x)) for x in n.descending],
                        sort_nulls_last=[int(bool(x)) for x in n.nulls_last], maintain_order=int(n.maintain_order)), schema
        if k == "unique":
            inp, schema = self.lower_node(n.input)
            names = list(schema) if n.subset is None else list(n.subset)
            if n.keep not in F.UNIQUE_KEEPS:
                raise ValueError(f"keep must be one of {list(F.UNIQUE_KEEPS)}, got {n.keep!r}")
            keys = [self.lower_expr(Expr("col", name=name), schema)[0] for name in names]          # KeyError: column not found
            # the keep strategy rides in the otherwise unread `how` slot of the node (plx_unique_keep); both values of maintain_order are served in row order
            return push(kind=F.IR_DISTINCT, input=inp, keys=keys, how=F.UNIQUE_KEEPS[n.keep], maintain_order=int(bool(n.maintain_order))), schema
        if k == "slice":
            inp, schema = self.lower_node(n.input)
            offset = int(n.offset)
            from . import io as _io
            src = _io.scan_under(n.input)
            if src is not None:                  # the scan below reads only the row groups this slice overlaps: the offset counts from its first row
                offset -= src.window_skip(int(n.offset), int(n.length))
            return push(kind=F.IR_SLICE, input=inp, slice_offset=offset, slice_len=int(n.length)), schema
        raise TypeError(f"unsupported plan node {k}")

    # -- marshalling to the C structs -----------------------------------------------------------
    def to_c(self):
        keep: List[Any] = []
        n_ae = len(self.aexprs)
        ae = (F.AExpr * max(n_ae, 1))()
        for i, d in enumerate(self.aexprs):
            a = ae[i]
            a.kind, a.op, a.lhs, a.rhs, a.dtype, a.is_null, a.cond = d["kind"], d["op"], d["lhs"], d["rhs"], d["dtype"], d["is_null"], d["cond"]
            if d["kind"] == F.AE_LITERAL and not d["is_null"]:
                dt = d["dtype"]
                if dt == F.F64:
                    a.lit.f64 = float(d["lit"])
                elif dt == F.F32:
                    a.lit.f32 = float(d["lit"])
                elif dt in (F.U8, F.U16, F.U32, F.U64, F.BOOL):
                    a.lit.u = int(d["lit"]) & 0xFFFFFFFFFFFFFFFF
                else:
                    a.lit.i = int(d["lit"])
            if d["kind"] == F.AE_SHIFT:
                a.lit.i = int(d["lit"])            # n, signed
            if d["kind"] in (F.AE_TEMPORAL, F.AE_CUMULATIVE, F.AE_RANK, F.AE_ROLLING) or (d["kind"] == F.AE_AGG and d["op"] in (F.AGG_VAR, F.AGG_STD)):
                a.lit.u = int(d["lit"])            # the operand's time unit / the ddof of var and std rides in the literal slot, like a lookup bitmap's handle
            if d["kind"] == F.AE_AGG and d["op"] == F.AGG_QUANTILE:
                a.lit.f64 = float(d["lit"])        # q (the interpolation went into the dtype slot with every other field)
            if d["kind"] == F.AE_BITMAP_LOOKUP:
                a.lit.u = d["lut"]._h              # the lookup bitmap's column handle rides in the literal slot (plx_aexpr.lit)
                keep.append(d["lut"])
            if d["name"] is not None:
                b = d["name"].encode()
                keep.append(b)
                a.name = b
        n_ir = len(self.irs)
        ir = (F.IR * n_ir)()
        for i, d in enumerate(self.irs):
            r = ir[i]
            r.kind, r.input, r.input_right, r.predicate = d["kind"], d["input"], d["input_right"], d["predicate"]
            r.frame = d["frame"]._frame_handle() if d["frame"] is not None else 0
            for field, nfield in (("exprs", "n_exprs"), ("keys", "n_keys"), ("keys_right", "n_keys_right")):
                vals = d[field]
                arr = (C.c_int32 * max(len(vals), 1))(*vals)
                keep.append(arr)
                setattr(r, field, C.cast(arr, C.POINTER(C.c_int32)))
                setattr(r, nfield, len(vals))
            r.how, r.maintain_order = d["how"], d["maintain_order"]
            sb = d["suffix"].encode()
            keep.append(sb)
            r.suffix = sb
            if d["kind"] == F.IR_SORT:
                for field in ("sort_descending", "sort_nulls_last"):
                    arr = (C.c_uint8 * max(len(d[field]), 1))(*d[field])
                    keep.append(arr)
                    setattr(r, field, C.cast(arr, C.POINTER(C.c_uint8)))
            r.slice_offset, r.slice_len = d["slice_offset"], d["slice_len"]
            r.coalesce = d["coalesce"]
        return ir, n_ir, ae, n_ae, keep


def expr_output_name(e: Expr) -> str:
    """Output column name: alias, else the leftmost leaf column (polars convention)."""
    if e.kind == "alias":
        return e.name
    if e.kind == "col":
        return e.name
    if e.kind == "len":
        return "len"
    if e.kind == "lit":
        return "literal"
    return expr_output_name(e.lhs)
