"""Expression DSL mirroring the subset of ``polars.Expr`` that reaches the hot path
(AExpr::{Column, Literal, BinaryExpr, Cast, Agg, Len} and Operator::{Eq..Or},
crates/polars-plan/src/plans/aexpr/mod.rs:150-259, dsl/expr/mod.rs:683-707).
"""
from __future__ import annotations

import datetime as _dt
from typing import Any, Optional

import numpy as np

from . import _ffi as F
from . import datatypes as T


class Expr:
    __slots__ = ("kind", "op", "lhs", "rhs", "name", "value", "dtype", "cond")

    def __init__(self, kind: str, op: Optional[int] = None, lhs: "Optional[Expr]" = None, rhs: "Optional[Expr]" = None,
                 name: Optional[str] = None, value: Any = None, dtype: Optional[T.DataType] = None, cond: "Optional[Expr]" = None):
        self.kind, self.op, self.lhs, self.rhs, self.name, self.value, self.dtype = kind, op, lhs, rhs, name, value, dtype
        self.cond = cond        # kind "ternary": the predicate (lhs = then, rhs = otherwise or None)

    def children(self):
        """The expressions this one reads, for walkers: lhs, rhs and a ternary's predicate."""
        return [c for c in (self.lhs, self.rhs, self.cond) if c is not None] + (list(self.value) if self.kind == "window" else [])

    # -- operators ---------------------------------------------------------------------
    def _bin(self, op: int, other: Any, swap: bool = False) -> "Expr":
        o = other if isinstance(other, Expr) else lit(other)
        return Expr("binary", op, o, self) if swap else Expr("binary", op, self, o)

    def __add__(self, o): return self._bin(F.OP_PLUS, o)
    def __radd__(self, o): return self._bin(F.OP_PLUS, o, True)
    def __sub__(self, o): return self._bin(F.OP_MINUS, o)
    def __rsub__(self, o): return self._bin(F.OP_MINUS, o, True)
    def __mul__(self, o): return self._bin(F.OP_MULTIPLY, o)
    def __rmul__(self, o): return self._bin(F.OP_MULTIPLY, o, True)
    def __truediv__(self, o): return self._bin(F.OP_TRUE_DIVIDE, o)
    def __rtruediv__(self, o): return self._bin(F.OP_TRUE_DIVIDE, o, True)
    def __floordiv__(self, o): return self._bin(F.OP_FLOOR_DIVIDE, o)
    def __rfloordiv__(self, o): return self._bin(F.OP_FLOOR_DIVIDE, o, True)
    def __mod__(self, o): return self._bin(F.OP_MODULUS, o)
    def __rmod__(self, o): return self._bin(F.OP_MODULUS, o, True)
    def __eq__(self, o): return self._bin(F.OP_EQ, o)  # type: ignore[override]
    def __ne__(self, o): return self._bin(F.OP_NE, o)  # type: ignore[override]
    def __lt__(self, o): return self._bin(F.OP_LT, o)
    def __le__(self, o): return self._bin(F.OP_LE, o)
    def __gt__(self, o): return self._bin(F.OP_GT, o)
    def __ge__(self, o): return self._bin(F.OP_GE, o)
    def __and__(self, o): return self._bin(F.OP_AND, o)
    def __rand__(self, o): return self._bin(F.OP_AND, o, True)
    def __or__(self, o): return self._bin(F.OP_OR, o)
    def __ror__(self, o): return self._bin(F.OP_OR, o, True)
    def __xor__(self, o): return self._bin(F.OP_XOR, o)
    def __invert__(self): return Expr("not", lhs=self)
    def __hash__(self): return id(self)

    def __neg__(self): return lit(0)._bin(F.OP_MINUS, self)                      # 0 - x, as the reference lowers unary minus for integers / floats
    def is_between(self, lower, upper, closed: str = "both") -> "Expr":
        """lower <= x <= upper (py-polars expr.is_between); closed in {"both", "left", "right", "none"}."""
        if closed not in ("both", "left", "right", "none"):
            raise ValueError(f"closed must be one of 'both', 'left', 'right', 'none', got {closed!r}")
        lo = self.__ge__(lower) if closed in ("both", "left") else self.__gt__(lower)
        hi = self.__le__(upper) if closed in ("both", "right") else self.__lt__(upper)
        return lo & hi

    def is_in(self, values) -> "Expr":
        """x is one of a short list of literals (Expr.is_in with a literal list): OR of equalities; a null x gives null, as the
        reference's is_in does with nulls_equal=False.  Strings compare through the column's dictionary like ==."""
        vals = [v for v in values if v is not None]      # nulls_equal=False: a null in the list equals nothing
        if not vals:
            return self.ne(self)                         # all-false for every non-null x, null for null x
        out = self.eq(vals[0])
        for v in vals[1:]:
            out = out | self.eq(v)
        return out

    def is_null(self) -> "Expr": return Expr("is_null", lhs=self)
    def is_not_null(self) -> "Expr": return Expr("is_not_null", lhs=self)
    def fill_null(self, value: Any) -> "Expr":
        """Replace nulls by a literal (py-polars expr.fill_null(value)); strategies are outside the hot path."""
        if value is None or isinstance(value, Expr) and value.kind != "lit":
            raise TypeError("fill_null takes a non-null literal on this path")
        return Expr("fill_null", lhs=self, rhs=value if isinstance(value, Expr) else lit(value))

    def eq(self, o): return self.__eq__(o)
    def ne(self, o): return self.__ne__(o)
    def not_(self): return self.__invert__()

    # -- aggregations -------------------------------------------------------------------
    def sum(self): return Expr("agg", F.AGG_SUM, self)
    def mean(self): return Expr("agg", F.AGG_MEAN, self)
    def min(self): return Expr("agg", F.AGG_MIN, self)
    def max(self): return Expr("agg", F.AGG_MAX, self)
    def count(self): return Expr("agg", F.AGG_COUNT, self)
    def len(self): return Expr("agg", F.AGG_LEN, self)

    def var(self, ddof: int = 1) -> "Expr":
        """Variance of the non-null values with `ddof` delta degrees of freedom (py-polars expr.var): Float64 (Float32 stays Float32), null when at most `ddof`
        values are left.  The node keeps ddof in `value`."""
        return Expr("agg", F.AGG_VAR, self, value=check_ddof(ddof, "var"))

    def std(self, ddof: int = 1) -> "Expr":
        """Standard deviation: the square root of var(ddof)."""
        return Expr("agg", F.AGG_STD, self, value=check_ddof(ddof, "std"))

    def quantile(self, quantile: float, interpolation: str = "nearest") -> "Expr":
        """The quantile of the non-null values (py-polars expr.quantile): `quantile` a real number in [0, 1], interpolation one of "nearest", "lower", "higher",
        "midpoint", "linear".  Float64 (Float32 stays Float32), null without a valid value; values rank in the sort's order (NaN greatest).  The node keeps
        (q, interpolation) in `value`."""
        return Expr("agg", F.AGG_QUANTILE, self, value=(check_quantile(quantile), check_interpolation(interpolation)))

    def median(self) -> "Expr":
        """quantile(0.5, "linear")."""
        return Expr("agg", F.AGG_QUANTILE, self, value=(0.5, "linear"))

    def n_unique(self) -> "Expr":
        """The number of distinct values, a null counting as one value of its own (py-polars expr.n_unique): UInt32, never null.  Values are equal by the sort's
        equality (every NaN equals every NaN, -0 == +0).  Any integer, float, Boolean, Date / Datetime or Categorical expression."""
        return Expr("agg", F.AGG_N_UNIQUE, self)

    # -- windows --------------------------------------------------------------------------
    def over(self, *partition_by: Any, order_by: Any = None, mapping_strategy: str = "group_to_rows") -> "Expr":
        """The aggregate per partition of the keys, given back on every row (py-polars expr.over with mapping_strategy="group_to_rows"): height and row order stay
        the frame's, row r holds the value of the partition of row r.  `self` must reduce to one value per partition (every column below an aggregate); 1..8 keys,
        strings or expressions, given one by one or as one list.  Partitions form as group_by groups do (a null key is a partition of its own).  order_by and the
        "join" / "explode" mappings are not built: they raise instead of being ignored."""
        keys = check_over(partition_by, order_by, mapping_strategy)
        return Expr("window", lhs=self, value=keys)

    # -- cumulative and ranking functions ---------------------------------------------------
    def cum_sum(self, *, reverse: bool = False) -> "Expr":
        """The running sum (py-polars expr.cum_sum): one value per row, a null row stays null and adds nothing.  Int8 / Int16 / UInt8 / UInt16 -> Int64, Boolean ->
        UInt32, every other integer and float dtype keeps its own; integers wrap, Float32 accumulates as the sum aggregate does.  reverse=True scans from the last
        row to the first.  Plain: over the whole column; directly under .over(keys): within each partition, in the frame's row order."""
        return Expr("cum", F.CUM_SUM, self, value=check_reverse(reverse, "cum_sum"))

    def cum_min(self, *, reverse: bool = False) -> "Expr":
        """The running minimum (py-polars expr.cum_min): the dtype stays, a null row stays null; a NaN is ignored unless every valid value so far is NaN, as min() does."""
        return Expr("cum", F.CUM_MIN, self, value=check_reverse(reverse, "cum_min"))

    def cum_max(self, *, reverse: bool = False) -> "Expr":
        """The running maximum (py-polars expr.cum_max); see cum_min."""
        return Expr("cum", F.CUM_MAX, self, value=check_reverse(reverse, "cum_max"))

    def cum_count(self, *, reverse: bool = False) -> "Expr":
        """The number of non-null values up to and including the row (py-polars expr.cum_count): UInt32, never null; any dtype."""
        return Expr("cum", F.CUM_COUNT, self, value=check_reverse(reverse, "cum_count"))

    def rank(self, method: str = "average", *, descending: bool = False) -> "Expr":
        """The rank of every value (py-polars expr.rank): method one of "average" (Float64), "min", "max", "dense", "ordinal" (UInt32).  A null row's rank is null and
        nulls take no part.  Values rank in the sort's order (NaN greatest, all NaNs tie, -0 == +0); "ordinal" breaks ties by row order, also when descending.
        Plain: over the whole column; directly under .over(keys): within each partition."""
        return Expr("rank", F.RANK_METHODS[check_rank_method(method)], self, value=(method, check_reverse(descending, "rank", "descending")))

    # -- shift / diff and the fixed-window rolling functions ------------------------------------
    def shift(self, n: int = 1, *, fill_value: Any = None) -> "Expr":
        """Row i takes the operand's row i - n (py-polars expr.shift): n any integer, negative looks ahead, 0 is the operand itself, |n| >= the partition length
        vacates every row.  Vacated rows are null, or hold `fill_value` (a literal the column's dtype can hold exactly) and are valid.  Dtype, name and the validity
        of the moved rows are the operand's; every column dtype is taken.  Plain: over the whole column; directly under .over(keys): within each partition, in the
        frame's row order."""
        return Expr("shift", F.SHIFT_SHIFT, self, value=(check_shift_n(n, "shift"), check_fill_value(fill_value)))

    def diff(self, n: int = 1, null_behavior: str = "ignore") -> "Expr":
        """x[i] - x[i - n] (py-polars expr.diff), null where either row is null or row i - n lies outside the partition.  UInt8 -> Int16, UInt16 -> Int32, UInt32 /
        UInt64 -> Int64, signed integers and floats keep their dtype; integers wrap.  null_behavior="drop" changes the height and is not built."""
        if null_behavior != "ignore":
            raise ValueError(f"diff(null_behavior={null_behavior!r}) is not built: the height is kept on this path, only null_behavior=\"ignore\" is served")
        return Expr("shift", F.SHIFT_DIFF, self, value=(check_shift_n(n, "diff"), None))

    def _rolling(self, what: str, window_size: Any, weights: Any, min_samples: Any, center: Any) -> "Expr":
        return Expr("rolling", F.ROLLING_OPS[what], self, value=check_rolling(what, window_size, weights, min_samples, center))

    def rolling_sum(self, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> "Expr":
        """The sum over a window of `window_size` rows (py-polars expr.rolling_sum): the window of row i is the rows [i - window_size + 1, i], or centered
        [i + h - window_size + 1, i + h] with h = (window_size - 1) // 2, clipped to the partition; null where it holds fewer than `min_samples` (default:
        window_size) non-null values.  The dtype of cum_sum.  Weights and the temporal form ("7d") are not built."""
        return self._rolling("rolling_sum", window_size, weights, min_samples, center)

    def rolling_mean(self, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> "Expr":
        """The mean of the window's non-null values (py-polars expr.rolling_mean): Float64, a Float32 operand stays Float32; see rolling_sum."""
        return self._rolling("rolling_mean", window_size, weights, min_samples, center)

    def rolling_min(self, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> "Expr":
        """The minimum of the window's non-null values (py-polars expr.rolling_min): the dtype stays (Date / Datetime included); a NaN is ignored unless every valid
        value of the window is NaN; see rolling_sum."""
        return self._rolling("rolling_min", window_size, weights, min_samples, center)

    def rolling_max(self, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> "Expr":
        """The maximum of the window's non-null values (py-polars expr.rolling_max); see rolling_min."""
        return self._rolling("rolling_max", window_size, weights, min_samples, center)

    # -- misc -----------------------------------------------------------------------------
    @property
    def str(self) -> "ExprStringNameSpace":
        """String predicates on a dictionary-encoded (Categorical) column: str.starts_with / ends_with / contains of a literal."""
        return ExprStringNameSpace(self)

    @property
    def dt(self) -> "ExprDateTimeNameSpace":
        """The parts of a Date / Datetime column: dt.year / month / day / quarter / weekday / ordinal_day / hour / minute / second / date."""
        return ExprDateTimeNameSpace(self)

    def alias(self, name: str) -> "Expr": return Expr("alias", lhs=self, name=name)
    def cast(self, dtype: T.DataType) -> "Expr": return Expr("cast", lhs=self, dtype=dtype)

    def __repr__(self) -> str:
        if self.kind == "col": return f"col({self.name!r})"
        if self.kind == "lit": return f"lit({self.value!r})"
        if self.kind == "binary": return f"({self.lhs!r} <{self.op}> {self.rhs!r})"
        if self.kind == "agg" and self.op in (F.AGG_VAR, F.AGG_STD): return f"{self.lhs!r}.{'var' if self.op == F.AGG_VAR else 'std'}(ddof={self.value})"
        if self.kind == "agg" and self.op == F.AGG_QUANTILE:
            return f"{self.lhs!r}.median()" if self.value == (0.5, "linear") else f"{self.lhs!r}.quantile({self.value[0]!r}, {self.value[1]!r})"
        if self.kind == "agg" and self.op == F.AGG_N_UNIQUE: return f"{self.lhs!r}.n_unique()"
        if self.kind == "agg": return f"{self.lhs!r}.agg{self.op}()"
        if self.kind == "cum": return f"{self.lhs!r}.{CUM_NAMES[self.op]}({'reverse=True' if self.value else ''})"
        if self.kind == "rank": return f"{self.lhs!r}.rank({self.value[0]!r}{', descending=True' if self.value[1] else ''})"
        if self.kind == "shift":
            n, fill = self.value
            return f"{self.lhs!r}.{'diff' if self.op == F.SHIFT_DIFF else 'shift'}({n}{'' if fill is None else f', fill_value={fill!r}'})"
        if self.kind == "rolling":
            w, m, c = self.value
            return f"{self.lhs!r}.{ROLLING_NAMES[self.op]}({w}{'' if m == w else f', min_samples={m}'}{', center=True' if c else ''})"
        if self.kind == "window": return f"{self.lhs!r}.over([{', '.join(repr(k) for k in self.value)}])"
        if self.kind == "alias": return f"{self.lhs!r}.alias({self.name!r})"
        if self.kind == "cast": return f"{self.lhs!r}.cast({self.dtype})"
        if self.kind == "not": return f"~{self.lhs!r}"
        if self.kind in ("is_null", "is_not_null"): return f"{self.lhs!r}.{self.kind}()"
        if self.kind == "fill_null": return f"{self.lhs!r}.fill_null({self.rhs!r})"
        if self.kind == "str_match": return f"{self.lhs!r}.str.{STR_MATCH_NAMES[self.op]}({self.value!r})"
        if self.kind == "dt_part": return f"{self.lhs!r}.dt.{DT_PART_NAMES[self.op]}()"
        if self.kind == "ternary":
            return f"when({self.cond!r}).then({self.lhs!r})" + (f".otherwise({self.rhs!r})" if self.rhs is not None else "")
        return self.kind

    def __bool__(self):
        raise TypeError("the truth value of an Expr is ambiguous; use & / | / ~")


def check_ddof(ddof: Any, what: str) -> int:
    """ddof of var / std: an integer 0..255 (it travels in one byte of the finalisation spec); anything else is a TypeError."""
    if isinstance(ddof, (bool, np.bool_)) or not isinstance(ddof, (int, np.integer)) or not 0 <= int(ddof) <= 255:
        raise TypeError(f"{what}(ddof=...) takes an integer 0..255, got {ddof!r}")
    return int(ddof)


def check_quantile(q: Any) -> float:
    """q of a quantile: a real number in [0, 1]; anything else (NaN, a number outside, no number at all) is a ValueError."""
    if isinstance(q, (bool, np.bool_)) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0.0 <= float(q) <= 1.0:
        raise ValueError(f"quantile takes a real number in [0, 1], got {q!r}")
    return float(q)


def check_keep(keep: Any) -> str:
    """The keep strategy of unique(): one of "any", "first", "last", "none"."""
    if not isinstance(keep, str) or keep not in F.UNIQUE_KEEPS:
        raise ValueError(f"keep must be one of {list(F.UNIQUE_KEEPS)}, got {keep!r}")
    return keep


CUM_NAMES = {F.CUM_SUM: "cum_sum", F.CUM_MIN: "cum_min", F.CUM_MAX: "cum_max", F.CUM_COUNT: "cum_count"}


def check_reverse(flag: Any, what: str, name: str = "reverse") -> bool:
    """reverse= of a cumulative function / descending= of rank: a bool; anything else is a TypeError (a truthy string would otherwise turn the scan around)."""
    if not isinstance(flag, (bool, np.bool_)):
        raise TypeError(f"{what}({name}=...) takes a bool, got {flag!r}")
    return bool(flag)


ROLLING_NAMES = {v: k for k, v in F.ROLLING_OPS.items()}


def check_shift_n(n: Any, what: str) -> int:
    """n of shift / diff: any Python or numpy integer; a bool, a float or None is a TypeError."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise TypeError(f"{what}(n=...) takes an integer, got n={n!r}")
    return int(n)


def check_fill_value(fill_value: Any) -> Any:
    """fill_value of shift: None or a literal; whether the column's dtype holds it is decided where the dtype is known (plan.shift_fill_literal)."""
    if isinstance(fill_value, Expr):
        if fill_value.kind == "lit" and fill_value.dtype is None:
            return fill_value.value
        raise TypeError(f"shift(fill_value=...): an expression as fill_value ({fill_value!r}) is not built; fill_value is a literal")
    return fill_value


def check_rolling(what: str, window_size: Any, weights: Any, min_samples: Any, center: Any) -> tuple:
    """(window_size, min_samples, center) of a rolling function: window_size an integer >= 1, min_samples an integer in 1..window_size (default: window_size),
    center a bool.  Weights and a string window_size (the temporal form) are refused by name."""
    if weights is not None:
        raise ValueError(f"{what}(weights=...) is not built: only unweighted windows are served")
    if isinstance(window_size, str):
        raise ValueError(f"{what}(window_size={window_size!r}): a temporal window (and by=) is not built; window_size is a number of rows")
    if isinstance(window_size, (bool, np.bool_)) or not isinstance(window_size, (int, np.integer)):
        raise TypeError(f"{what}(window_size=...) takes an integer, got window_size={window_size!r}")
    window_size = int(window_size)
    if not 1 <= window_size <= F.ROLLING_MAX_WINDOW:
        raise ValueError(f"{what}: window_size must be at least 1 (and below 2^31), got window_size={window_size}")
    if min_samples is None:
        min_samples = window_size
    if isinstance(min_samples, (bool, np.bool_)) or not isinstance(min_samples, (int, np.integer)):
        raise TypeError(f"{what}(min_samples=...) takes an integer, got min_samples={min_samples!r}")
    min_samples = int(min_samples)
    if not 1 <= min_samples <= window_size:
        raise ValueError(f"{what}: min_samples must lie in 1..window_size ({window_size}), got min_samples={min_samples}")
    return window_size, min_samples, check_reverse(center, what, "center")


def check_rank_method(method: Any) -> str:
    """The ranking method: one of "average", "min", "max", "dense", "ordinal" ("random" is not built)."""
    if not isinstance(method, str) or method not in F.RANK_METHODS:
        raise ValueError(f"rank method must be one of {list(F.RANK_METHODS)}, got {method!r}")
    return method


def check_over(partition_by: Any, order_by: Any = None, mapping_strategy: Any = "group_to_rows") -> tuple:
    """The keys of Expr.over as a tuple of expressions: strings name columns, one list / tuple argument is the key list itself.  ValueError for no key, for a
    mapping other than "group_to_rows" and for order_by (every aggregate here is order-insensitive; the argument is refused, not ignored); TypeError for a key
    that is neither a string nor an expression."""
    if mapping_strategy != "group_to_rows":
        raise ValueError(f"over(mapping_strategy={mapping_strategy!r}): only 'group_to_rows' is on this path ('join' and 'explode' are not built)")
    if order_by is not None:
        raise ValueError("over(order_by=...): ordered windows are not built on this path (every aggregate here is order-insensitive)")
    keys = list(partition_by)
    if keys and not keys[1:] and isinstance(keys[0], (list, tuple)):      # (len is pl.len() in this module)
        keys = list(keys[0])
    if not keys:
        raise ValueError("over() needs at least one partition key")
    out = []
    for k in keys:
        if isinstance(k, str):
            out.append(col(k))
        elif isinstance(k, Expr):
            out.append(k)
        else:
            raise TypeError(f"over(): a partition key is a column name or an expression, got {type(k).__name__}")
    return tuple(out)


def check_interpolation(interpolation: Any) -> str:
    """One of the five interpolations on this path ("equiprobable" is not built)."""
    if not isinstance(interpolation, str) or interpolation not in F.QUANTILE_INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {sorted(F.QUANTILE_INTERPOLATIONS)}, got {interpolation!r}")
    return interpolation


STR_MATCH_NAMES = {F.STR_STARTS_WITH: "starts_with", F.STR_ENDS_WITH: "ends_with", F.STR_CONTAINS: "contains"}


def str_pattern_bytes(pattern: Any, what: str) -> bytes:
    """The bytes a string predicate compares with: the UTF-8 bytes of a str, or bytes as they are.  Anything else -- another column, an expression -- is refused:
    only literal patterns are on this path."""
    if isinstance(pattern, Expr):
        if pattern.kind == "lit" and isinstance(pattern.value, (str, bytes)):
            pattern = pattern.value
        else:
            raise TypeError(f"str.{what}: the pattern must be a literal str or bytes; a pattern taken from an expression (another column) is not on this path")
    if isinstance(pattern, str):
        return pattern.encode("utf-8")
    if isinstance(pattern, (bytes, bytearray)):
        return bytes(pattern)
    raise TypeError(f"str.{what}: the pattern must be a literal str or bytes, got {type(pattern).__name__}")


def str_match_host(kind: int, value, pattern):
    """The reference semantics on the host, for one string (str or bytes; None stays None): Python's startswith / endswith / in on the UTF-8 bytes."""
    if value is None:
        return None
    b = value.encode("utf-8", errors="surrogateescape") if isinstance(value, str) else bytes(value)
    p = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
    return b.startswith(p) if kind == F.STR_STARTS_WITH else b.endswith(p) if kind == F.STR_ENDS_WITH else p in b


class ExprStringNameSpace:
    """pl.col("s").str: the string predicates of py-polars' expr.str that are on the hot path.  The result is an ordinary Boolean expression (null where the
    string is null): a filter predicate, an operand of ~ & |, the condition of when/then/otherwise, a group key or an output column."""

    def __init__(self, expr: Expr):
        self._expr = expr

    def _match(self, kind: int, pattern: Any) -> Expr:
        str_pattern_bytes(pattern, STR_MATCH_NAMES[kind])          # (type check now; the bytes are taken again at lowering)
        if isinstance(pattern, Expr):
            pattern = pattern.value
        return Expr("str_match", op=kind, lhs=self._expr, value=bytes(pattern) if isinstance(pattern, bytearray) else pattern)

    def starts_with(self, prefix: Any) -> Expr:
        return self._match(F.STR_STARTS_WITH, prefix)

    def ends_with(self, suffix: Any) -> Expr:
        return self._match(F.STR_ENDS_WITH, suffix)

    def contains(self, pattern: Any, *, literal: bool = True) -> Expr:
        if not literal:
            raise TypeError("str.contains(literal=False): regular expressions are not on this path; pass literal=True (the default here) for a substring test")
        return self._match(F.STR_CONTAINS, pattern)


DT_PART_NAMES = {F.PART_YEAR: "year", F.PART_MONTH: "month", F.PART_DAY: "day", F.PART_QUARTER: "quarter", F.PART_WEEKDAY: "weekday",
                 F.PART_ORDINAL_DAY: "ordinal_day", F.PART_HOUR: "hour", F.PART_MINUTE: "minute", F.PART_SECOND: "second", F.PART_DATE: "date"}
DT_DATETIME_ONLY = (F.PART_HOUR, F.PART_MINUTE, F.PART_SECOND, F.PART_DATE)      # the time of day, and the day of an instant: a Date has neither


def dt_part_dtype(part: int) -> T.DataType:
    """Output dtype of a date part, as the reference's: year Int32, ordinal_day Int16, date Date, every other part Int8."""
    return T.Int32 if part == F.PART_YEAR else T.Int16 if part == F.PART_ORDINAL_DAY else T.Date if part == F.PART_DATE else T.Int8


def dt_unit(dtype: T.DataType, part: int) -> int:
    """plx_time_unit of a logical dtype for dt.<part>(); TypeError for a dtype that is not temporal, and for the time of day or date() of a Date."""
    name = DT_PART_NAMES[part]
    if isinstance(dtype, T.DatetimeType):
        return {"ms": F.UNIT_MS, "us": F.UNIT_US, "ns": F.UNIT_NS}[dtype.time_unit]
    if dtype == T.Date:
        if part in DT_DATETIME_ONLY:
            raise TypeError(f"dt.{name}() needs a Datetime column, got Date" + (" (a Date has no time of day)" if part != F.PART_DATE else " (it is a date already)"))
        return F.UNIT_DATE
    raise TypeError(f"dt.{name}() needs a Date or Datetime column, got {'a literal' if dtype is None else dtype}")


class ExprDateTimeNameSpace:
    """pl.col("d").dt: the date parts of py-polars' expr.dt that are on the hot path.  The result is an ordinary integer expression (Date for dt.date()), null where
    the value is null, named like the column: a filter operand, a group key (its range is known without a pass over the data; year and date take it from the column's range), an aggregate source, a branch of
    when/then/otherwise or an output column.  Proleptic Gregorian calendar; weekday is ISO (Monday = 1 .. Sunday = 7)."""

    def __init__(self, expr: Expr):
        self._expr = expr

    def _part(self, part: int) -> Expr:
        return Expr("dt_part", op=part, lhs=self._expr)

    def year(self) -> Expr: return self._part(F.PART_YEAR)
    def month(self) -> Expr: return self._part(F.PART_MONTH)
    def day(self) -> Expr: return self._part(F.PART_DAY)
    def quarter(self) -> Expr: return self._part(F.PART_QUARTER)
    def weekday(self) -> Expr: return self._part(F.PART_WEEKDAY)
    def ordinal_day(self) -> Expr: return self._part(F.PART_ORDINAL_DAY)
    def hour(self) -> Expr: return self._part(F.PART_HOUR)
    def minute(self) -> Expr: return self._part(F.PART_MINUTE)
    def second(self) -> Expr: return self._part(F.PART_SECOND)
    def date(self) -> Expr: return self._part(F.PART_DATE)


def _as_expr(x: Any) -> Expr:
    return x if isinstance(x, Expr) else lit(x)


class When:
    """pl.when(predicate): waits for .then(value) (py-polars functions/whenthen.py)."""

    def __init__(self, predicate: Expr, chain: tuple = ()):
        self._predicate, self._chain = _as_expr(predicate), chain

    def then(self, value: Any) -> "Then":
        return Then(self._chain + ((self._predicate, _as_expr(value)),))

    def __repr__(self) -> str:
        return "".join(f"when({p!r}).then({v!r})." for p, v in self._chain) + f"when({self._predicate!r})"


class Then(Expr):
    """when(p).then(a): an expression of kind "ternary" whose otherwise is still open -- a null of a's dtype until .otherwise(b) closes it.
    A chain when(p1).then(a1).when(p2).then(a2).otherwise(b) nests in the falsy branch: the first true predicate wins."""
    __slots__ = ("_chain",)

    def __init__(self, chain: tuple, otherwise: Optional[Expr] = None):
        tail = otherwise
        for p, v in reversed(chain[1:]):
            tail = Expr("ternary", lhs=v, rhs=tail, cond=p)
        Expr.__init__(self, "ternary", lhs=chain[0][1], rhs=tail, cond=chain[0][0])
        self._chain = chain

    def when(self, predicate: Any) -> When:
        return When(predicate, self._chain)

    def otherwise(self, value: Any) -> Expr:
        closed = Then(self._chain, _as_expr(value))
        return Expr("ternary", lhs=closed.lhs, rhs=closed.rhs, cond=closed.cond)


def when(predicate: Any) -> When:
    return When(predicate)


def col(name: str) -> Expr:
    return Expr("col", name=name)


def lit(value: Any, dtype: Optional[T.DataType] = None) -> Expr:
    return Expr("lit", value=value, dtype=dtype)


def len() -> Expr:  # noqa: A001 - mirrors pl.len()
    return Expr("len")


def sum(name: str) -> Expr:  # noqa: A001
    return col(name).sum()


def mean(name: str) -> Expr:
    return col(name).mean()


def min(name: str) -> Expr:  # noqa: A001
    return col(name).min()


def max(name: str) -> Expr:  # noqa: A001
    return col(name).max()


def count(name: str) -> Expr:
    return col(name).count()


def var(name: str, ddof: int = 1) -> Expr:
    return col(name).var(ddof)


def std(name: str, ddof: int = 1) -> Expr:
    return col(name).std(ddof)


def median(name: str) -> Expr:
    return col(name).median()


def quantile(name: str, quantile: float, interpolation: str = "nearest") -> Expr:  # noqa: A002
    return col(name).quantile(quantile, interpolation)


def n_unique(name: str) -> Expr:
    return col(name).n_unique()


def cum_sum(name: str, *, reverse: bool = False) -> Expr:
    return col(name).cum_sum(reverse=reverse)


def cum_min(name: str, *, reverse: bool = False) -> Expr:
    return col(name).cum_min(reverse=reverse)


def cum_max(name: str, *, reverse: bool = False) -> Expr:
    return col(name).cum_max(reverse=reverse)


def cum_count(name: str, *, reverse: bool = False) -> Expr:
    return col(name).cum_count(reverse=reverse)


def rank(name: str, method: str = "average", *, descending: bool = False) -> Expr:
    return col(name).rank(method, descending=descending)


def shift(name: str, n: int = 1, *, fill_value: Any = None) -> Expr:
    return col(name).shift(n, fill_value=fill_value)


def diff(name: str, n: int = 1, null_behavior: str = "ignore") -> Expr:
    return col(name).diff(n, null_behavior)


def rolling_sum(name: str, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> Expr:
    return col(name).rolling_sum(window_size, weights, min_samples=min_samples, center=center)


def rolling_mean(name: str, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> Expr:
    return col(name).rolling_mean(window_size, weights, min_samples=min_samples, center=center)


def rolling_min(name: str, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> Expr:
    return col(name).rolling_min(window_size, weights, min_samples=min_samples, center=center)


def rolling_max(name: str, window_size: int, weights: Any = None, *, min_samples: Optional[int] = None, center: bool = False) -> Expr:
    return col(name).rolling_max(window_size, weights, min_samples=min_samples, center=center)


_EPOCH = _dt.date(1970, 1, 1)


def literal_physical(value: Any):
    """(python value, logical dtype or None for dynamic int/float) of a literal."""
    if value is None:
        return None, None
    if isinstance(value, (bool, np.bool_)):
        return bool(value), T.Boolean
    if isinstance(value, np.generic):
        return value.item(), T.NP_TO_DTYPE[value.dtype]
    if isinstance(value, _dt.datetime):
        delta = value - _dt.datetime(1970, 1, 1)
        return (delta.days * 86400 + delta.seconds) * 1_000_000 + delta.microseconds, T.Datetime
    if isinstance(value, _dt.date):
        return (value - _EPOCH).days, T.Date
    if isinstance(value, int):
        return value, "dyn_int"
    if isinstance(value, float):
        return value, "dyn_float"
    raise TypeError(f"unsupported literal {value!r}")
