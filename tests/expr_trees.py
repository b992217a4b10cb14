"""Random typed expression trees with their own numpy evaluation, shared by tests/test_program_eval_cpu.py (the compiled program through the numpy
interpreter) and tests/test_gpu_program_ops.py (the same queries on the device).  Importable without a GPU."""
import numpy as np

import polars_amd as pl

N_ROWS = 4000


class Gen:
    """Random typed expression trees over four columns; every node carries its mirror-API expression and a numpy
    evaluation (values, valid) that follows the reference's rules: nulls propagate through arithmetic and comparisons,
    and / or are Kleene, integer + - * wrap, / is float division (col / literal = col * (1 / literal)), // and % follow
    Python sign rules with divisor 0 -> null."""

    def __init__(self, rng, cols):
        self.rng, self.cols = rng, cols

    def leaf(self, ty):
        r = self.rng
        if ty == "i":
            if r.random() < 0.7:
                name = ["a", "b"][int(r.integers(0, 2))]
                v, m = self.cols[name]
                return pl.col(name), (v, np.ones(len(v), bool) if m is None else m)
            k = int(r.integers(-7, 8))
            return pl.lit(k, dtype=pl.Int64), (np.full(self.n, k, np.int64), np.ones(self.n, bool))
        if r.random() < 0.7:
            name = ["x", "y"][int(r.integers(0, 2))]
            v, m = self.cols[name]
            return pl.col(name), (v, np.ones(len(v), bool) if m is None else m)
        k = float(r.integers(-6, 7)) / 2 + 0.25
        return pl.lit(k, dtype=pl.Float64), (np.full(self.n, k, np.float64), np.ones(self.n, bool))

    @property
    def n(self):
        return len(self.cols["a"][0])

    def num(self, ty, depth):
        r = self.rng
        if depth == 0 or r.random() < 0.25:
            return self.leaf(ty)
        with np.errstate(all="ignore"):
            if ty == "f" and r.random() < 0.2:          # int -> float through true division
                (ea, (va, ma)), (eb, (vb, mb)) = self.num("i", depth - 1), self.num("i", depth - 1)
                return ea / eb, (va.astype(np.float64) / vb.astype(np.float64), ma & mb)
            (ea, (va, ma)), (eb, (vb, mb)) = self.num(ty, depth - 1), self.num(ty, depth - 1)
            op = int(r.integers(0, 5 if ty == "i" else 4))
            if op == 0: return ea + eb, (va + vb, ma & mb)
            if op == 1: return ea - eb, (va - vb, ma & mb)
            if op == 2: return ea * eb, (va * vb, ma & mb)
            if ty == "f":
                return ea / eb, (va / vb, ma & mb)
            nz = vb != 0
            vs = np.where(nz, vb, 1)
            if op == 3: return ea // eb, (np.floor_divide(va, vs), ma & mb & nz)
            return ea % eb, (np.mod(va, vs), ma & mb & nz)

    def boolean(self, depth):
        r = self.rng
        if depth == 0 or r.random() < 0.35:
            ty = "i" if r.random() < 0.5 else "f"
            (ea, (va, ma)), (eb, (vb, mb)) = self.num(ty, 1), self.num(ty, 1)
            op = int(r.integers(0, 6))
            if ty == "f":      # total order: NaN == NaN, NaN greatest
                an, bn = np.isnan(va), np.isnan(vb)
                eq = (an & bn) | (va == vb)
                lt = ~an & (bn | (va < vb)) & ~eq
            else:
                eq, lt = va == vb, va < vb
            val = [eq, ~eq, lt, lt | eq, ~(lt | eq), ~lt][op]
            e = [ea == eb, ea != eb, ea < eb, ea <= eb, ea > eb, ea >= eb][op]
            return e, (val, ma & mb)
        if r.random() < 0.2:
            e, (v, m) = self.boolean(depth - 1)
            return ~e, (~v, m)
        (ea, (va, ma)), (eb, (vb, mb)) = self.boolean(depth - 1), self.boolean(depth - 1)
        if r.random() < 0.5:
            return ea & eb, (va & vb, (~va & ma) | (~vb & mb) | (ma & mb))
        return ea | eb, (va | vb, (va & ma) | (vb & mb) | (ma & mb))


def tree_case(seed, n=N_ROWS):
    """The columns and the three trees of one seed: cols {name: (values, valid or None)}, then (expression, (values, valid)) of the predicate, the float tree and
    the integer tree.  The draws come in this order from one generator, so a seed means the same query wherever it is built."""
    rng = np.random.default_rng(9000 + seed)
    cols = {"a": (rng.integers(-40, 40, n).astype(np.int64), rng.random(n) < 0.85), "b": (rng.integers(-4, 5, n).astype(np.int64), None),
            "x": (np.round(rng.normal(size=n) * 8) / 4, rng.random(n) < 0.9), "y": (rng.integers(-3, 4, n).astype(np.float64) / 2, None)}
    g = Gen(rng, cols)
    pred = g.boolean(3)
    ftree = g.num("f", 3)
    itree = g.num("i", 3)
    return cols, pred, ftree, itree


def tree_query(lf, pred, ftree, itree):
    """filter(pred).select(n, fs, fc, fmin, isum, imax, imean) over a LazyFrame that has the columns of tree_case."""
    pe_, fe, ie = pred[0], ftree[0], itree[0]
    return lf.filter(pe_).select(pl.len().alias("n"), fe.sum().alias("fs"), fe.count().alias("fc"), fe.min().alias("fmin"),
                                 ie.sum().alias("isum"), ie.max().alias("imax"), ie.mean().alias("imean"))
