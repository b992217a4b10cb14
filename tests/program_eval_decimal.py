"""tests/program_eval.py extended by OP_DEC10 (fused.hpp: dst <- (double)(int64) slot a / 10^c, with the validity of a), the op that turns the integer of a
decimal-encoded input back into its f64 value (csrc/decimal.hpp div10: q = n * r, rem = fma(-q, d, n), q' = fma(rem, r, q) with d = 10^c and r = RN(1 / d)).

program_eval.run_rows and the evaluators stacked on it stay as they are: this run_rows walks the program, hands every op it does not know to the next run_rows
down (tests/program_eval_dict.py, which knows OP_DICT and OP_SELECT) as one-op programs over their operand slots, and computes the three steps itself.  numpy has
no fused multiply-add, so each one is done exactly in rationals and rounded once (fractions.Fraction -> float is correctly rounded): the same function, written
without the instruction.  The dictionaries of a program travel as prog["dicts"], as in program_eval_dict.
"""
from fractions import Fraction

import numpy as np

from tests import program_eval as pe
from tests import program_eval_dict as ped
from tests import program_eval_select as pes

OP_DEC10 = 31
_base_run_rows = ped.run_rows


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def div10(n, e):
    """n: integer-valued f64 array -> n / 10^e in the three-FMA form"""
    d = float(10**e)
    r = 1.0 / d
    out = np.empty(len(n), np.float64)
    for i, x in enumerate(n.tolist()):
        q = x * r
        out[i] = fma(fma(-q, d, x), r, q)
    return out


def run_rows(prog, cols, luts=None, split=False):
    n = len(next(iter(cols.values()))[0]) if cols else 0
    slots = {}
    for i in (pe.split_order(prog) if split else range(len(prog["ops"]))):
        op = prog["ops"][i]
        code, dst, a, b, c = op[:5]
        if code == OP_DEC10:
            x, vx = slots[a]
            slots[dst] = (div10(x.view(np.int64).astype(np.float64), c).view(np.uint64), vx.copy())
        elif code in (pe.OP_LOAD, pe.OP_CONST):
            one, _ = _base_run_rows({"ops": [op], "inputs": prog["inputs"], "pred": pe.NONE}, cols, luts)
            slots[dst] = one[dst]
        elif code == pes.OP_SELECT:
            sub = {"ops": [[pe.OP_LOAD, 0, 0, 0, 0, "0"], [pe.OP_LOAD, 1, 1, 0, 0, "0"], [pe.OP_LOAD, 2, 2, 0, 0, "0"], [code, 3, 0, 1, 2, op[5]]],
                   "inputs": [{"name": "a", "dtype": pe.U64}, {"name": "b", "dtype": pe.U64}, {"name": "c", "dtype": pe.U64}], "pred": pe.NONE}
            one, _ = _base_run_rows(sub, {"a": slots[a], "b": slots[b], "c": slots[c]}, luts)
            slots[dst] = one[3]
        else:
            sub = {"ops": [[pe.OP_LOAD, 0, 0, 0, 0, "0"], [pe.OP_LOAD, 1, 1, 0, 0, "0"], [code, 2, 0, 1, c, op[5]]], "dicts": prog.get("dicts"),
                   "inputs": [{"name": "a", "dtype": pe.U64}, {"name": "b", "dtype": pe.U64}], "pred": pe.NONE}
            one, _ = _base_run_rows(sub, {"a": slots[a], "b": slots[b]}, luts)
            slots[dst] = one[2]
    if prog["pred"] == pe.NONE:
        return slots, np.ones(n, dtype=bool)
    pv, pm = slots[prog["pred"]]
    return slots, (pv & pe.U(1)).astype(bool) & pm
