"""tests/program_eval.py extended by OP_SELECT (fused.hpp; the op of when / then / otherwise), the one op with three source slots.

program_eval.run_rows restates every other opcode and stays as it is: this run_rows walks the program itself, hands every op but the select to that loop as a
one-op program over its operand slots (so the device semantics keep a single restatement), and executes the select as fused_device.hpp exec_op does:
t = predicate value bit & predicate validity bit, d = t ? a : b, vd = t ? va : vb.  Installed over program_eval.run_rows (the `pe` fixture of
tests/test_when_then_cpu.py), evaluate / split_matches / evaluate_join then interpret programs that contain the op.
"""
import numpy as np

from tests import program_eval as pe

OP_SELECT = 28
_base_run_rows = pe.run_rows


def run_rows(prog, cols, luts=None, split=False):
    n = len(next(iter(cols.values()))[0]) if cols else 0
    slots = {}
    for i in (pe.split_order(prog) if split else range(len(prog["ops"]))):
        op = prog["ops"][i]
        code, dst, a, b, c = op[:5]
        if code == OP_SELECT:
            (x, vx), (y, vy), (p, vp) = slots[a], slots[b], slots[c]
            t = (p & pe.U(1)).astype(bool) & vp
            slots[dst] = (np.where(t, x, y), np.where(t, vx, vy))
        elif code in (pe.OP_LOAD, pe.OP_CONST):
            one, _ = _base_run_rows({"ops": [op], "inputs": prog["inputs"], "pred": pe.NONE}, cols, luts)
            slots[dst] = one[dst]
        else:       # the operand slots as two u64 inputs of a one-op program
            sub = {"ops": [[pe.OP_LOAD, 0, 0, 0, 0, "0"], [pe.OP_LOAD, 1, 1, 0, 0, "0"], [code, 2, 0, 1, c, op[5]]],
                   "inputs": [{"name": "a", "dtype": pe.U64}, {"name": "b", "dtype": pe.U64}], "pred": pe.NONE}
            one, _ = _base_run_rows(sub, {"a": slots[a], "b": slots[b]}, luts)
            slots[dst] = one[2]
    if prog["pred"] == pe.NONE:
        return slots, np.ones(n, dtype=bool)
    pv, pm = slots[prog["pred"]]
    return slots, (pv & pe.U(1)).astype(bool) & pm
