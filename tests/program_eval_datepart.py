"""tests/program_eval.py extended by OP_DATEPART (fused.hpp: dst <- a date part of slot a, with the validity of a; Op::c = part | unit << 4, csrc/temporal.hpp).

program_eval.run_rows and the evaluators stacked on it stay as they are: this run_rows walks the program, hands every op it does not know to the next run_rows
down (tests/program_eval_dict.py, which knows OP_DICT and OP_SELECT) as one-op programs over their operand slots, and computes the part itself with the reference
of tests/dt_parts_ref.py -- the part's output dtype widened to the 64 bits of a slot, as the device does.  Installed over program_eval.run_rows (the `pe` fixture of
tests/test_dt_parts_cpu.py), evaluate / split_matches / evaluate_join then interpret programs that contain the op.
"""
import numpy as np

from tests import dt_parts_ref as R
from tests import program_eval as pe
from tests import program_eval_dict as ped
from tests import program_eval_select as pes

OP_DATEPART = 30
_base_run_rows = ped.run_rows


def run_rows(prog, cols, luts=None, split=False):
    n = len(next(iter(cols.values()))[0]) if cols else 0
    slots = {}
    for i in (pe.split_order(prog) if split else range(len(prog["ops"]))):
        op = prog["ops"][i]
        code, dst, a, b, c = op[:5]
        if code == OP_DATEPART:
            x, vx = slots[a]
            unit, name = R.UNITS[(c >> 4) & 3], R.PARTS[c & 15]
            v = x.view(np.int64)
            if unit == "date":
                v = v.astype(np.int32)                  # a Date slot is the sign extension of its 32 bits
            slots[dst] = (R.part(v, unit, name).astype(np.int64).view(np.uint64), vx.copy())
        elif code in (pe.OP_LOAD, pe.OP_CONST):
            one, _ = _base_run_rows({"ops": [op], "inputs": prog["inputs"], "pred": pe.NONE}, cols, luts)
            slots[dst] = one[dst]
        elif code == pes.OP_SELECT:
            sub = {"ops": [[pe.OP_LOAD, 0, 0, 0, 0, "0"], [pe.OP_LOAD, 1, 1, 0, 0, "0"], [pe.OP_LOAD, 2, 2, 0, 0, "0"], [code, 3, 0, 1, 2, op[5]]],
                   "inputs": [{"name": "a", "dtype": pe.U64}, {"name": "b", "dtype": pe.U64}, {"name": "c", "dtype": pe.U64}], "pred": pe.NONE}
            one, _ = _base_run_rows(sub, {"a": slots[a], "b": slots[b], "c": slots[c]}, luts)
            slots[dst] = one[3]
        else:
            sub = {"ops": [[pe.OP_LOAD, 0, 0, 0, 0, "0"], [pe.OP_LOAD, 1, 1, 0, 0, "0"], [code, 2, 0, 1, c, op[5]]],
                   "inputs": [{"name": "a", "dtype": pe.U64}, {"name": "b", "dtype": pe.U64}], "pred": pe.NONE}
            one, _ = _base_run_rows(sub, {"a": slots[a], "b": slots[b]}, luts)
            slots[dst] = one[2]
    if prog["pred"] == pe.NONE:
        return slots, np.ones(n, dtype=bool)
    pv, pm = slots[prog["pred"]]
    return slots, (pv & pe.U(1)).astype(bool) & pm
