"""tests/program_eval.py extended by OP_DICT (fused.hpp: dst <- dictionary c [slot a], with the validity of a), the op that turns the one-byte code of a
dictionary-encoded input back into its 64-bit pattern (csrc/encoded_inputs.hpp).

program_eval.run_rows restates every other opcode and stays as it is: this run_rows walks the program, hands the ops it knows to the next run_rows down (the one
of tests/program_eval_select.py, which knows OP_SELECT) as one-op programs over their operand slots, and does the lookup itself.  The dictionaries live in HBM, not
in the program dump: the caller puts them into the program as prog["dicts"] = [u64 array, ..], in the order of the encoded inputs.
"""
import numpy as np

from tests import program_eval as pe
from tests import program_eval_select as pes

OP_DICT = 29
_base_run_rows = pes.run_rows


def run_rows(prog, cols, luts=None, split=False):
    n = len(next(iter(cols.values()))[0]) if cols else 0
    slots = {}
    for i in (pe.split_order(prog) if split else range(len(prog["ops"]))):
        op = prog["ops"][i]
        code, dst, a, b, c = op[:5]
        if code == OP_DICT:
            x, vx = slots[a]
            slots[dst] = (np.asarray(prog["dicts"][c], dtype=np.uint64)[(x & pe.U(255)).astype(np.int64)], vx.copy())
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
