"""tests/program_eval.py extended by the two finalisation kinds of var / std (fused.hpp FIN_VAR / FIN_STD; csrc/variance.hpp from_shifted + finalize).

program_eval and the evaluators stacked on it stay as they are.  The lowering of var / std adds no opcode and no aggregate kind (OP_CONST, OP_SUB_F, OP_MUL_F and
three ordinary cells: sum(d), sum(d * d), count), so every run_rows / _cells below already interprets the program; only the last step is new.  evaluate() here
hands program_eval.evaluate a copy of the program in which each var / std final is replaced by plain copies of its three cells, and finishes those itself, in the
operation order of the device code.  contract_bound() is the accuracy contract of DESIGN.md 4.14 as a function of the data.
"""
import copy

import numpy as np

from tests import program_eval as pe

FIN_VAR, FIN_STD = 6, 7
EPS = 2.0 ** -53


def from_shifted(n, s1, s2):
    with np.errstate(all="ignore"):
        m2 = s2 - s1 * (s1 / n)
        m2 = np.where(m2 < 0.0, 0.0, m2)
    return np.where(n > 0, m2, 0.0)


def finalize(n, m2, ddof, want_std):
    """-> (values, valid): null when n <= ddof; NaN / inf -> NaN; a negative quotient is 0."""
    valid = n > ddof
    with np.errstate(all="ignore"):
        v = m2 / np.where(valid, n - ddof, 1.0)
        v = np.where(np.isfinite(v), np.maximum(v, 0.0), np.nan)
        if want_std:
            v = np.sqrt(v)
    return np.where(valid, v, 0.0), valid


def evaluate(prog, cols, luts=None):
    """program_eval.evaluate for programs whose finals may be FIN_VAR / FIN_STD."""
    p = copy.deepcopy(prog)
    pending = {}
    for o in prog["outputs"]:
        j = o["final"]
        if j < 0 or prog["finals"][j]["kind"] not in (FIN_VAR, FIN_STD):
            continue
        fs = prog["finals"][j]
        names = []
        for cell, dt in ((fs["a"], pe.F64), (fs["c"], pe.F64), (fs["b"], pe.U64)):
            p["finals"].append({"kind": pe.FIN_COPY64, "a": cell, "b": pe.NONE, "c": pe.NONE, "out_dtype": dt})
            names.append(f"__var{len(p['finals'])}")
            p["outputs"].append({"name": names[-1], "final": len(p["finals"]) - 1})
        pending[o["name"]] = (fs, names)
    p["outputs"] = [o for o in p["outputs"] if o["name"] not in pending]
    with np.errstate(invalid="ignore", over="ignore"):      # (inf - inf inside the sums of a group that holds an infinity: the NaN is the expected result)
        res = pe.evaluate(p, cols, luts)
    for name, (fs, (na, nc, nb)) in pending.items():
        s1, s2, n = res.pop(na)[0], res.pop(nc)[0], res.pop(nb)[0].astype(np.float64)
        v, valid = finalize(n, from_shifted(n, s1, s2), fs["ddof"], fs["kind"] == FIN_STD)
        res[name] = (v.astype(np.float32) if fs["out_dtype"] == pe.F32 else v, valid)
    # the order of the query's outputs
    order = list(res)
    want = [part["name"] for part in prog.get("key_plan", {}).get("parts", [])] + [o["name"] for o in prog["outputs"]]
    return {k: res[k] for k in want if k in res} | {k: res[k] for k in order if k not in want}


def contract_bound(x, ddof, D):
    """8 n eps (sigma^2 + D^2) n / (n - ddof) for the valid values x of one group (float64), sigma^2 = their population variance; D = max - min of the source over
    the whole frame (max |x| when the pivot is 0)."""
    n = len(x)
    if n <= ddof:
        return 0.0
    return 8.0 * n * EPS * (float(np.var(x)) + D * D) * n / (n - ddof)


def within_contract(got, x, ddof, D, want_std=False, f32=False):
    """Is `got` the var (std) of the float64 values x within the contract?  Reference = numpy's two-pass np.var; std is checked through its square with twice the
    bound; a Float32 output adds one 2^-24 relative rounding."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) <= ddof:
        return got is None
    if got is None:
        return False
    ref = float(np.var(x, ddof=ddof))
    if not np.isfinite(ref):
        return got != got
    bound = contract_bound(x, ddof, D) * (2.0 if want_std else 1.0)
    g = float(got) ** 2 if want_std else float(got)
    if f32:
        bound += (2.0 if want_std else 1.0) * 2.0 ** -24 * abs(ref) * 1.0000001 + 1e-45
    return abs(g - ref) <= bound
