"""Shared cells of the LDS-table scans without a GPU (csrc/fused_cells.hpp, csrc/fused_sinks.hpp LdsCellSink; DESIGN.md 4.11 "Shared cells").

The plan function through plx_cell_plan: which aggregates share a cell, and where each of its two rules flips.  The packed word, the fold over 16 copies and the
unpacking as a stand-alone program under -fsanitize=address,undefined (tests/emu/shared_cells_main.cpp).  The row bound R against a walk over the tiles as the
kernel hands them out.  The compiled kernels: the two ahead-of-time ones from the built library's code objects, a run-time compiled one from the files
plx_jit_selftest leaves in PLX_JIT_DUMP_DIR."""
import os
import re
import shutil
import subprocess

import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests.test_plan_compile_cpu import ph
from tests.test_wide_tiles_cpu import LLVM, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F64 = 5, 10
OP_LOAD, OP_CONST, OP_ADD_I, OP_MUL_I, OP_I2F = 1, 2, 7, 9, 10
SUM_F, SUM_I, COUNT, LEN = 1, 2, 3, 5
SHAPE_Q1_ENCODED, SHAPE_Q1_ENCODED_PRICE = 15, 16


def test_pack_fold_and_unpack_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shared_cells_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "shared_cells_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


# ---- the plan function ---------------------------------------------------------------------------------------------------------------------
def bits(x):
    return int(x).bit_length()


def small(nullable=False, expression=False, count_other=False):
    """count, sum(q), sum(x), mean(q) -- q is input 0 (u8) decoded in place, x * stride + base; tests/emu/shared_cells_main.cpp small_shape"""
    ops = [(OP_LOAD, 0, 0, 0, 0), (OP_LOAD, 1, 1, 0, 0), (OP_LOAD, 4, 2, 0, 0), (OP_CONST, 5, 0, 0, 0), (OP_MUL_I, 0, 0, 5, 0), (OP_CONST, 5, 0, 0, 0),
           (OP_ADD_I, 0, 0, 4 if expression else 5, 0), (OP_I2F, 2, 0, 0, 0)]
    aggs = [(COUNT, 4) if count_other else (LEN, 0), (SUM_I, 0), (SUM_F, 1), (SUM_F, 2)]
    return dict(dtypes=[U8, F64, U8], nullable=[int(nullable), 0, 0], ops=ops, aggs=aggs)


def plan(shape, lo, hi, R, n, known=1):
    facts = [(known if kind == SUM_I else 0, lo, hi) for kind, _ in shape["aggs"]]
    return F.cell_plan(facts, R, n, **shape)


IDENTITY4 = (4, [0, 1, 2, 3], [-1, -1, -1, -1])


def test_q1_shares_one_cell_among_count_sum_and_mean():
    for sid in (SHAPE_Q1_ENCODED, SHAPE_Q1_ENCODED_PRICE):
        facts = [(0, 0, 0), (1, 1, 50)] + [(0, 0, 0)] * 5
        cells, shift, cell, frm = F.cell_plan(facts, 470_000, 600_000_000, static_shape_id=sid)
        assert cells == 5 and shift == bits(470_000 * 50)
        assert frm == [1, -1, -1, -1, -1, 1, -1] and cell == [0, 0, 1, 2, 3, 0, 4]
        # nothing known about the quantity, or a range that reaches below zero: every aggregate keeps its cell
        for f1 in ((0, 1, 50), (1, -1, 50)):
            cells, _, cell, frm = F.cell_plan([facts[0], f1] + facts[2:], 470_000, 600_000_000, static_shape_id=sid)
            assert (cells, cell, frm) == (7, list(range(7)), [-1] * 7), f1


def test_identity_cases():
    assert plan(small(), 0, 255, 1000, 1000) == (2, bits(1000 * 255), [0, 0, 1, 0], [1, -1, -1, 1])
    for what, shape, lo in (("nullable", small(nullable=True), 0), ("negative lower bound", small(), -1), ("expression", small(expression=True), 0),
                            ("count of another column", small(count_other=True), 0)):
        cells, _, cell, frm = plan(shape, lo, 255, 1000, 1000)
        assert (cells, cell, frm) == IDENTITY4, what
    assert plan(small(), 0, 255, 1000, 1000, known=0)[0] == 4


def test_rule_a_flips_between_64_and_65_bits():
    R = (1 << 24) - 1
    hi64, hi65 = ((1 << 40) - 1) // R, (1 << 40) // R + 1
    assert bits(R) + bits(R * hi64) == 64 and bits(R) + bits(R * hi65) == 65
    cells, shift, cell, frm = plan(small(), 0, hi64, R, 1)
    assert (cells, shift, frm) == (2, 40, [1, -1, -1, 1])
    p65 = plan(small(), 0, hi65, R, 1)
    assert (p65[0], p65[2], p65[3]) == IDENTITY4      # (rule B goes with it: it reads the packed cell only)
    for R, hi, packs in (((1 << 32) - 1, 1, True), (1 << 32, 1, False), ((1 << 64) - 1, 0, True), (3, (1 << 63) - 1, False)):
        assert (plan(small(), 0, hi, R, 1)[0] == 2) == packs, (R, hi)


def test_rule_b_flips_between_2_53_less_one_and_2_53():
    n, hi = 6361 * 69431, 20394401
    assert n * hi == (1 << 53) - 1
    assert plan(small(), 0, hi, 1000, n)[3] == [1, -1, -1, 1]
    assert plan(small(), 0, 1 << 27, 1000, 1 << 26)[0::3] == (3, [1, -1, -1, -1])      # 2^53: the mean keeps its cell, the count still shares
    assert plan(small(), 0, hi, 1000, n + 1)[3] == [1, -1, -1, -1]
    assert plan(small(), 0, hi + 1, 1000, n)[3] == [1, -1, -1, -1]


def test_bad_arguments():
    assert F.lib().plx_cell_plan(-1, 11, None, None, 0, None, 0, None, None, None, None, 1, 1, None) == -1
    assert F.lib().plx_cell_plan(999, 0, None, None, 0, None, 0, None, None, None, None, 1, 1, None) == -1


# ---- R ---------------------------------------------------------------------------------------------------------------------------------------
def rows_per_workgroup(n, grid, wide):
    """the rows every workgroup adds to its table, walking the tiles as fused_scan_body hands them out: wave w takes tiles w, w + waves, ..."""
    waves = grid * 4
    per_wave = [0] * waves
    nwide = n // 512 if wide else 0
    for w in range(waves):
        per_wave[w] += 512 * len(range(w, nwide, waves))
    first = nwide * 4
    ntiles = (n + 127) // 128
    for w in range(waves):
        for t in range(first + w, ntiles, waves):
            per_wave[w] += min(128, n - t * 128)
    return max(sum(per_wave[4 * g:4 * g + 4]) for g in range(grid))


@pytest.mark.parametrize("wide", [False, True])
def test_row_bound_holds_for_both_tile_sizes_and_the_tail(wide):
    for grid in (1, 2, 3, 7, 1280):
        for n in (1, 127, 128, 511, 512, 513, 1025, 4 * 512 * grid, 4 * 512 * grid + 1, 4 * 512 * grid + 511, 5 * 4 * 512 * grid + 385, 1_000_003):
            bound = F.lib().plx_lds_wg_rows(n, grid, int(wide))
            assert rows_per_workgroup(n, grid, wide) <= bound <= n, (n, grid, wide, bound)
    # the benchmark's scan: 6.0e8 rows over 1280 workgroups, as the issue states it
    assert F.lib().plx_lds_wg_rows(600_000_000, 1280, 1) <= 470_000


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------------------
def disassembly(obj, cwd):
    """{kernel symbol: [instruction mnemonics]} of a code object"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], cwd=cwd, capture_output=True, text=True, timeout=600).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(re.sub(r"_(e32|e64|dpp|sdwa)$", "", line.split()[0]))      # the mnemonic without its encoding suffix
    return out


def test_ahead_of_time_kernels_drop_two_atomics_and_the_conversion_per_row(tmp_path):
    """Every row pass of the plain kernel (8 in the wide loop, 2 in the 128-row tail) issues two ds_add_u64, five ds_add_f64 and the i64 -> f64 conversion of the
    quantity (v_cvt_f64_i32, v_ldexp_f64, v_cvt_f64_u32, v_add_f64); with shared cells one ds_add_u64, four ds_add_f64 and no conversion -- the conversion is left
    once, in finish, for each of its two output forms."""
    lib = os.path.join(ROOT, "polars_amd", "libpolars_amd.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build)"
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    notes, code = {}, {}
    for f in sorted(f for f in os.listdir(tmp_path) if f.endswith("gfx950")):
        found = {n: r for n, r in kernel_notes(f, tmp_path).items() if "fused_scan" in n and ("StatProgILi15E" in n or "StatProgILi16E" in n)}
        if found:
            notes.update(found)
            code.update({n: c for n, c in disassembly(f, tmp_path).items() if n in found})
    passes = 10
    for shape in (15, 16):
        for form in ("fused_scan_wide_kernel", "fused_scan_kernel"):
            plain = [n for n in code if f"{form}INS0_8StatProgILi{shape}E" in n and "10LdsAggSinkE" in n]
            shared = [n for n in code if f"{form}INS0_8StatProgILi{shape}E" in n and "11LdsCellSinkI" in n]
            assert len(plain) == 1 and len(shared) == 1, (shape, form, sorted(code))
            p, s = code[plain[0]], code[shared[0]]
            rows = passes if "wide" in form else 2
            assert p.count("ds_add_u64") == 2 * rows and s.count("ds_add_u64") == rows, (shape, form)
            assert p.count("ds_add_f64") == 5 * rows and s.count("ds_add_f64") == 4 * rows, (shape, form)
            for op in ("v_cvt_f64_i32", "v_ldexp_f64"):
                assert p.count(op) == rows and s.count(op) == 2, (shape, form, op, p.count(op), s.count(op))
            r = notes[shared[0]]
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["vgpr_count"] <= notes[plain[0]]["vgpr_count"], (shape, form, r)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cells")
    old = os.environ.get("PLX_JIT_DUMP_DIR")
    os.environ["PLX_JIT_DUMP_DIR"] = str(d)
    try:
        t = pl.DataFrame([ph("g", pl.UInt8, rng=(0, 5)), ph("a", pl.Int16), ph("c", pl.UInt8)])
        c = pl.col
        t.lazy().filter(c("a") > 3).group_by("g").agg(c("c").sum().alias("sc"), c("c").mean().alias("mc"), c("a").max().alias("xa"), pl.len().alias("n")).jit_selftest()
    finally:
        if old is None:
            del os.environ["PLX_JIT_DUMP_DIR"]
        else:
            os.environ["PLX_JIT_DUMP_DIR"] = old
    return str(d)


def test_run_time_compiled_kernels_carry_the_plan_in_source_and_symbol(dumped):
    """the plan is a template argument of the sink in the generated source -- the disk-cache key -- and part of the kernel symbol: an entry the plain sink left in a
    cache (this version's or an earlier one's) is never loaded for it"""
    sub = os.path.join(dumped, "shared_cells")
    files = sorted(os.listdir(sub))
    assert [f for f in files if f.endswith(".hip")] == sorted(f[:-6] + ".hip" for f in files if f.endswith(".hsaco")) and len(files) == 4, files
    plain = {f: open(os.path.join(dumped, f)).read() for f in os.listdir(dumped) if f.startswith("LdsAggSink") and f.endswith(".hip")}
    assert len(plain) == 2, sorted(plain)
    symbols = {re.search(r"#define plx_jit_kernel (\S+)", src).group(1) for src in plain.values()}
    for f in files:
        if not f.endswith(".hip"):
            continue
        src = open(os.path.join(sub, f)).read()
        m = re.search(r"fused_scan_body<JitProg, LdsCellSink<JitProg, (\d+)u>(, true)?>\(dsh, args, sp\)", src)
        assert m and (m.group(2) is not None) == ("_wide_" in f), f
        code = int(m.group(1))
        assert code & 0xffff != 0xffff and code >> 16, code      # a packed cell and a derived one
        sym = re.search(r"#define plx_jit_kernel (\S+)", src).group(1)
        assert sym.startswith("plx_jit_LdsCellSink_") and sym not in symbols
        symbols.add(sym)
        assert src not in plain.values()
    assert len(symbols) == 4
    for f in files:
        if f.endswith(".hsaco"):
            for name, r in kernel_notes(f, sub).items():
                assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["vgpr_count"] <= 96, (f, name, r)
            ops = [op for body in disassembly(f, sub).values() for op in body]
            assert "ds_add_u64" in ops and ops.count("v_ldexp_f64") <= 2, f      # the mean's conversion is left in finish only
