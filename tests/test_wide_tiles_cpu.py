"""Wide tiles without a GPU: the launchers' choice between 512-row and 128-row tiles as a pure function (plx_wide_tiles_choice = csrc/kernels_fused.hip
wide_tiles_choice), and the registers of the new kernels -- read from the built library's code objects and, for a run-time compiled program, from the code objects
plx_jit_selftest leaves in PLX_JIT_DUMP_DIR (as tests/test_kernel_resources_cpu.py reads them).

The default grid is five workgroups of four waves per CU, five waves per SIMD: 512 / 5 = 102 registers, 96 after rounding down to the allocation granule of 8."""
import os
import re
import shutil
import subprocess

import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from tests.test_plan_compile_cpu import ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
BOOL, I8, I16, I32, I64, U8, U16, U32, U64, F32, F64 = range(11)      # plx_dtype
WIDTH = {I8: 1, U8: 1, I16: 2, U16: 2, I32: 4, U32: 4, F32: 4, I64: 8, U64: 8, F64: 8}
BASE = 1 << 20      # any address that is a multiple of 64


def choice(dtypes, compiled=True, knob=True, n_rows=1 << 20, nullable=None, values=None, validity=None):
    n = len(dtypes)
    return F.wide_tiles_choice(compiled, knob, n_rows, dtypes, nullable or [0] * n, values or [BASE * (i + 1) for i in range(n)], validity or [0] * n)


Q1_ROW = [U16, U8, U8, U8, U32, U8, U8]          # the encoded Q1 row with the decimal price: 11 bytes
Q1_ROW_F64 = [U16, U8, U8, U8, F64, U8, U8]      # ... with the price as stored: 15 bytes


def test_chosen_exactly_when_every_condition_holds():
    for row in (Q1_ROW, Q1_ROW_F64, [U8], [I16, I32], [I8] * 10):
        assert choice(row) == 1, row
        assert choice(row, compiled=False) == 0          # the interpreter has no wide form
        assert choice(row, knob=False) == 0              # PLX_WIDE_TILES=0
        for i in range(len(row)):
            nullable = [int(j == i) for j in range(len(row))]
            assert choice(row, nullable=nullable) == 0, (row, i)
            assert choice(row, validity=[BASE * 64 * nullable[j] for j in range(len(row))]) == 0, (row, i)      # a bitmap the shape does not announce
    # rows wider than 16 bytes; a bit-packed input; eight-byte columns alone (one 16-byte load per two rows already)
    assert choice([U16, U8, U8, U8, F64, F64]) == 0 and choice([U32] * 5) == 0
    assert choice([U8, BOOL]) == 0 and choice([I16, F32]) == 0      # (no fused program reads an f32 column, and the 128-row loads have no case for one)
    assert choice([I64]) == 0 and choice([F64, I64]) == 0 and choice([F64, I32]) == 1
    assert choice([]) == 0


def test_whole_tiles_only():
    assert choice(Q1_ROW, n_rows=511) == 0 and choice(Q1_ROW, n_rows=512) == 1 and choice(Q1_ROW, n_rows=0) == 0


def test_every_pointer_aligned_to_eight_rows_of_its_column():
    for row in (Q1_ROW, Q1_ROW_F64):
        for i, dt in enumerate(row):
            pack = 8 * WIDTH[dt]
            for off in range(WIDTH[dt], 64 + WIDTH[dt], WIDTH[dt]):      # every row offset of a slice up to 64 bytes
                values = [BASE * (j + 1) + (off if j == i else 0) for j in range(len(row))]
                assert choice(row, values=values) == int(off % pack == 0), (row, i, off)


def test_bad_arguments():
    assert F.lib().plx_wide_tiles_choice(1, 1, 1024, 11, None, None, None, None) == -1
    assert F.lib().plx_wide_tiles_choice(1, 1, 1024, 1, None, None, None, None) == -1


# ---- registers ------------------------------------------------------------------------------------------------------------------------------
def kernel_notes(obj, cwd):
    """{kernel symbol: {field: int}} from the AMDGPU metadata note of a code object"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], cwd=cwd, capture_output=True, text=True, timeout=300).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s*(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s*(\d+)", block)}
    return out


def assert_fits_five_waves(name, r):
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    assert r["vgpr_count"] <= 96, (name, r)


def test_ahead_of_time_wide_kernels_fit_five_waves_per_simd(tmp_path):
    lib = os.path.join(ROOT, "polars_amd", "libpolars_amd.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build)"
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    found = {}
    for f in sorted(f for f in os.listdir(tmp_path) if f.endswith("gfx950")):
        for name, r in kernel_notes(f, tmp_path).items():
            if "fused_scan_wide_kernel" in name:
                found[name] = r
    for shape in (15, 16):
        hit = [n for n in found if f"StatProgILi{shape}E" in n and "10LdsAggSinkE" in n]
        assert len(hit) == 1, (shape, sorted(found))
    for name, r in found.items():
        assert_fits_five_waves(name, r)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """the run-time compiled kernels of a narrow program with no ahead-of-time shape -- 8-byte rows, a predicate, a u8 key, sums, a max and a mean -- keyed and
    unkeyed, compiled once for this module: {file name: path} of the code objects and their sources"""
    d = tmp_path_factory.mktemp("jit")
    old = os.environ.get("PLX_JIT_DUMP_DIR")
    os.environ["PLX_JIT_DUMP_DIR"] = str(d)
    try:
        t = pl.DataFrame([ph("g", pl.UInt8, rng=(0, 5)), ph("a", pl.Int16), ph("b", pl.Int32), ph("c", pl.UInt8)])
        c = pl.col
        aggs = [c("b").sum().alias("sb"), c("c").max().alias("mc"), c("a").mean().alias("ma"), pl.len().alias("n")]
        t.lazy().filter(c("a") > 3).group_by("g").agg(*aggs).jit_selftest()
        t.lazy().filter(c("a") > 3).select(*aggs).jit_selftest()
    finally:
        if old is None:
            del os.environ["PLX_JIT_DUMP_DIR"]
        else:
            os.environ["PLX_JIT_DUMP_DIR"] = old
    return {f: os.path.join(d, f) for f in os.listdir(d)}


def test_run_time_compiled_wide_kernels_fit_five_waves_per_simd(dumped):
    objs = sorted(f for f in dumped if f.endswith(".hsaco"))
    for want in ("LdsAggSink_wide_", "RegAggSink_wide_"):
        assert any(f.startswith(want) for f in objs), (want, objs)
    checked = 0
    for f in objs:
        src = open(dumped[f[:-6] + ".hip"]).read()
        assert ("true>(dsh, args, sp)" in src) == ("_wide_" in f), f
        if "_wide_" not in f:
            continue
        for name, r in kernel_notes(os.path.basename(dumped[f]), os.path.dirname(dumped[f])).items():
            assert name.startswith("plx_jit_"), name
            assert_fits_five_waves(f + ":" + name, r)
            checked += 1
    assert checked == 2, (checked, objs)


def test_symbols_and_sources_of_the_forms_differ(dumped):
    """a code object cached for the 128-row form is never loaded for the wide one: the generated source -- the disk-cache key -- and the kernel symbol both differ"""
    forms = {}
    for f, path in dumped.items():
        if f.startswith(("LdsAggSink", "RegAggSink")) and f.endswith(".hip"):
            src = open(path).read()
            forms[f] = (re.search(r"#define plx_jit_kernel (\S+)", src).group(1), src)
    assert len(forms) == 4, sorted(forms)
    assert len({sym for sym, _ in forms.values()}) == 4 and len({src for _, src in forms.values()}) == 4
