"""The tail of the LDS-table group-by without a GPU (csrc/groupby_tail.hpp, kernels_fused.hip groupby_tail_kernel; DESIGN.md 4.11 "One tail kernel").

The layout of the result block and the rank computation as a stand-alone program under -fsanitize=address,undefined (tests/emu/groupby_tail_main.cpp); the compiled
kernel's resources from the built library's code objects; the switch and the reporters through the C ABI."""
import os
import shutil
import subprocess

from polars_amd import _ffi as F
from tests.test_wide_tiles_cpu import LLVM, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_and_ranks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "groupby_tail_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "groupby_tail_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_tail_kernel_uses_no_scratch(tmp_path):
    """one workgroup, everything it indexes dynamically in LDS (the layout, the ranks, the slot list): no private segment, no spills"""
    lib = os.path.join(ROOT, "polars_amd", "libpolars_amd.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build)"
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    found = {}
    for f in sorted(f for f in os.listdir(tmp_path) if f.endswith("gfx950")):
        found.update({n: r for n, r in kernel_notes(f, tmp_path).items() if "groupby_tail_kernel" in n})
    assert len(found) == 1, sorted(found)
    r = next(iter(found.values()))
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r


def test_switch_and_reporters_are_exported():
    before = (F.last_groupby_tail(), F.last_download_mirrored())
    assert before[0] in (0, 1) and before[1] in (0, 1)
    F.set_groupby_tail(False)
    F.set_groupby_tail(True)      # (the default)
    assert (F.last_groupby_tail(), F.last_download_mirrored()) == before      # the reporters speak of queries and downloads, not of the switch
