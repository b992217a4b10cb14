"""Build-time guard for the wide-key join kernels (kernels_join_wide.hip): no scratch -- a per-lane array of key words indexed by a run-time loop, or a by-value array
of column descriptors copied to the stack, would put it there -- and at most 128 registers.  Compiled with -Rpass-analysis=kernel-resource-usage; no GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars_amd", "csrc")


def resource_usage(src):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-munsafe-fp-atomics",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900).stderr
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(": ", 1)[1]
            res[cur] = {}
        elif cur and ": " in t:
            k, v = t.split(": ", 1)
            res[cur][k.strip()] = v.strip()
    return res


def test_wide_join_kernels_use_no_scratch_and_at_most_128_registers():
    res = resource_usage("kernels_join_wide.hip")
    for part in ("join_wide_build_kernel", "join_wide_count_kernel", "join_wide_emit_kernel"):
        assert sum(part in name for name in res) == 1, (part, sorted(res))
    for name, r in res.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 128, (name, r)


def test_wide_join_is_listed_in_the_library_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        kernels = re.search(r"^KERNELS = (.*)$", f.read(), re.M).group(1).split()
    assert "kernels_join_wide" in kernels and "kernels_join" in kernels
