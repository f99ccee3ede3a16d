"""CPU: what hipcc made of the two kernels of the segmented filtered search (svs_amd/csrc/segments.h), read from the
build's own resource report (svs_amd/lib/build/, as tests/test_compact_resources.py does): every instantiation of
gather_segments_kernel<DT, T, NC, U> that tests/gather_kernel_table.py names and select_segments_kernel are in the
library, none uses scratch memory or spills a register, and each fits the registers its launch bounds leave a wave."""
import os
import re
import subprocess

import pytest

from gather_kernel_table import CASES, gather_wpb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "svs_amd", "lib", "build", "svs_amd.resources.txt")
FINAL_THREADS, SORT_CAP = 256, 4096
REGS_PER_SIMD = 512   # VGPRs + AGPRs per lane a SIMD has; a workgroup's waves spread over four SIMDs


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(RES):
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    with open(RES) as f:
        txt = f.read()
    blocks = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = block.split()[0]
        if "segments_kernel" in name:
            blocks[name] = block
    pretty = subprocess.run(["c++filt"], input="\n".join(blocks), capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for (name, block), p in zip(blocks.items(), pretty):
        fields = {}
        for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, block)
            assert m, f"{p}: no '{key}' in the resource report"
            fields[key] = int(m.group(1))
        out[re.search(r"((?:gather|select)_segments_kernel(?:<[^>]*>)?)", p).group(1)] = fields
    return out


def _segments_name(gather_name):
    """gather_scores_kernel<DT, T, NC, U, G> -> the segmented kernel of the same geometry."""
    args = gather_name[gather_name.index("<") + 1:-1].split(", ")
    return f"gather_segments_kernel<{', '.join(args[:4])}>"


def test_every_instantiation_is_in_the_library(table):
    want = {_segments_name(c[3]) for c in CASES} | {"select_segments_kernel"}
    assert len(want) == 3 * 14 + 1
    assert set(table) == want, sorted(set(table) ^ want)


def test_no_scratch_no_spills_registers_within_launch_bounds(table):
    for k, r in table.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{k}: {r}"
        if k.startswith("gather"):
            nc = int(k[k.index("<") + 1:-1].split(", ")[2])
            waves = gather_wpb(nc)
            assert r["lds"] == 0, f"{k}: {r}"
        else:
            waves = FINAL_THREADS // 64
            assert r["lds"] == 8 * SORT_CAP, f"{k}: {r}"
        per_simd = -(-waves // 4)
        assert r["vgpr"] + r["agpr"] <= REGS_PER_SIMD // per_simd, f"{k}: {r} -- {per_simd} waves of one workgroup share a SIMD"
