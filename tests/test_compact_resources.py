"""CPU: what hipcc made of the compaction kernels (svs_amd/csrc/compact.h), read from the build's own resource report
(svs_amd/lib/build/, as tests/test_kernel_resources.py does): the six instantiations of compact_move_kernel -- plain,
with scales, with shadow; gathering from the corpus or reading the bounce buffer -- are all in the library, none uses
scratch memory or spills a register, and all keep the occupancy a copy kernel lives on."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLD = os.path.join(ROOT, "svs_amd", "lib", "build")
RES = os.path.join(BLD, "svs_amd.resources.txt")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(RES):
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    with open(RES) as f:
        return f.read()


def _kernels(txt):
    """{demangled kernel: {field: int}} for the compaction kernels."""
    blocks = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = block.split()[0]
        if "compact_move_kernel" in name:
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
        out[re.search(r"(compact_move_kernel<[^>]*>)", p).group(1)] = fields
    return out


def test_compaction_kernels_use_no_scratch(report):
    table = _kernels(report)
    want = {f"compact_move_kernel<{form}, {gather}>" for form in (0, 1, 2) for gather in ("true", "false")}
    assert set(table) == want, sorted(table)
    for k, r in table.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{k}: {r}"
        assert r["lds"] == 0 and r["agpr"] == 0, f"{k}: {r}"
        assert r["vgpr"] <= 128, f"{k}: {r} -- four waves per SIMD need <= 128 registers"
