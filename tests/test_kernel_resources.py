"""CPU: what hipcc made of the LDS-DMA kernels (read from the build's own reports, svs_amd/lib/build/).

The phased GEMM (svs_amd/csrc/gemm_phased.h; the kernel of BASELINE.json configs[2] and configs[4],
i.e. a batch of the reference's np.dot, src/svs/kb.py:1623) keeps seven half-tiles of LDS-DMA in flight
behind counted `s_waitcnt vmcnt(N)`.  A spilled VGPR is reloaded with a scratch load followed by
`s_waitcnt vmcnt(0)`, which drains that ring: in round 2 the fp8 instantiation spilled three registers
and paid three drains per output tile.  These tests fail the build when that
comes back."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLD = os.path.join(ROOT, "svs_amd", "lib", "build")
RES = os.path.join(BLD, "svs_amd.resources.txt")
ISA = os.path.join(BLD, "svs_amd-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.fixture(scope="module")
def build_reports():
    if not (os.path.exists(RES) and os.path.exists(ISA)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    return RES, ISA


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def _resources(path):
    """{mangled kernel name: {field: int}} from -Rpass-analysis=kernel-resource-usage."""
    with open(path) as f:
        txt = f.read()
    table = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = block.split()[0]
        fields = {}
        for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, block)
            assert m, f"{name}: no '{key}' in the resource report"
            fields[key] = int(m.group(1))
        table[name] = fields
    return table


def test_no_fused_phased_kernel_uses_scratch(build_reports):
    table = _resources(build_reports[0])
    names = _demangle([n for n in table if "gemm_phased_kernel" in n])
    fused = {names[n]: table[n] for n in names if "gemm_phased_kernel<true" in names[n]}
    # f16 and fp8; 256- and 128-query tiles; default / nontemporal-corpus / A-B forms: all of them ship in the library
    assert len(fused) >= 10, sorted(fused)
    for want in ("<true, 1, 20, 256>", "<true, 2, 0, 256>", "<true, 1, 20, 128>", "<true, 2, 20, 128>"):
        assert any(want in k for k in fused), f"no gemm_phased_kernel{want} in the build"
    for k, r in fused.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{k}: {r} -- a spill reload drains the LDS-DMA ring"
        assert r["vgpr"] + r["agpr"] <= 256, f"{k}: {r} -- two waves per SIMD need <= 256 registers"
    plain = {names[n]: table[n] for n in names if "gemm_phased_kernel<false" in names[n]}
    for k, r in plain.items():
        assert r["scratch"] == 0, f"{k}: {r}"


def _function_body(isa_lines, mangled):
    start = next(i for i, l in enumerate(isa_lines) if l.startswith(mangled + ":"))
    end = next(i for i in range(start, len(isa_lines)) if isa_lines[i].startswith(".Lfunc_end"))
    return isa_lines[start:end]


def test_no_ring_drain_between_tile_loop_header_and_k_loop(build_reports):
    """Per output tile: side data staged, accumulators cleared, then the k loop.  Nothing in that
    stretch may wait for vmcnt(0) (the next tile's first half-tiles are already in flight), and the
    kernel may not touch scratch anywhere."""
    table = _resources(build_reports[0])
    names = _demangle([n for n in table if "gemm_phased_kernel" in n])
    with open(build_reports[1]) as f:
        isa = f.read().splitlines()
    checked = 0
    for mangled, pretty in names.items():
        if "gemm_phased_kernel<true" not in pretty:
            continue
        body = _function_body(isa, mangled)
        assert not [l for l in body if "scratch_" in l], f"{pretty}: scratch access"
        outer = next(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
        inner = next(i for i in range(outer, len(body)) if "Inner Loop Header: Depth=2" in body[i])
        assert inner - outer < 600, f"{pretty}: tile-loop header and k loop are {inner - outer} lines apart (layout changed?)"
        stretch = body[outer:inner]
        assert any("buffer_load_dword" in l and " lds" in l for l in stretch), f"{pretty}: the side-data LDS-DMA is not where it was"
        drains = [l.strip() for l in stretch if re.search(r"s_waitcnt.*vmcnt\(0\)", l)]
        assert not drains, f"{pretty}: {len(drains)} ring-draining waits before the k loop"
        # the k loop itself: counted waits only
        # (the loop's blocks are the ones hipcc annotates with its header -- they need not be contiguous, the latch sits ABOVE
        #  the header, and wave-uniform branches inside the loop, the flush of the previous tile's candidates has some, end nothing)
        hdr_line = next(i for i in range(inner, max(inner - 6, 0), -1) if re.match(r"\.LBB\d+_\d+:", body[i]))
        hdr = re.match(r"\.L(BB\d+_\d+):", body[hdr_line]).group(1)
        mfma, loop_drains, cur_in = [], [], False
        for i, l in enumerate(body):
            if re.match(r"\.LBB\d+_\d+:", l):
                j, head = i + 1, l
                while j < len(body) and re.match(r"\s+;", body[j]):
                    head += body[j]
                    j += 1
                cur_in = i == hdr_line or f"Header={hdr} Depth=2" in head
            if cur_in and "v_mfma" in l:
                mfma.append(l)
            if cur_in and re.search(r"s_waitcnt.*vmcnt\(0\)", l):
                loop_drains.append(l.strip())
        assert len(mfma) >= 32, f"{pretty}: {len(mfma)} MFMAs in what should be the k loop (two k-tiles: 32 at fp8 128-query tiles .. 128 at f16 256-query tiles)"
        if re.search(r"gemm_phased_kernel<true, [12], (0|20), ", pretty):   # the shipped forms: nothing in the loop drains the LDS-DMA ring
            assert not loop_drains, f"{pretty}: {len(loop_drains)} vmcnt(0) waits inside the k loop"
        checked += 1
    assert checked >= 10


def test_no_shipped_gemm_kernel_touches_scratch_inside_its_k_loop(build_reports):
    """Every GEMM kernel the library dispatches to (gemm_phased / gemm_tiled / gemm_q16r, all instantiations): no VGPR spill
    and no scratch access -- with ONE documented exception, gemm_tiled_kernel<256, true, 1, 256> (the fp8 256 x 256 tile with
    the fused epilogue: the fallback for rows with an odd number of 128-byte k-tiles, d = 384, 640, 1152 ...), whose 128
    accumulators + epilogue temporaries do not fit 256 registers: its spills must all sit in the EPILOGUE, after the k loop,
    where nothing is in flight that a scratch reload's vmcnt(0) could drain (the scratch gate only
    looked at gemm_phased_kernel)."""
    table = _resources(build_reports[0])
    gemm = [n for n in table if any(k in n for k in ("gemm_phased_kernel", "gemm_tiled_kernel", "gemm_q16r_kernel", "gemm_f32_q16_kernel"))]
    names = _demangle(gemm)
    assert len(names) >= 40, len(names)
    with open(build_reports[1]) as f:
        isa = f.read().splitlines()
    allowed = "gemm_tiled_kernel<256, true, 1, 256>"
    seen_allowed = False
    for mangled, pretty in names.items():
        r = table[mangled]
        if allowed in pretty:
            seen_allowed = True
            body = _function_body(isa, mangled)
            mfma = [i for i, l in enumerate(body) if "v_mfma" in l]
            scr = [i for i, l in enumerate(body) if "scratch_" in l]
            assert len(mfma) >= 32 and scr, (len(mfma), len(scr))
            # the k loop is the only place with MFMAs; the epilogue follows it in the layout
            assert min(scr) > max(mfma), f"{pretty}: scratch access at line {min(scr)} of the kernel, before its last MFMA ({max(mfma)})"
            continue
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{pretty}: {r}"
    assert seen_allowed


def _gemm_instantiations(table):
    """'gemm_tiled_kernel<32, true, 4, 128>', ...: every batched score kernel in the report, as c++filt spells it."""
    names = _demangle([n for n in table if re.search(r"gemm_(q16r|tiled|phased|f32_q16)_kernel", n)])
    out = set()
    for pretty in names.values():
        m = re.search(r"(gemm_\w+_kernel<[^>]*>)", pretty)
        assert m, pretty
        out.add(m.group(1))
    return out


def test_every_shipped_gemm_kernel_has_a_test_case(build_reports):
    """Every gemm_q16r / gemm_tiled / gemm_phased (and gemm_f32_q16) instantiation in the library is the main-pass kernel
    of some case of tests/batch_kernel_table.py (which tests/test_batch_kernels_gpu.py checks against f64 and asserts it
    reached), or on the table's list of kernels that only an A/B variant reaches.  A kernel added without a case fails
    here, on CPU."""
    from batch_kernel_table import AB_ONLY, CASES
    built = _gemm_instantiations(_resources(build_reports[0]))
    assert len(built) >= 48, sorted(built)
    tested = {c[6] for c in CASES}
    untested = sorted(built - tested - set(AB_ONLY))
    assert not untested, f"kernels in the build that no case of tests/batch_kernel_table.py reaches: {untested}"
    stale = sorted((tested | set(AB_ONLY)) - built - {"gemv"})
    assert not stale, f"kernels the table names that the build does not hold: {stale}"
    both = sorted(tested & set(AB_ONLY))
    assert not both, f"kernels both tested and listed as A/B-only: {both}"
    assert set(AB_ONLY.values()) <= {3, 4, 8, 9}


def _gemv_instantiations(table):
    """'gemv_unrolled_kernel<64, 2, 4, svs::DotF16>', ...: every single-query score kernel in the report."""
    names = _demangle([n for n in table if "gemv_" in n])
    out = set()
    for pretty in names.values():
        m = re.search(r"(gemv_\w+<[^>]*>)", pretty)
        assert m, pretty
        out.add(m.group(1))
    return out


def test_every_shipped_gemv_kernel_has_a_test_case(build_reports):
    """Every single-query score kernel in the library (gemv_*: one-shot, persistent, unrolled and loop kernels of the
    three dtypes) has a row in tests/single_kernel_table.py, which tests/test_single_kernels_gpu.py runs, asserting the
    kernel was reached -- or is on the table's short list of instantiations that no index can launch.  A kernel added
    without a case, or a row deleted from the table, fails here, on CPU."""
    from single_kernel_table import CASES, LONG_ROWS, NO_SHAPE
    built = _gemv_instantiations(_resources(build_reports[0]))
    assert len(built) >= 161, sorted(built)
    tested = {c[3] for c in CASES}
    assert len(tested) == len(CASES), "two rows of CASES name one kernel"
    untested = sorted(built - tested - set(NO_SHAPE))
    assert not untested, f"kernels in the build that tests/single_kernel_table.py has no row for: {untested}"
    stale = sorted((tested | set(NO_SHAPE)) - built)
    assert not stale, f"kernels the table names that the build does not hold: {stale}"
    assert not tested & set(NO_SHAPE)
    assert {c[3] for c in LONG_ROWS} <= tested
    assert {c[2] for c in CASES} == {0, 1, 2, 3, 4, 5}


def _geometry(chunks):
    """(T, NC) of for_row_geometry / for_width for a row of `chunks` 16-byte chunks (NC None: too long to unroll)."""
    if chunks <= 64:
        return next(t for t in (1, 2, 4, 8, 16, 32, 64) if t >= chunks), 1
    return 64, next((nc for nc in (2, 3, 4, 6, 8, 12, 16) if 64 * nc >= chunks), None)


def test_single_kernel_table_rows_have_the_row_length_their_kernel_takes():
    """Each row's d, through the padding rule, is a row length of its kernel's geometry (which kernel really runs is
    asserted on the GPU); and no f32 dimension gives a row that gemv_unrolled_kernel<64, 12 | 16, 1, svs::DotF32>
    would take -- the two instantiations the table lists as unreachable."""
    from single_kernel_table import CASES, FP8_HOT, LONG_ROWS, NO_SHAPE, PER16, choose_ld
    for dtype, d, variant, kernel in CASES + LONG_ROWS:
        ld = choose_ld(d, dtype)
        chunks, args = ld // PER16[dtype], kernel[kernel.index("<") + 1:-1].split(", ")
        assert ld % PER16[dtype] == 0 and ld >= d
        if "oneshot" in kernel or "rows_kernel" in kernel:
            assert ld == d, (dtype, d, ld)
            if dtype == "fp8":
                assert FP8_HOT[ld] == tuple(int(a) for a in args[:3]) and ld == int(args[0]) * 64 * int(args[1])
            else:
                assert chunks == 64 * int(args[0]) and chunks <= (1024 if dtype == "f32" else 512), (kernel, ld)
        else:
            exact = chunks % 64 == 0 and (chunks <= 1024 if dtype == "f32" else chunks <= 512 if dtype == "f16" else ld in FP8_HOT)
            assert not exact, f"{dtype} d={d}: ld {ld} is a one-shot kernel's"
            t, nc = _geometry(chunks)
            if kernel.startswith("gemv_unrolled_kernel"):
                assert variant == 0 and chunks <= 1024 and (t, nc) == (int(args[0]), int(args[1])), (kernel, d, ld)
            else:
                assert t == int(args[0]) and (variant == 4) == (chunks <= 1024), (kernel, d, ld)
    assert sorted(NO_SHAPE) == ["gemv_unrolled_kernel<64, 12, 1, svs::DotF32>", "gemv_unrolled_kernel<64, 16, 1, svs::DotF32>"]
    for d in range(1, 4097):      # (longer rows are more than 1024 chunks: not the unrolled kernel's)
        chunks = choose_ld(d, "f32") // 4
        assert chunks <= 512 or chunks % 64 == 0, f"f32 d={d}: {chunks} chunks would reach an unrolled kernel of 12 or 16 chunks per lane"


def _gather_instantiations(table):
    """'gather_scores_kernel<2, 64, 16, 1, 4>', ...: every filtered-search score kernel in the report."""
    names = _demangle([n for n in table if "gather_scores_kernel" in n])
    out = set()
    for pretty in names.values():
        m = re.search(r"(gather_scores_kernel<[^>]*>)", pretty)
        assert m, pretty
        out.add(m.group(1))
    return out


def test_every_shipped_gather_kernel_has_a_test_case(build_reports):
    """Every gather_scores_kernel instantiation in the library (14 row geometries x 3 dtypes x a lone query / a batch)
    is named by a row of tests/gather_kernel_table.py, which tests/test_gather_kernels_gpu.py runs, asserting the kernel
    was reached.  A geometry added to for_row_geometry without a row, or a row deleted from the table, fails here."""
    from gather_kernel_table import CASES
    built = _gather_instantiations(_resources(build_reports[0]))
    assert len(built) >= 84, sorted(built)
    tested = {k for c in CASES for k in c[3:5]}
    untested = sorted(built - tested)
    assert not untested, f"kernels in the build that tests/gather_kernel_table.py has no row for: {untested}"
    stale = sorted(tested - built)
    assert not stale, f"kernels the table names that the build does not hold: {stale}"


GATHER_U = {1: 8, 2: 6, 3: 4, 4: 3, 6: 2, 8: 2, 12: 1, 16: 1}      # gather_u, per chunks per lane


def test_gather_kernel_table_rows_have_the_row_length_their_kernels_take():
    """Each row's d, through the padding rule, is a row length of the geometry in its two kernel names; U and G follow
    gather_u and GATHER_G; and every geometry has a ragged and an exact row in all three dtypes."""
    from gather_kernel_table import CASES, DT, case_id, rows_per_block, rows_per_wave
    from single_kernel_table import PER16, choose_ld
    seen = {}
    for case in CASES:
        dtype, d, shape, k1, k4 = case
        ld = choose_ld(d, dtype)
        assert ld % PER16[dtype] == 0 and ld >= d
        chunks = ld // PER16[dtype]
        t, nc = _geometry(chunks)
        assert nc is not None, case
        assert k1 == f"gather_scores_kernel<{DT[dtype]}, {t}, {nc}, {GATHER_U[nc]}, 1>", (case, chunks)
        assert k4 == f"gather_scores_kernel<{DT[dtype]}, {t}, {nc}, {GATHER_U[nc]}, 4>", (case, chunks)
        for k in (k1, k4):
            assert rows_per_wave(k) == 64 // t * GATHER_U[nc] and rows_per_block(k) == rows_per_wave(k) * (8 if nc >= 12 else 16)
        if shape == "exact":       # no lane past the row, no padding
            assert d == ld == t * nc * PER16[dtype], case
        else:                      # the last chunk ends in one zero column
            assert shape == "ragged" and ld == d + 1, case
        assert (dtype, t, nc, shape) not in seen, f"{case_id(case)} and {case_id(seen[(dtype, t, nc, shape)])} are one case"
        seen[(dtype, t, nc, shape)] = case
    geometries = [(t, 1) for t in (1, 2, 4, 8, 16, 32, 64)] + [(64, nc) for nc in (2, 3, 4, 6, 8, 12, 16)]
    want = {(dtype, t, nc, shape) for dtype in ("f32", "f16", "fp8") for t, nc in geometries for shape in ("ragged", "exact")}
    assert set(seen) == want, sorted(want ^ set(seen))
    assert len({case_id(c) for c in CASES}) == len(CASES) == 84
    # the ragged rows leave lanes past the row for every geometry but T = 1 and 2
    assert sorted(t * nc - choose_ld(d, dtype) // PER16[dtype] for (dtype, t, nc, shape), (_, d, *_) in seen.items()
                  if shape == "ragged" and dtype == "f32") == [0, 0, 1, 2, 4, 8, 24, 24, 32, 32, 104, 120, 192, 192]


def test_no_gather_kernel_uses_scratch(build_reports):
    """Every gather_scores_kernel and gather_segments_kernel instantiation (3 dtypes x 14 row geometries x a lone query /
    a batch / the tile table: 126) holds its U x NC row chunks in registers: a spill would put scratch reloads between
    the row loads that keep the HBM busy and the dot loop (gather.h; fp8 pins each chunk's decode for this reason)."""
    table = _resources(build_reports[0])
    names = _demangle([n for n in table if "gather_scores_kernel" in n or "gather_segments_kernel" in n])
    assert len(names) >= 126, len(names)
    for mangled, pretty in names.items():
        r = table[mangled]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{pretty}: {r}"
