"""CPU: the arithmetic of tests/far_rows.py -- that the planted blocks of test_far_rows_gpu.py really sit on the offset
boundaries they are meant to test, in every unit a kernel may count in, and that filler rows can neither hide nor fake
an answer of the whole-corpus cases.  No GPU, no library."""
import numpy as np
import pytest

import far_rows as fr
from single_kernel_table import choose_ld

DTYPES = ("f32", "f16", "fp8")
# the widest tolerance the project holds any score kernel to (test_batch_kernels_gpu.TOL["fp8"]); restated here only
# because importing a GPU test module on a machine without the library is not this test's business
WIDEST_TOL = 1e-5


def test_rows_are_3072_bytes_and_unpadded_for_every_dtype():
    for dtype in DTYPES:
        d = fr.DIMS[dtype]
        assert d * fr.ELEM_BYTES[dtype] == fr.ROW_BYTES
        assert choose_ld(d, dtype) == d, (dtype, d)
    assert fr.LD16 * fr.CHUNK_BYTES == fr.ROW_BYTES
    assert all((1 << p) % fr.ROW_BYTES for p in fr.POWERS)          # no boundary falls between two rows


def test_size_of_the_index():
    n = fr.n_rows()
    assert n % 4 and n % 64 and n % 1024
    assert n == fr.spans()[-1].row_last + 1 + fr.TAIL
    assert 22_300_000 < n < 22_500_000
    assert (1 << 36) < n * fr.ROW_BYTES < (1 << 36) + (8 << 20)
    assert n < 2 ** 31                                              # (rows themselves stay 32-bit: keys.h packs a u32 row)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_block_holds_a_row_that_straddles_its_boundary(dtype):
    loc = fr.loc()
    assert loc.shape == (len(fr.POWERS) * fr.BLOCK,) and np.all(np.diff(loc) > 0)
    for s in fr.spans():
        mid = s.row_first + fr.MID
        assert loc[fr.block_of(s.p)][fr.MID] == mid
        first_byte, last_byte = mid * fr.ROW_BYTES, (mid + 1) * fr.ROW_BYTES - 1
        assert first_byte < (1 << s.p) <= last_byte, (dtype, s.p)
        # ... and in the dtype's elements: the boundary is an element offset inside that row, not at its first element
        eb = fr.ELEM_BYTES[dtype]
        assert first_byte // eb < (1 << s.p) // eb <= last_byte // eb
        # the block is centred: as many planted rows wholly below the boundary as wholly above it, give or take one
        below, above = mid - s.row_first, s.row_last - mid
        assert below == fr.MID and above == fr.BLOCK - fr.MID - 1 and abs(below - above) <= 1
        assert s.byte_first == s.row_first * fr.ROW_BYTES and s.byte_last < (1 << s.p) + (fr.BLOCK * fr.ROW_BYTES)
        assert s.byte_first < (1 << s.p) < s.byte_last


def test_block_36_is_where_a_32_bit_chunk_product_wraps():
    s = fr.spans()[-1]
    assert s.p == 36
    rows = np.arange(s.row_first, s.row_last + 1)
    wraps = rows * fr.LD16 >= 1 << 32
    assert not wraps[:fr.MID + 1].any() and wraps[fr.MID + 1:].all()     # the straddling row starts below, ends above
    assert (s.row_first + fr.MID) * fr.LD16 < (1 << 32) <= (s.row_first + fr.MID + 1) * fr.LD16 - 1
    assert s.chunk_first < (1 << 32) <= s.chunk_last
    # a narrowed product sends those rows to the FIRST rows of the buffer, which are filler: block 31 starts far above
    for r in rows[wraps]:
        w = fr.wrapped_row(int(r))
        assert 0 <= w < fr.BLOCK and w + 1 < fr.block_start(31)
    assert fr.filler_source(int(fr.wrapped_row(int(rows[-1])))) == int(fr.wrapped_row(int(rows[-1])))


def test_block_35_straddles_2_31_chunks():
    s = fr.spans()[-2]
    assert s.p == 35 and s.chunk_first < (1 << 31) <= s.chunk_last
    mid = s.row_first + fr.MID
    assert mid * fr.LD16 < (1 << 31) <= (mid + 1) * fr.LD16 - 1
    assert fr.wrapped_row(s.row_last, signed=True) < 0            # a signed product points below the buffer there
    assert fr.wrapped_row(s.row_first, signed=True) == s.row_first


@pytest.mark.parametrize("dtype,powers", [("f16", (32, 33)), ("f32", (33, 34))])
def test_element_offsets_2_31_and_2_32_fall_inside_planted_blocks(dtype, powers):
    eb = fr.ELEM_BYTES[dtype]
    by_p = {s.p: s for s in fr.spans()}
    for e, p in zip((31, 32), powers):
        s = by_p[p]
        assert s.byte_first // eb < (1 << e) <= s.byte_last // eb, (dtype, e, p)
        assert (1 << e) * eb == 1 << p


def test_fp8_byte_offsets_are_its_element_offsets():
    by_p = {s.p: s for s in fr.spans()}
    for e in (31, 32):
        assert by_p[e].byte_first < (1 << e) <= by_p[e].byte_last


def test_schedule_sums_to_n_and_keeps_every_block_whole_and_in_place():
    sched = fr.schedule()
    assert sum(a.count for a in sched) == fr.n_rows()
    at = 0
    for a in sched:
        assert a.row0 == at and a.count > 0
        at += a.count
        if a.kind == "fill":
            assert a.source == 0 and a.count <= fr.FILL_ROWS
    plants = [a for a in sched if a.kind == "plant"]
    assert [a.source for a in plants] == list(fr.POWERS)
    for a in plants:
        assert a.count == fr.BLOCK and a.row0 == fr.block_start(a.source)     # one append, at its position
    assert len(sched) < 100
    assert fr.FILL_ROWS * fr.ROW_BYTES <= 1 << 30 < (fr.FILL_ROWS + 1) * fr.ROW_BYTES


def test_boundary_fillers_are_filler_on_both_sides_of_every_block():
    rows = fr.boundary_fillers()
    planted = set(fr.loc().tolist())
    assert len(rows) == 4 * len(fr.POWERS) and not planted & set(rows.tolist())
    for s in fr.spans():
        assert np.any(rows < s.row_first) and np.any(rows > s.row_last)
        assert s.row_first - 1 in rows and s.row_last + 1 in rows
    for r in rows:
        assert 0 <= fr.filler_source(int(r)) < fr.FILL_ROWS
    with pytest.raises(ValueError):
        fr.filler_source(int(fr.loc()[0]))
    with pytest.raises(ValueError):
        fr.filler_source(fr.n_rows())


def test_the_shadowed_geometry():
    """The f32-only second layout (rows of 8 KiB, d = 2048): eligible for a half shadow, planted blocks around every
    boundary of the row buffer, and the SHADOW's own offsets pass 2^32 bytes, 2^31 halves and 2^31 chunks inside them."""
    lay = fr.SHADOWED
    d = lay.dims["f32"]
    assert d * 4 == lay.row_bytes and choose_ld(d, "f32") == d
    assert d % 512 == 0 and d <= 4096 and choose_ld(d, "f16") == d          # shadow_eligible (svs_amd.hip)
    n = lay.n_rows()
    assert n % 4 and n % 64 and n % 1024 and (1 << 36) < n * lay.row_bytes < (1 << 36) + (16 << 20)
    assert n * d * 2 > 1 << 35                                              # 32 GiB of halves, and a little
    by_p = {s.p: s for s in lay.spans()}
    for p, s in by_p.items():
        mid = s.row_first + fr.MID
        assert mid * lay.row_bytes == 1 << p                                # the middle row STARTS on the boundary
        assert s.byte_first < (1 << p) < s.byte_last and lay.loc()[fr.block_of(p)][fr.MID] == mid
    rows36 = np.arange(by_p[36].row_first, by_p[36].row_last + 1)
    wraps = rows36 * lay.ld16 >= 1 << 32
    assert not wraps[:fr.MID].any() and wraps[fr.MID:].all()
    for r in rows36[wraps]:
        assert 0 <= lay.wrapped_row(int(r)) < fr.BLOCK < lay.block_start(31)   # a narrowed product lands in filler
    assert lay.wrapped_row(by_p[35].row_last, signed=True) < 0
    for e, p in ((31, 33), (32, 34)):                                       # f32 element offsets
        assert by_p[p].byte_first // 4 < (1 << e) <= by_p[p].byte_last // 4
    # the shadow: row r lies at byte r * 2 d of it
    sh = lambda row: row * d * 2
    assert sh(by_p[33].row_first) < (1 << 32) <= sh(by_p[33].row_last)      # 2^32 shadow bytes = 2^31 halves
    assert sh(by_p[34].row_first) // 2 < (1 << 32) <= sh(by_p[34].row_last) // 2          # 2^32 halves
    assert sh(by_p[36].row_first) // 16 < (1 << 31) <= sh(by_p[36].row_last) // 16        # 2^31 shadow chunks
    sched = lay.schedule()
    assert sum(a.count for a in sched) == n and all(a.count <= lay.fill_rows for a in sched if a.kind == "fill")
    assert [(a.row0, a.count) for a in sched if a.kind == "plant"] == [(lay.block_start(p), fr.BLOCK) for p in fr.POWERS]
    assert lay.fill_rows * lay.row_bytes <= 1 << 30
    for r in lay.boundary_fillers():
        assert 0 <= lay.filler_source(int(r)) < lay.fill_rows


@pytest.mark.parametrize("case", list(fr.LAYOUTS))
def test_filler_can_neither_hide_nor_fake_an_answer(case):
    """On the f32 planted rows themselves (quantisation moves a score by far less than the margin asserted): every
    query's K-th best planted score, and so every score the whole-corpus cases ask for, is several times the filler
    bound plus the widest tolerance; and the threshold case's cut-off separates filler from what it must return."""
    dtype, lay = fr.LAYOUTS[case]
    d = lay.dims[dtype]
    rows, qs = fr.planted_rows(dtype, d), fr.queries(dtype, d=d)
    assert rows.shape == (len(fr.POWERS) * fr.BLOCK, d) and qs.shape == (fr.NQ, d)
    assert np.allclose(np.linalg.norm(rows.astype(np.float64), axis=1), 1.0, atol=1e-6)
    scores = rows.astype(np.float64) @ qs.astype(np.float64).T             # (2052, NQ)
    kth = np.sort(scores, axis=0)[-fr.K]
    print(f"{case}: smallest {fr.K}-th best planted score {kth.min():.4f}, filler bound {fr.FILL_BOUND:.5f}")
    assert fr.planted_only(kth, WIDEST_TOL)
    assert kth.min() > 2 * (fr.FILL_BOUND + WIDEST_TOL)                    # (a margin fp8 rounding, ~1e-3, cannot eat)
    assert not fr.planted_only([fr.FILL_BOUND], 0.0)
    # the cut-off: no filler row can reach it, and it admits a useful number of planted rows per query
    assert fr.ABOVE_CUT > 2 * fr.FILL_BOUND + WIDEST_TOL
    totals = (scores[:, :fr.ABOVE_QUERIES] >= fr.ABOVE_CUT).sum(axis=0)
    assert np.all(totals >= 50) and np.all(totals < len(rows)), totals
    # ... in every block, so that a block whose rows were misread would change the total
    for p in fr.POWERS:
        assert np.all((scores[fr.block_of(p), :fr.ABOVE_QUERIES] >= fr.ABOVE_CUT).sum(axis=0) >= 3), p
    assert fr.FILL_BOUND == pytest.approx(0.00882, abs=1e-5)
