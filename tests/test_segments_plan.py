"""CPU: the tile plan of the segmented filtered search (svs_amd/csrc/segments.h, through svs_internal_segments_plan).

A wave of gather_segments_kernel takes one tile: rows list[off .. off + rows) of ONE segment against one query, its scores
at the same offsets.  The plan is checked against a restatement in Python for every W = (64 / T) U of
tests/gather_kernel_table.py and on its properties: tiles never span segments, offsets are contiguous, the tiles' rows
add up to the segments', and the query index is carried.  The 2^31-row limit of one call is checked here too: no GPU
test can reach it."""
import numpy as np
import pytest

from gather_kernel_table import CASES, rows_per_wave

from svs_amd import _native

SORT_CAP = 4096
WS = sorted({rows_per_wave(c[3]) for c in CASES})


def plan(sizes, seg_query, w, cap=None):
    lib = _native.load()
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    sq = None if seg_query is None else np.ascontiguousarray(seg_query, dtype=np.int32)
    sqp = None if sq is None else sq.ctypes.data
    total = np.zeros(1, dtype=np.int64)
    off = np.full(len(sizes), -7, dtype=np.int64)
    nt = int(lib.svs_internal_segments_plan(sizes.ctypes.data, sqp, len(sizes), w, None, 0, off.ctypes.data,
                                            total.ctypes.data_as(_native.C.POINTER(_native.C.c_int64))))
    assert nt >= 0, _native.last_error()
    cap = nt if cap is None else cap
    tiles = np.full((max(cap, nt, 1), 4), -7, dtype=np.int64)
    assert int(lib.svs_internal_segments_plan(sizes.ctypes.data, sqp, len(sizes), w, tiles.ctypes.data, cap, None, None)) == nt
    return tiles[:nt], off, int(total[0])


def restated(sizes, seg_query, w):
    """The plan in ten lines: (offset, rows, query, segment) per tile, a segment's list offset or -1."""
    tiles, offs, off = [], [], 0
    for s, m in enumerate(sizes):
        small = 1 <= m <= SORT_CAP
        offs.append(off if small else -1)
        if small:
            q = s if seg_query is None else seg_query[s]
            tiles += [(off + p, min(w, m - p), q, s) for p in range(0, m, w)]
            off += m
    return tiles, offs, off


def test_the_table_has_every_wave_width():
    assert WS == [1, 2, 3, 4, 6, 8, 16, 32, 64, 128, 256, 512]


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("with_query", [False, True])
def test_plan_equals_restatement_and_its_properties(w, with_query):
    core = [1, w - 1, w, w + 1, 0, 2 * w + 1, 3]
    layouts = [core, [0] + core + [0], [0, 0] + core + [0, 0], core[::-1], [0, 0, 0], []]
    for sizes in layouts:
        rng = np.random.default_rng(w * 100 + len(sizes))
        nq = 3
        sq = rng.integers(0, nq, len(sizes)).tolist() if with_query else None
        tiles, off, total = plan(sizes, sq, w)
        want_tiles, want_off, want_total = restated(sizes, sq, w)
        assert tiles.tolist() == [list(t) for t in want_tiles], (w, sizes)
        assert off.tolist() == want_off and total == want_total == sum(sizes)
        # properties, stated on their own
        assert len(tiles) == sum(-(-m // w) for m in sizes)
        pos = 0
        for o, r, q, s in tiles.tolist():
            assert o == pos and 1 <= r <= w, (w, sizes, o, pos)             # contiguous, never empty, never wider than a wave
            assert off[s] <= o and o + r <= off[s] + sizes[s], (w, sizes)    # inside its segment
            assert q == (s if sq is None else sq[s])
            pos = o + r
        assert pos == sum(sizes)
        for s, m in enumerate(sizes):
            assert int(tiles[tiles[:, 3] == s, 1].sum()) == m


def test_large_segments_get_no_tiles():
    sizes = [5, SORT_CAP + 1, SORT_CAP, 10 ** 6, 2]
    tiles, off, total = plan(sizes, None, 24)
    assert off.tolist() == [0, -1, 5, -1, 5 + SORT_CAP] and total == 5 + SORT_CAP + 2
    assert sorted(set(tiles[:, 3].tolist())) == [0, 2, 4]
    assert tiles.tolist() == [list(t) for t in restated(sizes, None, 24)[0]]


def test_plan_written_up_to_cap_only():
    tiles, _, _ = plan([10, 10], None, 4, cap=2)
    assert len(tiles) == 6 and tiles[:2].tolist() == [[0, 4, 0, 0], [4, 4, 0, 0]] and (tiles[2:] == -7).all()


def test_two_to_the_31_rows_are_refused():
    lib = _native.load()
    nseg = (1 << 31) // SORT_CAP
    sizes = np.full(nseg, SORT_CAP, dtype=np.int64)
    assert lib.svs_internal_segments_plan(sizes.ctypes.data, None, nseg, 512, None, 0, None, None) == _native.SVS_ERR_UNSUPPORTED
    assert "2^31" in _native.last_error()
    sizes[-1] -= 1   # one row fewer fits
    assert lib.svs_internal_segments_plan(sizes.ctypes.data, None, nseg, 512, None, 0, None, None) == nseg * (SORT_CAP // 512)
    big = np.array([1 << 40], dtype=np.int64)   # a large segment is not part of the list
    assert lib.svs_internal_segments_plan(big.ctypes.data, None, 1, 512, None, 0, None, None) == 0


def test_bad_arguments_are_refused():
    lib = _native.load()
    one = np.array([4], dtype=np.int64)
    neg = np.array([4, -1], dtype=np.int64)
    assert lib.svs_internal_segments_plan(one.ctypes.data, None, 1, 0, None, 0, None, None) == _native.SVS_ERR_INVALID
    assert lib.svs_internal_segments_plan(neg.ctypes.data, None, 2, 8, None, 0, None, None) == _native.SVS_ERR_INVALID
    assert lib.svs_internal_segments_plan(one.ctypes.data, None, -1, 8, None, 0, None, None) == _native.SVS_ERR_INVALID
    assert lib.svs_internal_segments_plan(one.ctypes.data, None, 1, 8, None, 3, None, None) == _native.SVS_ERR_INVALID
