"""CPU: the groups in which the host re-runs overflowed positions of a fused batched search (next_redo_group in
svs_amd/csrc/svs_amd.hip, through svs_internal_redo_groups).

A position whose candidate list overflowed carries -2 in the first entry of its result rows.  search_host and
svs_index_neighbors re-run such positions in groups of at most `max` -- 256, and fewer once a group's score matrix would
pass 2 GiB, which takes more than 2 M rows: no quick GPU test reaches the limited case, this one does.  The model: walk
the range, collect marked positions, close a group when it holds `max` of them or the range ends (a group may span
unmarked positions)."""
import ctypes as C

import numpy as np
import pytest

from svs_amd import _native


def hook(first, count, q0, q1, mx, seed=0):
    """(groups, found): `first` = the first-entry column of nq positions; the other count - 1 entries of every position
    are noise that contains -2, so that a wrong stride finds marks that are not there."""
    nq = len(first)
    block = np.random.default_rng(seed).choice(np.array([-2, -1, 0, 5], dtype=np.int64), size=(nq, count))
    block[:, 0] = first
    block = np.ascontiguousarray(block)
    cap = max(q1 - q0, 1)
    pos, sizes, ng = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64), C.c_int64(-1)
    found = int(_native.load().svs_internal_redo_groups(block.ctypes.data, count, q0, q1, mx, pos.ctypes.data, sizes.ctypes.data, C.byref(ng)))
    assert found >= 0, _native.last_error()
    assert int(sizes[:ng.value].sum()) == found and np.all(pos[found:] == -7) and np.all(sizes[ng.value:] == -7)
    cuts = np.cumsum(sizes[:ng.value])[:-1]
    return [g.tolist() for g in np.split(pos[:found], cuts)] if found else [], found


def model(first, q0, q1, mx):
    groups, g = [], []
    for q in range(q0, q1):
        if first[q] == -2:
            g.append(q)
            if len(g) == mx:
                groups.append(g)
                g = []
    return groups + ([g] if g else [])


def check(first, count, q0, q1, mx):
    first = np.asarray(first, dtype=np.int64)
    groups, found = hook(first, count, q0, q1, mx)
    marked = [q for q in range(q0, q1) if first[q] == -2]
    assert found == len(marked)
    assert [q for g in groups for q in g] == marked            # the union, in order: ascending, inside [q0, q1)
    assert all(1 <= len(g) <= mx for g in groups)
    assert groups == model(first, q0, q1, mx)
    return groups


def mask(nq, marked):
    first = np.arange(nq, dtype=np.int64)       # unmarked positions hold a row number (0 and up), never -2
    first[list(marked)] = -2
    return first


@pytest.mark.parametrize("count", [1, 7])
@pytest.mark.parametrize("mx", [1, 3, 256])
def test_groups_of_chosen_masks(count, mx):
    nq = 40
    assert check(mask(nq, []), count, 0, nq, mx) == []                                   # nothing marked
    every = check(mask(nq, range(nq)), count, 0, nq, mx)                                 # all marked
    assert len(every) == -(-nq // mx) and all(len(g) == mx for g in every[:-1])
    check(mask(nq, [3, 4, 9, 20, 21, 22, 37]), count, 0, nq, mx)                         # scattered
    check(mask(nq, [0, nq - 1]), count, 0, nq, mx)                                       # first and last index
    check(mask(nq, [0]), count, 0, nq, mx)
    check(mask(nq, [nq - 1]), count, 0, nq, mx)
    # a range inside the block: marks outside it (2, 9, 30, 39) are not touched, those on its edges (10, 29) are
    inner = check(mask(nq, [2, 9, 10, 15, 16, 29, 30, 39]), count, 10, 30, mx)
    assert [q for g in inner for q in g] == [10, 15, 16, 29]
    assert check(mask(nq, [2, 39]), count, 10, 30, mx) == []
    assert check(mask(nq, [5]), count, 5, 5, mx) == []                                   # an empty range


def test_more_than_one_full_group_at_the_production_limit():
    """600 marked positions at max = 256 (REDO_BATCH): 256 + 256 + 88."""
    groups = check(mask(600, range(600)), 7, 0, 600, 256)
    assert [len(g) for g in groups] == [256, 256, 88]
    # the limited case of a 10 M-row corpus: 2 GiB / (4 bytes x 10 M rows) = 53 positions per pass
    assert [len(g) for g in check(mask(600, range(0, 600, 2)), 1, 0, 600, 53)] == [53] * 5 + [35]


def test_random_masks_match_the_model():
    rng = np.random.default_rng(5)
    for _ in range(300):
        nq = int(rng.integers(1, 601))
        first = mask(nq, np.flatnonzero(rng.random(nq) < rng.choice([0.02, 0.3, 0.9])))
        q0 = int(rng.integers(0, nq + 1))
        q1 = int(rng.integers(q0, nq + 1))
        check(first, int(rng.choice([1, 7])), q0, q1, int(rng.choice([1, 3, 53, 256])))


def test_bad_arguments_are_refused():
    lib = _native.load()
    a = np.zeros(8, dtype=np.int64)
    ng = C.c_int64(0)
    for count, q0, q1, mx in [(0, 0, 4, 3), (1, -1, 4, 3), (1, 5, 4, 3), (1, 0, 4, 0), (1, 0, 4, 257)]:
        assert lib.svs_internal_redo_groups(a.ctypes.data, count, q0, q1, mx, a.ctypes.data, a.ctypes.data, C.byref(ng)) == _native.SVS_ERR_INVALID
    assert lib.svs_internal_redo_groups(None, 1, 0, 4, 3, a.ctypes.data, a.ctypes.data, C.byref(ng)) == _native.SVS_ERR_INVALID
