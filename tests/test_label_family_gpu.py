"""GPU: the three entries that take a label SET -- svs_index_search_labeled, svs_index_search_by_label and
svs_index_label_sums -- build it with one host type (LabelSet) and search it with one device function (label_slot), so
they must agree on membership: per distinct label, the rows ``search_batch_by_label`` totals, the rows ``label_sums``
counts and the rows numpy selects among the live ones are the same number, and their sum is what
``search_batch_labeled`` reports as matched.  Every comparison is integer equality.

Corpora: f16, d = 32, row counts one either side of the three kernels' workgroup strips (label_sums.h 1,024 rows,
labels.h 2,048, by_label.h 4,096); labels from a pool of five values with 0 and 2^32 - 1 among them; tombstones on the
first and last row of every strip.  Sets of 1, 2, 3 and 1,024 distinct labels, given unsorted, with repeats and with
labels no row carries.  Also here: the 1,025-label refusal of all three entries, and the one rule of the two timing
hooks (svs_internal_assign_kernel_ms, svs_internal_label_sums_kernel_ms)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import by_label_model
import collapse_model

D = 32
SIZES = [1023, 1025, 2049, 4099]
LS_STRIP = 1024                                       # label_sums.h (not exported; the other two are read below)
POOL = np.array([0, 1, 7, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
WEIGHTS = [0.3, 0.1, 0.1, 0.1, 0.4]
ABSENT = [5, 0xFFFFFFFE]                              # no row carries them, nor any of FILL
FILL = list(range(1000, 1000 + 1024))
SET_SIZES = [1, 2, 3, 1024]


def _model(n):
    """The rows and labels of the n-row corpus"""
    rng = np.random.default_rng(4100 + n)
    m = rng.standard_normal((n, D)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    lab = POOL[rng.choice(len(POOL), size=n, p=WEIGHTS)]
    return m, lab


def _dead_rows(n, strips, rng):
    edge = {0, n - 1}
    for s in strips:
        edge |= {r for r in (s - 1, s, 2 * s - 1, 2 * s) if r < n}
    return np.array(sorted(edge | set(rng.integers(0, n, size=5).tolist())), dtype=np.int64)


def _label_lists(lab, live):
    """{case: the caller's list}: unsorted, with repeats, naming labels that no row carries (a set of one label: the
    most frequent label, and an absent one)."""
    counts = {int(v): int(np.count_nonzero(lab[live] == v)) for v in POOL}
    by_freq = sorted(counts, key=counts.get, reverse=True)
    top, second = by_freq[0], by_freq[1]
    big = [int(v) for v in POOL] + ABSENT + FILL[:1024 - len(POOL) - len(ABSENT)]
    big = np.random.default_rng(7).permutation(np.array(big, dtype=np.uint64)).tolist()
    lists = {
        "1-present": [top, top],
        "1-absent": [ABSENT[0], ABSENT[0], ABSENT[0]],
        "2": [ABSENT[1], top, ABSENT[1]],
        "3": [top, ABSENT[0], second, top, ABSENT[0]],
        "1024": big + [big[3], big[900], big[3]],
    }
    for name, lst in lists.items():
        assert len(set(lst)) == int(name.split("-")[0]) and len(lst) > len(set(lst))
    assert {len(set(lst)) for lst in lists.values()} == set(SET_SIZES)
    return lists


def _host_counts(lab, live, labels):
    """(c): per distinct label of the list, the live rows that carry it"""
    return {int(v): int(np.count_nonzero(np.isin(lab, np.uint32(v)) & live)) for v in set(labels)}


def _live(n, dead):
    live = np.ones(n, dtype=bool)
    live[dead] = False
    return live


def test_host_model_counts_are_not_trivial():
    """No GPU: for the seeds above, every corpus and every list but the absent single label has a label of more than
    256 live rows, and every list that can has one with none."""
    for n in SIZES:
        _, lab = _model(n)
        live = _live(n, _dead_rows(n, [LS_STRIP, 2048, 4096], np.random.default_rng(n)))
        assert 0 < np.count_nonzero(~live) < 32
        for name, labels in _label_lists(lab, live).items():
            c = _host_counts(lab, live, labels)
            assert (max(c.values()) > 256) == (name != "1-absent"), (n, name, c)
            assert (min(c.values()) == 0) == (name != "1-present"), (n, name, c)
            assert 0 in c or name != "1024"
            assert sum(c.values()) <= np.count_nonzero(live)


@pytest.fixture(scope="module")
def strips(gpu):
    from svs_amd import _native
    lib = _native.load()
    geo = np.zeros(2, dtype=np.int32)
    assert lib.svs_internal_by_label_geometry(geo.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    got = [LS_STRIP, int(lib.svs_internal_labels_strip()), int(geo[0])]
    for s in got:      # every strip length has a corpus that ends inside the first strip and one just past it
        assert any(n < s for n in SIZES) and any(s < n <= s + 3 for n in SIZES), (s, SIZES)
    return got


@pytest.fixture(scope="module", params=SIZES, ids=lambda n: f"n{n}")
def case(request, strips):
    import svs_amd
    n = request.param
    m, lab = _model(n)
    dead = _dead_rows(n, strips, np.random.default_rng(n))
    live = _live(n, dead)
    idx = svs_amd.DeviceIndex(m, dtype="f16")
    idx.set_labels(lab)
    idx.mask_rows(dead)
    q = m[[1, n // 2]] if n > 2 else m[:1]
    for a in (m, lab, live):
        a.setflags(write=False)
    yield SimpleNamespace(idx=idx, n=n, lab=lab, live=live, q=np.ascontiguousarray(q), lists=_label_lists(lab, live))
    idx.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1-present", "1-absent", "2", "3", "1024"])
def test_the_three_entries_agree_on_membership(case, name):
    k = case
    labels = k.lists[name]
    want = _host_counts(k.lab, k.live, labels)                                   # (c)
    # (a) every query's totals, without a cut-off: every live row of the label qualifies
    for got_l, _, _, totals, groups in k.idx.search_batch_by_label(k.q, labels, None, n=len(labels)):
        a = dict.fromkeys(want, 0)
        a.update(zip(got_l.tolist(), totals.tolist()))
        assert a == want and groups == sum(1 for v in want.values() if v)
    # (b) the histogram alone; every position of a repeated label gets the same count
    _, counts = k.idx.label_sums(labels, sums=False)
    b = {}
    for v, c in zip(labels, counts.tolist()):
        assert b.setdefault(int(v), c) == c
    assert b == want
    # the filter's count
    _, _, matched = k.idx.search_batch_labeled(k.q, 0, labels)
    assert matched == sum(want.values())


@pytest.mark.gpu
def test_one_label_too_many_is_refused_by_all_three(case):
    k = case
    labels = FILL[:1024] + [3, 3]                    # 1,025 distinct
    assert len(set(labels)) == 1025
    for call in (lambda: k.idx.search_batch_labeled(k.q, 1, labels),
                 lambda: k.idx.search_batch_by_label(k.q, labels),
                 lambda: k.idx.label_sums(labels, sums=False)):
        with pytest.raises(NotImplementedError, match="at most 1024"):
            call()


@pytest.mark.gpu
def test_timing_hooks_follow_one_rule(case):
    """An entry's reading is -1 from the moment a call of that entry begins until that call has timed its kernels; a
    call of the other entry never touches it."""
    from svs_amd import _native
    k = case
    lib = _native.load()
    a_ms, l_ms = C.c_double(0.0), C.c_double(0.0)

    def readings():
        _native.check(lib.svs_internal_assign_kernel_ms(C.byref(a_ms)))
        _native.check(lib.svs_internal_label_sums_kernel_ms(C.byref(l_ms)))
        return a_ms.value, l_ms.value

    k.idx.set_timing(1)
    try:
        k.idx.label_sums([0])
        assert readings()[1] >= 0.0
        k.idx.assign(k.q)                             # timed; the label-sums reading is not this entry's
        a, l = readings()
        assert a >= 0.0 and l >= 0.0
        k.idx.label_sums([0], sums=False)             # times nothing: its own reading goes, the other stays
        assert readings() == (a, -1.0)
        # an assign that fails validation (c = 0) leaves no earlier call's time behind
        assert lib.svs_index_assign(k.idx._handle(), None, 0, D, 0, k.n, None, None, None, None) == _native.SVS_ERR_INVALID
        assert readings() == (-1.0, -1.0)
    finally:
        k.idx.set_timing(0)


# -- the wave fold that by_label_reduce_kernel and collapse_reduce_kernel share ---------------------------------------
FOLD_D = 64
FOLD_WAVE_ROWS = 256      # one call of the fold: the rows r of one 256-row block with one r % 4; lane = r % 256 // 4


def _fold_corpus(n):
    """(m, q, values, ties): blocks of 256 rows take three layouts in turn.  Block b % 3 == 0: every lane of a wave
    holds value 1000 + b.  == 1: lane l holds 100 + l, so no two lanes of a wave share a value (and every such block
    shares them with the others).  == 2: the even lanes hold 2000 + b, the leader's, every odd lane l holds
    3000 + 64 b + l.  In every block of the first and the third layout two rows on even lanes that are not lane 0, with
    one r % 4, are ONE vector close to the query: their group's largest score twice in one call of the fold, away from
    the leader.  ties: [(smaller row, larger row)]."""
    rng = np.random.default_rng(8229)
    unit = lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    m = unit(rng.standard_normal((n, FOLD_D)))
    q = unit(rng.standard_normal(FOLD_D))
    r = np.arange(n)
    b, lane = r // FOLD_WAVE_ROWS, r % FOLD_WAVE_ROWS // 4
    values = np.where(b % 3 == 0, 1000 + b, np.where(b % 3 == 1, 100 + lane, np.where(lane % 2 == 0, 2000 + b, 3000 + 64 * b + lane)))
    ties = []
    for blk in range((n + FOLD_WAVE_ROWS - 1) // FOLD_WAVE_ROWS):
        if blk % 3 == 1:
            continue
        lanes = min(64, (n - blk * FOLD_WAVE_ROWS + 3) // 4)
        e = blk % 4 if lanes == 64 else 0
        la, lb = (2 + 2 * (blk % 5), lanes - 2 - 2 * (blk % 7)) if lanes == 64 else (2, (lanes - 1) // 2 * 2)
        r1, r2 = (blk * FOLD_WAVE_ROWS + 4 * l + e for l in (la, lb))
        assert 0 < la < lb and r2 < n and values[r1] == values[r2] == values[blk * FOLD_WAVE_ROWS + e]
        m[r1] = m[r2] = unit(q + 0.05 * (1 + blk) / 40 * unit(rng.standard_normal(FOLD_D)))
        ties.append((r1, r2))
    return m, q, values.astype(np.uint32), ties


@pytest.mark.gpu
def test_both_callers_of_the_wave_fold_agree_with_their_models(strips):
    """search_by_label and search_collapsed over one corpus of 2 * BL_STRIP + 37 f32 rows whose column puts a wave's
    lanes all on one value, all on different values, and half on the leader's value with the group's largest score on two
    later lanes (_fold_corpus): labels, values, rows, totals, groups and score bits equal the numpy models' over the
    library's own scores, and every planted tie goes to the larger row."""
    import svs_amd
    n = 2 * strips[2] + 37
    m, q, values, ties = _fold_corpus(n)
    assert len(ties) >= 2 * (n // FOLD_WAVE_ROWS) // 3 and {r1 // FOLD_WAVE_ROWS % 3 for r1, _ in ties} == {0, 2}
    idx = svs_amd.DeviceIndex(m, dtype="f32")
    try:
        idx.set_labels(values)
        s = idx.scores(q)
        for r1, r2 in ties:     # the pair is the best of its group, with one score
            group = np.nonzero(values == values[r1])[0]
            assert s[r1].view(np.uint32) == s[r2].view(np.uint32) and s[r1] > np.delete(s[group], np.searchsorted(group, [r1, r2])).max()
        label_set = np.unique(values)
        assert len(label_set) <= 1024
        bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()
        # by label: every group, best first
        l, sc, rows, totals, groups = idx.search_batch_by_label(q[None, :], label_set, None, len(label_set))[0]
        el, es, er, et, eg = by_label_model.by_label(s, values, None, label_set, None, len(label_set))
        assert groups == eg == len(label_set)
        assert (l.tolist(), rows.tolist(), totals.tolist(), bits(sc)) == (el.tolist(), er.tolist(), et.tolist(), bits(es))
        assert {r2 for _, r2 in ties} <= set(rows.tolist()) and not {r1 for r1, _ in ties} & set(rows.tolist())
        # collapsed on the same column: one row per value
        for zero in ("single", "group"):
            cs, cr, cv, counts, cgroups = idx.search_batch_collapsed(q[None, :], len(label_set), 0, zero)
            es, er, ev, eg = collapse_model.collapsed(s, values, None, zero == "single", len(label_set))
            assert int(cgroups[0]) == eg == len(label_set) and int(counts[0]) == eg
            assert (cr[0].tolist(), cv[0].tolist(), bits(cs[0])) == (er.tolist(), ev.tolist(), bits(es))
            assert {r2 for _, r2 in ties} <= set(cr[0].tolist()) and not {r1 for r1, _ in ties} & set(cr[0].tolist())
    finally:
        idx.release()
