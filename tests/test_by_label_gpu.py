"""GPU: the per-label breakdown (svs_index_search_by_label; svs_amd/csrc/by_label.h) against its definition.

The truth is ``idx.scores(q)`` (svs_index_scores_n: the same kernel), ``idx.labels()`` and the masked rows fed to the
numpy model (by_label_model.py): labels, rows, totals and groups must be EQUAL, score bits equal with NaN canonicalised
as in test_above_gpu.py.  No tolerances.

Shape: N = 24,579 rows (3 x 8,192 + 3: no multiple of 4, several strips for any strip size up to 8,192, the last strip
holds 3 rows) of 64 unit-norm Gaussian elements, under f32, f16 and fp8.  The reduce kernel strides over strips
(BL_GRID_MAX workgroups at most), so one more case, ``test_several_strips_per_workgroup``, has
n = 2 * BL_GRID_MAX * BL_STRIP + BL_STRIP + 3 rows (2,101,251 with the constants as they are: two strips for every
workgroup, a third for the first, and a ragged rest of 3 rows), read from the library.

The label column: row r carries the DEALT label 10 + 2 (r mod 1030), so every strip holds every dealt label; then
  rows 50 .. 59 stay unlabelled (0);  rows 123 and 9000 carry 0xFFFFFFFF;
  ONE_FIRST lives in the first strip only (rows 7, 900, 4000), ONE_LAST in the last full strip only (rows 20485 and
  24575), ONE_TAIL in the 3-row tail only (row 24577);
  row N - 1 (in the tail) IS query 0, so it is the best row of its dealt label and of the corpus;
  rows 17 and 20000 are one vector under ONE label (different strips), rows 33 and 15000 one vector under two labels;
  both vectors lie close to query 0 so that they are the best of their labels."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import above_model
import by_label_model
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N, D = 24579, 64
DTYPES = ["f32", "f16", "fp8"]
DEALT = 1030
ONE_FIRST, ONE_LAST, ONE_TAIL, TOP = 5_000_001, 5_000_002, 5_000_003, 0xFFFFFFFF
NEG_INF = np.float32(-np.inf)


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _dealt(r):
    return 10 + 2 * (int(r) % DEALT)


def _column():
    lab = (10 + 2 * (np.arange(N) % DEALT)).astype(np.uint32)
    lab[50:60] = 0
    lab[[123, 9000]] = TOP
    lab[[7, 900, 4000]] = ONE_FIRST
    lab[[20485, 24575]] = ONE_LAST
    lab[24577] = ONE_TAIL
    lab[20000] = lab[17]
    return lab


# 1,024 labels: the five special ones, 0, and the dealt labels number 3 .. 1020 -- dealt labels 0 .. 2 lie below every
# dealt entry of the set, 1021 .. 1029 above them, and every odd value between two entries is a label nobody carries
SET_BIG = [0, TOP, ONE_FIRST, ONE_LAST, ONE_TAIL] + [10 + 2 * i for i in range(3, 1022)]
assert len(set(SET_BIG)) == 1024


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20262)
    m = _unit(rng.standard_normal((N, D)))
    q = _unit(rng.standard_normal((3, D)))
    near = lambda w: _unit(q[0] + w * _unit(rng.standard_normal(D)))
    m[N - 1] = q[0]
    m[17] = m[20000] = near(0.3)
    m[33] = m[15000] = near(0.4)
    lab = _column()
    m.setflags(write=False)
    lab.setflags(write=False)
    return m, q, lab


@pytest.fixture(scope="module", params=DTYPES)
def case(request, gpu, data):
    m, q, lab = data
    idx = svs_amd.DeviceIndex(m, dtype=request.param)
    idx.set_labels(lab)
    assert idx.labels().tolist() == lab.tolist()
    s = [idx.scores(qq) for qq in q]          # the reference, computed once, never written
    for v in s:
        v.setflags(write=False)
    yield SimpleNamespace(idx=idx, s=s, m=m, q=q, lab=lab, dtype=request.param)
    idx.release()


def _canon(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).tolist()


def _check(got, exp, what, row_offset=0):
    l, s, r, t, g = got
    el, es, er, et, eg = exp
    assert g == eg, (what, g, eg)
    assert l.tolist() == el.tolist(), what
    assert r.tolist() == (er + row_offset).tolist(), what
    assert t.tolist() == et.tolist(), what
    assert _canon(s) == _canon(es), what


def _ask(c, qi, label_set, cut=None, n=None, dead=None, what=None):
    """One query through the Python entry, checked against the model; returns the answer."""
    got = c.idx.search_batch_by_label(c.q[qi:qi + 1], label_set, None if cut is None else [cut], n)[0]
    exp = by_label_model.by_label(c.s[qi], c.lab, dead, label_set, cut, len(list(label_set)) if n is None else n)
    _check(got, exp, (c.dtype, what))
    return got


def _raw(idx, q, labels, cuts, k, outs, counts, groups, d=None, nq=None, nlabels=None):
    q = np.ascontiguousarray(q, dtype=np.float32)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    cuts = None if cuts is None else np.ascontiguousarray(cuts, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    return idx._lib.svs_index_search_by_label(idx._handle(), q.ctypes.data, q.shape[0] if nq is None else nq, q.shape[1] if d is None else d,
                                              p(lab), (0 if lab is None else len(lab)) if nlabels is None else nlabels, p(cuts), k,
                                              *[p(o) for o in outs], p(counts), p(groups))


def _fresh(nq, k):
    outs = (np.full((nq, k), 7, dtype=np.uint32), np.full((nq, k), -7.0, dtype=np.float32),
            np.full((nq, k), -7, dtype=np.int64), np.full((nq, k), -7, dtype=np.int64))
    return outs, np.full(nq, -7, dtype=np.int32), np.full(nq, -7, dtype=np.int32)


def _untouched(outs, counts=None, groups=None, frm=0):
    ok = (outs[0][..., frm:] == 7).all() and all((o[..., frm:] == -7).all() for o in outs[1:])
    return ok and (counts is None or (counts == -7).all()) and (groups is None or (groups == -7).all())


def test_cross_strip_merge(case):
    c = case
    l, s, r, t, g = _ask(c, 0, SET_BIG, NEG_INF, what="big set")
    assert g == 1024 and len(l) == 1024 and int(t.sum()) == N - int((~np.isin(c.lab, SET_BIG)).sum())
    at = {int(x): i for i, x in enumerate(l.tolist())}
    # every dealt label has rows in every strip; the one-strip labels: first strip, last full strip, the 3-row tail
    assert t[at[ONE_FIRST]] == 3 and r[at[ONE_FIRST]] in (7, 900, 4000)
    assert t[at[ONE_LAST]] == 2 and r[at[ONE_LAST]] in (20485, 24575)
    assert t[at[ONE_TAIL]] == 1 and r[at[ONE_TAIL]] == 24577
    assert t[at[0]] == 10 and t[at[TOP]] == 2
    # the best row of a dealt label sits in the tail, and is the best of the corpus
    assert r[0] == N - 1 and l[0] == _dealt(N - 1) and t[0] == len(np.nonzero(c.lab == _dealt(N - 1))[0])
    for qi in (1, 2):
        _ask(c, qi, SET_BIG, NEG_INF, what=("big set", qi))


def test_ties(case):
    c = case
    s = c.s[0]
    assert s[17].view(np.uint32) == s[20000].view(np.uint32) and s[33].view(np.uint32) == s[15000].view(np.uint32)
    # one vector twice under ONE label, in different strips: the higher row wins
    l, sc, r, t, g = _ask(c, 0, [int(c.lab[17])], NEG_INF, what="tie in a label")
    assert r.tolist() == [20000] and t[0] == int((c.lab == c.lab[17]).sum())
    # one vector under TWO labels: equal best scores, ordered by row descending
    a, b = int(c.lab[33]), int(c.lab[15000])
    assert a != b
    l, sc, r, t, g = _ask(c, 0, [a, b], NEG_INF, what="tie across labels")
    assert l.tolist() == [b, a] and r.tolist() == [15000, 33] and sc[0].view(np.uint32) == sc[1].view(np.uint32)


def test_set_edges(case):
    c = case
    for label_set in ([ONE_TAIL], [0], [TOP], [_dealt(5), _dealt(700)], [0, TOP], [_dealt(400), ONE_FIRST, 13],
                      [13, 15], [_dealt(500), _dealt(501), _dealt(502)]):
        for cut in (NEG_INF, np.float32(0.1)):
            _ask(c, 1, label_set, cut, what=(label_set, float(cut)))
    # stored labels below set[0] (0, dealt 0 .. 499), above the last entry (dealt 503 .., TOP), between entries (dealt 501)
    l, _, _, t, g = _ask(c, 1, [_dealt(500), _dealt(502)], NEG_INF, what="between")
    assert g == 2 and sorted(l.tolist()) == [_dealt(500), _dealt(502)]
    # label 0 with unlabelled rows present, 0xFFFFFFFF as a label
    l, _, r, t, g = _ask(c, 1, [0, TOP], NEG_INF, what="0 and TOP")
    assert dict(zip(l.tolist(), t.tolist())) == {0: 10, TOP: 2} and set(r.tolist()) <= set(range(50, 60)) | {123, 9000}
    # repeats and a shuffled order give the identical answer
    rng = np.random.default_rng(5)
    base = c.idx.search_batch_by_label(c.q[1:2], SET_BIG, [np.float32(0.2)], 40)[0]
    mixed = np.array(SET_BIG + SET_BIG[:300], dtype=np.uint32)
    rng.shuffle(mixed)
    again = c.idx.search_batch_by_label(c.q[1:2], mixed, [np.float32(0.2)], 40)[0]
    _check(again, base[:4] + (base[4],), "shuffled")
    _check(base, by_label_model.by_label(c.s[1], c.lab, None, SET_BIG, np.float32(0.2), 40), "big set, cut")
    # 1,025 distinct labels
    with pytest.raises(NotImplementedError, match="1025 distinct"):
        c.idx.search_by_label(c.q[0], list(range(1025)))
    assert c.idx.search_by_label(c.q[0], []) == []


def test_no_column_and_one_label_holding_every_row(gpu, data):
    m, q, _ = data
    for dtype in DTYPES:
        idx = svs_amd.DeviceIndex(m, dtype=dtype)
        try:
            s = idx.scores(q[0])
            c = SimpleNamespace(idx=idx, s=[s], q=q, lab=None, dtype=dtype)
            # no column: {0} holds every live row; a set without 0 gives no group
            l, sc, r, t, g = _ask(c, 0, [0], NEG_INF, what="no column")
            assert (l.tolist(), r.tolist(), t.tolist(), g) == ([0], [N - 1], [N], 1)
            _ask(c, 0, [0, 5, 9], np.float32(0.3), what="no column, cut")
            assert idx.search_batch_by_label(q[:1], [1, 2, TOP])[0][4] == 0
            # a column in which ONE label holds all 24,579 rows, cut-off -inf: the count's width, the same-slot path
            idx.set_labels(np.full(N, 77, dtype=np.uint32))
            c.lab = np.full(N, 77, dtype=np.uint32)
            for label_set in ([77], [3, 77, 900]):
                l, sc, r, t, g = _ask(c, 0, label_set, NEG_INF, what="one label")
                assert (l.tolist(), r.tolist(), t.tolist(), g) == ([77], [N - 1], [N], 1)
        finally:
            idx.release()


def test_cut_offs(case):
    c = case
    s = c.s[1]
    label_set = [_dealt(i) for i in range(40, 60)] + [ONE_LAST]
    full = _ask(c, 1, label_set, NEG_INF, what="-inf")
    assert full[4] == 21
    _check(c.idx.search_batch_by_label(c.q[1:2], label_set)[0], full[:4] + (21,), "min_scores=None")
    # exactly one group's best score: inclusive; the next float above it: the group disappears
    i = 10
    best = np.float32(full[1][i])
    at = _ask(c, 1, label_set, best, what="at the best score")
    up = _ask(c, 1, label_set, np.nextafter(best, np.float32(np.inf)), what="just above")
    assert at[4] == i + 1 and at[0][-1] == full[0][i] and at[3][-1] == 1
    assert up[4] == i and full[0][i] not in up[0]
    # -0.0 against +0.0; +inf admits nothing
    a = _ask(c, 1, label_set, np.float32(0.0), what="+0.0")
    b = _ask(c, 1, label_set, np.float32(-0.0), what="-0.0")
    _check(a, b[:4] + (b[4],), "zeros")
    assert 0 < int(a[3].sum()) < int(full[3].sum())
    assert _ask(c, 1, label_set, np.float32(np.inf), what="+inf")[4] == 0
    with pytest.raises(ValueError, match="query 0"):
        c.idx.search_by_label(c.q[0], [1], float("nan"))


def test_nan_score_qualifies_for_every_cut_off(gpu, data):
    m, q, lab = data
    mm = m[:9001].copy()
    mm[1234, 5] = np.nan
    idx = svs_amd.DeviceIndex(mm, dtype="f32")
    try:
        idx.set_labels(lab[:9001])
        s = idx.scores(q[2])
        assert np.isnan(s[1234])
        c = SimpleNamespace(idx=idx, s=[None, None, s], q=q, lab=lab[:9001], dtype="f32")
        mine = int(lab[1234])
        for cut in (np.float32(np.inf), np.float32(0.2), NEG_INF):
            l, sc, r, t, g = _ask(c, 2, [mine, _dealt(3), _dealt(4)], cut, what=("nan", float(cut)))
            assert l[0] == mine and r[0] == 1234 and np.isnan(sc[0])
        assert idx.search_batch_by_label(q[2:3], [mine, _dealt(3)], [np.inf])[0][3].tolist() == [1]
    finally:
        idx.release()


def test_k(case):
    c = case
    label_set = [_dealt(i) for i in range(100, 130)]
    exp = by_label_model.by_label(c.s[2], c.lab, None, label_set, np.float32(0.15), 1 << 20)
    G = exp[4]
    assert 8 < G <= 30
    # k < |G| cuts; k > nlabels: the caller's stride is k; entries past the count are untouched
    for k in (1, 5, G, 30, 47):
        outs, counts, groups = _fresh(1, k)
        assert _raw(c.idx, c.q[2:3], label_set, [0.15], k, outs, counts, groups) == 0, _native.last_error()
        cnt = min(k, G)
        assert counts.tolist() == [cnt] and groups.tolist() == [G]
        got = tuple(o[0, :cnt] for o in outs) + (G,)
        _check(got, tuple(e[:cnt] for e in exp[:4]) + (G,), (c.dtype, k))
        assert _untouched(outs, frm=cnt)
        _ask(c, 2, label_set, np.float32(0.15), n=k, what=("n", k))
    # k = 0 and k < 0: count-only, null result pointers; out_groups may be NULL
    for k in (0, -4):
        counts, groups = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
        assert _raw(c.idx, c.q[2:3], label_set, [0.15], k, (None,) * 4, counts, groups) == 0, _native.last_error()
        assert counts.tolist() == [0] and groups.tolist() == [G]
    counts = np.full(1, -7, dtype=np.int32)
    assert _raw(c.idx, c.q[2:3], label_set, [0.15], 0, (None,) * 4, counts, None) == 0 and counts.tolist() == [0]
    assert c.idx.search_batch_by_label(c.q[2:3], label_set, [0.15], 0)[0][4] == G
    # nq == 0 and nlabels == 0: nothing launched
    outs, counts, groups = _fresh(2, 3)
    assert _raw(c.idx, c.q[:2], None, [0.1, 0.1], 3, outs, counts, groups) == 0
    assert counts.tolist() == [0, 0] and groups.tolist() == [0, 0] and _untouched(outs) and _native.last_launches() == []
    outs, counts, groups = _fresh(2, 3)
    assert _raw(c.idx, c.q[:2], label_set, [0.1, 0.1], 3, outs, counts, groups, nq=0) == 0
    assert _untouched(outs, counts, groups) and _native.last_launches() == []


def test_three_queries_in_one_call(case):
    c = case
    s = c.s
    # query 0 fills every slot; query 1's cut leaves two groups; query 2's none: a table that is not zeroed in between
    # would carry query 0's groups over
    two = by_label_model.by_label(s[1], c.lab, None, SET_BIG, NEG_INF, 3)
    cuts = [NEG_INF, np.float32(two[1][1]), np.float32(np.inf)]
    for _ in range(2):                                        # the call repeated on the same handle
        batch = c.idx.search_batch_by_label(c.q, SET_BIG, cuts)
        assert [b[4] for b in batch] == [1024, 2, 0]
        for qi in range(3):
            exp = by_label_model.by_label(s[qi], c.lab, None, SET_BIG, cuts[qi], 1024)
            _check(batch[qi], exp, (c.dtype, "batch", qi))
            _check(c.idx.search_batch_by_label(c.q[qi:qi + 1], SET_BIG, cuts[qi:qi + 1])[0], exp, (c.dtype, "alone", qi))
    rev = c.idx.search_batch_by_label(c.q[::-1], SET_BIG, cuts[::-1])[::-1]
    for a, b in zip(rev, batch):
        _check(a, b[:4] + (b[4],), "reversed")


def test_tombstones(gpu, data, case):
    m, q, lab = data
    dtype = case.dtype
    s = case.s[0]
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        idx.set_labels(lab)
        c = SimpleNamespace(idx=idx, s=[s], q=q, lab=lab, dtype=dtype)
        dead = np.zeros(N, dtype=bool)
        # the best row of a label (N - 1, in the tail): the runner-up takes over
        top = _dealt(N - 1)
        before = _ask(c, 0, [top, ONE_TAIL, ONE_FIRST], NEG_INF, what="before")
        dead[N - 1] = True
        idx.mask_rows([N - 1])
        after = _ask(c, 0, [top, ONE_TAIL, ONE_FIRST], NEG_INF, dead=dead, what="best row masked")
        i, j = before[0].tolist().index(top), after[0].tolist().index(top)
        assert after[2][j] != N - 1 and after[3][j] == before[3][i] - 1 and after[4] == 3
        # every row of a label: the label leaves G
        dead[[7, 900, 4000, 24577]] = True
        idx.mask_rows([7, 900, 4000, 24577])
        gone = _ask(c, 0, [top, ONE_TAIL, ONE_FIRST], NEG_INF, dead=dead, what="labels masked")
        assert gone[4] == 1 and gone[0].tolist() == [top]
        # each of the four nibble positions, a whole bitmap word, the other tail rows; then a random 5 %
        more = [1000, 1001, 1002, 1003, 2005, 2010, 2015, 2016, 24576, 24578] + list(range(6400, 6432))
        dead[more] = True
        idx.mask_rows(more)
        _ask(c, 0, SET_BIG, NEG_INF, dead=dead, what="nibbles")
        rnd = np.nonzero((np.random.default_rng(8).random(N) < 0.05) & ~dead)[0]
        dead[rnd] = True
        idx.mask_rows(rnd)
        got = _ask(c, 0, SET_BIG, np.float32(0.05), dead=dead, what="5 % masked")
        assert not dead[got[2]].any()
        # -inf: a masked row never comes back through its score
        got = _ask(c, 0, SET_BIG, NEG_INF, dead=dead, what="5 % masked, -inf")
        assert int(got[3].sum()) == int((~dead & np.isin(lab, SET_BIG)).sum())
    finally:
        idx.release()


def test_append_compact_and_row_offset(gpu, data, case):
    m, q, lab = data
    dtype = case.dtype
    off = 1_000_000
    idx = svs_amd.DeviceIndex(m[:9000], dtype=dtype, row_offset=off)
    try:
        idx.set_labels(lab[:9000])
        s = idx.scores(q[1])
        label_set = [0, TOP] + [_dealt(i) for i in range(0, 200)]
        c = SimpleNamespace(idx=idx, s=[None, s], q=q, lab=lab[:9000], dtype=dtype)
        got = idx.search_batch_by_label(q[1:2], label_set, [np.float32(0.1)])[0]
        _check(got, by_label_model.by_label(s, c.lab, None, label_set, np.float32(0.1), len(label_set)), "row_offset", row_offset=off)
        assert (got[2] >= off).all()
        # after append: the new rows carry label 0
        idx.append(m[9000:9500])
        s2 = idx.scores(q[1])
        lab2 = np.concatenate([lab[:9000], np.zeros(500, dtype=np.uint32)])
        assert idx.labels().tolist() == lab2.tolist()
        got = idx.search_batch_by_label(q[1:2], label_set)[0]
        exp = by_label_model.by_label(s2, lab2, None, label_set, None, len(label_set))
        _check(got, exp, "append", row_offset=off)
        assert dict(zip(got[0].tolist(), got[3].tolist()))[0] == 510
        # after compact: the labels move with the rows
        dead = np.zeros(9500, dtype=bool)
        dead[[0, 55, 123, 4000, 9499]] = True
        dead[2000:2600] = True
        idx.mask_rows(np.nonzero(dead)[0] + off)
        _check(idx.search_batch_by_label(q[1:2], label_set)[0], by_label_model.by_label(s2, lab2, dead, label_set, None, len(label_set)),
               "masked", row_offset=off)
        old = idx.compact()
        keep = np.nonzero(~dead)[0]
        assert (old - off).tolist() == keep.tolist()
        s3 = idx.scores(q[1])
        assert idx.labels().tolist() == lab2[keep].tolist()
        got = idx.search_batch_by_label(q[1:2], label_set, [np.float32(0.0)])[0]
        _check(got, by_label_model.by_label(s3, lab2[keep], None, label_set, np.float32(0.0), len(label_set)), "compacted", row_offset=off)
    finally:
        idx.release()


def test_cross_checks_against_other_entries(case):
    c = case
    every = sorted(set(c.lab.tolist()))
    assert len(every) > 1024
    rest = every[1024:]
    for qi, cut in ((0, np.float32(0.2)), (1, np.float32(0.0)), (2, NEG_INF)):
        a = c.idx.search_batch_by_label(c.q[qi:qi + 1], every[:1024], [cut])[0]
        b = c.idx.search_batch_by_label(c.q[qi:qi + 1], rest, [cut])[0]
        # a set (here: two) covering every stored label: the totals add up to search_above's, the first entry is its first
        sc, rows, total = c.idx.search_batch_above(c.q[qi:qi + 1], [cut], 1)[0]
        assert int(a[3].sum()) + int(b[3].sum()) == total == c.idx.search_batch_above(c.q[qi:qi + 1], [cut], 0)[0][2]
        first = max((x for x in (a, b) if len(x[2])), key=lambda x: (above_model.score_key(x[1][0])[0], x[2][0]))
        assert first[2][0] == rows[0] and _canon(first[1][:1]) == _canon(sc)
    # one label, -inf: the total is search_labeled's count-only `matched`
    for label in (_dealt(3), 0, TOP, ONE_TAIL, 13):
        got = c.idx.search_batch_by_label(c.q[:1], [label])[0]
        matched = c.idx.search_batch_labeled(c.q[:1], 0, [label])[2]
        assert (int(got[3][0]) if got[4] else 0) == matched == int((c.lab == label).sum())


def test_launch_record(case):
    c = case
    c.idx.search_batch_by_label(c.q, SET_BIG, [0.1, 0.2, -np.inf], 5)
    rec = _native.last_launches()
    names = [k for k, _, _ in rec]
    assert [e for e in rec if e[0] == "by_label_reduce_kernel"] == [("by_label_reduce_kernel", N, 1)] * 3
    assert names.count("gemv") == 3 and len(names) == 9, names       # per query: "gemv", its score kernel, the reduction
    kernels = [k for k in names if k not in ("gemv", "by_label_reduce_kernel")]
    assert len(kernels) == 3 and len(set(kernels)) == 1, names
    c.idx.scores(c.q[0])
    assert _native.last_launches()[1][0] == kernels[0]               # the kernel svs_index_scores_n runs
    assert not [k for k in names if k.startswith(("select_", "keys_", "bitonic", "above_", "label_", "gather_"))], names


def test_four_threads_on_one_handle(case):
    c = case
    asks = [(0, SET_BIG, NEG_INF), (1, [_dealt(i) for i in range(0, 300)], np.float32(0.1)),
            (2, [0, TOP, ONE_FIRST, ONE_LAST, ONE_TAIL], np.float32(-0.2)), (1, [_dealt(77)], np.float32(0.3))]
    want = [by_label_model.by_label(c.s[qi], c.lab, None, ls, cut, len(ls)) for qi, ls, cut in asks]
    got = [[] for _ in asks]
    errors = []

    def work(i):
        qi, ls, cut = asks[i]
        try:
            for _ in range(6):
                got[i].append(c.idx.search_batch_by_label(c.q[qi:qi + 1], ls, [cut])[0])
        except BaseException as e:          # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(asks))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, answers in enumerate(got):
        assert len(answers) == 6
        for a in answers:
            _check(a, want[i], (c.dtype, "thread", i))


def test_both_cross_workgroup_routes_give_the_same_bits(case):
    c = case
    lib = _native.load()
    cuts = [NEG_INF, np.float32(0.15), np.float32(0.3)]
    base = c.idx.search_batch_by_label(c.q, SET_BIG, cuts)
    try:
        assert lib.svs_internal_tune(7, 1) == 0
        other = c.idx.search_batch_by_label(c.q, SET_BIG, cuts)
        one = c.idx.search_batch_by_label(c.q[:1], [77, ONE_TAIL], cuts[:1])[0]
    finally:
        assert lib.svs_internal_tune(7, 0) == 0
    for qi, (a, b) in enumerate(zip(base, other)):
        _check(b, a[:4] + (a[4],), "partials")
        _check(a, by_label_model.by_label(c.s[qi], c.lab, None, SET_BIG, cuts[qi], 1024), (c.dtype, qi))
    _check(one, by_label_model.by_label(c.s[0], c.lab, None, [77, ONE_TAIL], NEG_INF, 2), "partials, small set")
    _check(c.idx.search_batch_by_label(c.q, SET_BIG, cuts)[1], base[1][:4] + (base[1][4],), "back")


def test_argument_errors_leave_the_outputs_untouched(case):
    c = case
    k = 4
    q2, ok, ls = c.q[:2], [0.1, 0.2], [1, 2, 3]
    INV, SHAPE, UNS = _native.SVS_ERR_INVALID, _native.SVS_ERR_SHAPE, _native.SVS_ERR_UNSUPPORTED

    def call(expect, *args, outs=True, counts=True, **kw):
        o, cn, g = _fresh(2, k)
        rc = _raw(c.idx, *args, o if outs is True else outs, cn if counts else None, g, **kw)
        assert rc == expect, (rc, _native.last_error())
        assert _untouched(o, cn, g)
        return _native.last_error()

    call(SHAPE, np.zeros((2, D + 1), dtype=np.float32), ls, ok, k)
    call(INV, q2, ls, ok, k, nq=-1)
    call(INV, q2, ls, ok, k, nlabels=-1)
    call(INV, q2, None, ok, k, nlabels=3)
    assert "query 1" in call(INV, q2, ls, [0.1, np.nan], k)
    call(INV, q2, ls, ok, k, counts=False)
    call(UNS, q2, np.arange(1025), ok, k)
    for missing in range(4):
        o, cn, g = _fresh(2, k)
        part = tuple(None if i == missing else x for i, x in enumerate(o))
        assert _raw(c.idx, q2, ls, ok, k, part, cn, g) == INV and _untouched(o, cn, g)
    o, cn, g = _fresh(2, k)
    assert c.idx._lib.svs_index_search_by_label(c.idx._handle(), None, 2, D, np.array(ls, dtype=np.uint32).ctypes.data, 3, None, k,
                                                *[x.ctypes.data for x in o], cn.ctypes.data, g.ctypes.data) == INV
    assert _untouched(o, cn, g)
    empty = svs_amd.DeviceIndex.empty(D)
    try:
        o, cn, g = _fresh(2, k)
        assert _raw(empty, q2, ls, ok, k, o, cn, g) == SHAPE and _untouched(o, cn, g)
    finally:
        empty.release()
    with pytest.raises(ValueError):
        c.idx.search_batch_by_label(c.q, ls, [0.1])             # three queries, one cut-off
    with pytest.raises(ValueError):
        c.idx.search_by_label(c.q[0], [-1])


def test_several_strips_per_workgroup(gpu):
    geo = (np.zeros(2, dtype=np.int32))
    assert _native.load().svs_internal_by_label_geometry(geo.ctypes.data_as(_native.C.POINTER(_native.C.c_int32))) == 0
    strip, grid = int(geo[0]), int(geo[1])
    n = 2 * grid * strip + strip + 3          # two strips for every workgroup, a third for the first, a ragged rest
    d = 16
    rng = np.random.default_rng(77)
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    q = _unit(rng.standard_normal((1, d)))
    lab = rng.integers(0, 1500, n).astype(np.uint32)       # more labels than a set holds: some rows match nothing
    lab[n - 2] = 4_000_000                                   # a label that lives in the ragged rest only
    idx = svs_amd.DeviceIndex(m, dtype="f16")
    try:
        idx.set_labels(lab)
        dead = np.zeros(n, dtype=bool)
        dead[rng.integers(0, n, 5000)] = True
        dead[[n - 1, grid * strip, grid * strip + 1]] = True
        idx.mask_rows(np.nonzero(dead)[0])
        s = idx.scores(q[0])
        label_set = list(range(0, 1023)) + [4_000_000]
        for cut in (NEG_INF, np.float32(0.5)):
            got = idx.search_batch_by_label(q, label_set, [cut])[0]
            assert _native.last_launches()[2] == ("by_label_reduce_kernel", n, 1)
            _check(got, by_label_model.by_label(s, lab, dead, label_set, cut, len(label_set)), ("strided", float(cut)))
        one = idx.search_batch_by_label(q, [4_000_000, 7])[0]
        _check(one, by_label_model.by_label(s, lab, dead, [4_000_000, 7], None, 2), "strided, two labels")
        assert dict(zip(one[0].tolist(), one[3].tolist()))[4_000_000] == 1
    finally:
        idx.release()
