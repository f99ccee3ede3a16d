"""GPU: every entry point that reads corpus rows, on rows that lie on the 32-bit offset boundaries of a 64 GiB index.

tests/far_rows.py lays the index out (test_far_rows_layout.py checks the arithmetic without a GPU): rows of 3,072 bytes
for every dtype, six blocks of 342 planted unit-norm rows centred on byte offsets 2^31 .. 2^36 of the row buffer -- which
are also the f16 / f32 element offsets 2^31 and 2^32, 2^31 chunks (block 35) and 2^32 chunks (block 36, where
``row * ld16`` no longer fits 32 bits) -- and about 22.4M filler rows scaled by 2^-7 everywhere else.  One dtype is
resident at a time (module-scoped fixture): L, the far index, built by append_device behind a reserve; and two small
twins built the ordinary way from the same f32 rows:

  S  the 2,052 planted rows (L row = loc[S row]): the reference of every case that ranks the whole corpus;
  G  six windows of 676 rows -- each planted block with the 167 filler rows below and above it (L row = gloc[G row]):
     the reference of every case over row lists, row ranges, labels and columns, which mix planted and filler rows
     on both sides of every boundary.

Truth is numpy f64 on a twin's stored_rows and the stored queries, at the tolerances the project already holds the
kernels to (imported, not restated).  Where svs_internal_last_launches names the same kernels for L and for the twin,
rows and score BITS must be equal; elsewhere compare.assert_topk_parity decides with the f64 truth.  A filler row scores
at most far_rows.FILL_BOUND, so a whole-corpus case first asserts, on the reference alone, that the k-th best reference
score exceeds that bound plus the tolerance: its answer then holds planted rows only, and no query is left out.

Teeth (reasoned, never run): narrowing gather.h's ``(int64_t)row[u] * ld16`` to a 32-bit unsigned product sends every
row of block 36 above the boundary (rows with row * 192 >= 2^32) to chunk offset (row * 192) mod 2^32, which is one of
the first 171 rows of the buffer -- filler (test_far_rows_layout.py::test_block_36_is_where_a_32_bit_chunk_product_wraps).
Such a build compiles; under it search_within over G's list returns for those 170 rows a score below FILL_BOUND =
0.0088 where the twin has the planted row's (|score| up to 0.1, the K-th best above 0.028), so the bit comparison, the
f64 tolerance and -- in the whole-corpus cases -- search_above's total at the cut-off 0.02 all fail.  A signed 32-bit
product additionally turns negative for the upper half of block 35 and addresses below the buffer.

Out of scope: top_pairs and kmeans (quadratic, or iterative, over 22M rows), and svs_multi_* / ShardedIndex (their
shards are ordinary indices).  An f32 row of 3,072 bytes is 768 floats, and only rows of whole 512-float steps get a
half shadow, so the screened f32 route runs on a fourth index: f32 at d = 2048 (far_rows.SHADOWED: rows of 8 KiB, which
start on each boundary instead of straddling it).  Every case runs on it too, unscreened; test_screened_f32 then
turns the shadow on (98 GiB in all) and the compaction case moves rows and shadow.  The compaction case moves
the whole corpus once (about 0.1 s on an MI355X); it prints its own wall time and runs under a limit of its own
(COMPACT_LIMIT_S: faulthandler ends the process if the move is stuck).

f32 is built with the shadow off (set_screen(0) on the empty index, before the first append); hbm_bytes is then
exactly n * 3,072 (asserted), plus 4 bytes per row of scales for fp8.

The min op of the public combined entry uses SIGNED = (0.3, -1.0, 0.7) at k = 10: MIXED's zero weight makes every
row's min at most 0 and ties the filler rows with the best planted ones, so no planted-only answer exists under it.
The group-combined sum and min take positive weights for the reason given at the case.  The hook
(svs_internal_combined_scores) checks all three ops under test_combined_gpu.MIXED on both routes.

WIDEST_TOL of test_far_rows_layout.py restates the widest imported tolerance; test_tolerances_match pins it."""
import faulthandler
import time
from types import SimpleNamespace

import numpy as np
import pytest

import above_model
import assign_model
import collapse_model
import collapse_scope_model
import collapsed_combined_model
import combine_model
import diverse_model
import far_rows as fr
import ingest_model
import label_sums_model
from batch_kernel_table import _phased, _q16, _tiled
from compare import assert_topk_parity
from gather_kernel_table import CASES as GATHER_CASES
from test_batch_kernels_gpu import TOL as TOL_BATCH
from test_combined_gpu import FUSED, MIXED, OPS, PASSES, SHAPES as COMBINE_SHAPES
from test_gather_kernels_gpu import TOL as TOL_GATHER
from test_single_kernels_gpu import KERNEL as SINGLE_KERNEL, TOL as TOL_SINGLE

pytestmark = pytest.mark.gpu

CASES = ("fp8", "f16", "f32", "f32-shadowed")      # far_rows.LAYOUTS: the last is f32 at d = 2048, which has a half shadow
GIB = 1 << 30
WING = 167                      # filler rows of a window below and above its planted block
WIN = fr.BLOCK + 2 * WING       # 676
SEED_FILL = 20282
COMPACT_LIMIT_S = 120           # compact() moves a far index in 0.1 - 0.2 s on an MI355X
SIGNED = np.array([0.3, -1.0, 0.7], dtype=np.float32)       # a negative weight and no zero (module docstring)
POSITIVE = np.array([1.0, 0.7, 1.5], dtype=np.float32)      # the group-combined sum and min (module docstring)
# main pass of a fused batched search over rows of 3,072 bytes (batch_kernel_table.py's dispatch rules)
BATCH_KERNEL = {      # (f32: the same three kernels at d = 768 and at d = 2048)
    "f32": {16: _q16("f32", True), 64: _tiled(64, True, 4, 128), 256: _tiled(64, True, 4, 128)},
    "f16": {16: _q16("f16", True), 64: _tiled(64, True, 2, 128), 256: _phased(True, 2, 20, 256)},
    "fp8": {16: _tiled(32, True, 1, 128), 64: _tiled(64, True, 1, 128), 256: _phased(True, 1, 20, 256)},
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launches():
    from svs_amd import _native
    return _native.last_launches()


def _names(launches=None):
    return [x[0] for x in (_launches() if launches is None else launches)]


def _pairs(got):
    """[(score, row)] -> (f32 scores, i64 rows)"""
    return np.array([s for s, _ in got], dtype=np.float32), np.array([r for _, r in got], dtype=np.int64)


def _stored(vectors, dtype):
    """Vectors as an index of ``dtype`` stores them (queries are rounded / quantised by the same kernels)."""
    from svs_amd import DeviceIndex
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    if dtype == "f32":
        return v.copy()
    tmp = DeviceIndex(v, dtype=dtype)
    try:
        return tmp.stored_rows()
    finally:
        tmp.release()


class Twin:
    """A small index over rows of L: ``rows`` (i64, ascending) are the L rows of its rows."""

    def __init__(self, src, rows, dtype, qd64):
        from svs_amd import DeviceIndex
        self.src, self.rows, self.n = src, rows, len(rows)
        self.idx = DeviceIndex(src, dtype=dtype)
        if dtype == "f32":
            self.idx.set_screen(0)          # as L: every search reads the f32 rows
        self.md = self.idx.stored_rows()
        self.md.setflags(write=False)
        self.truth = self.md.astype(np.float64) @ qd64.T          # (rows, NQ): computed once, never written
        self.truth.setflags(write=False)

    def pos(self, far, label=""):
        """Twin rows of L rows; every one of them must be a row of the twin."""
        far = np.asarray(far, dtype=np.int64)
        p = np.searchsorted(self.rows, far)
        ok = (p < self.n) & (self.rows[np.minimum(p, self.n - 1)] == far)
        assert ok.all(), f"{label}: L rows outside the twin (filler, or a misread row number): {far[~ok][:8].tolist()}"
        return p


def _agree(twin, got, exp, truth, same, tol, label):
    """got = (scores, L rows) of the far index, exp = (scores, twin rows) of the twin or of a model on the twin's
    scores.  Same kernels: rows and bits are equal.  Otherwise near ties may swap under the f64 truth.  Always: every
    score within tol of the truth of the row it names."""
    gs, gr = np.asarray(got[0], dtype=np.float32), np.asarray(got[1], dtype=np.int64)
    es, er = np.asarray(exp[0], dtype=np.float32), np.asarray(exp[1], dtype=np.int64)
    assert gs.shape == es.shape and gr.shape == er.shape, (label, gs.shape, es.shape)
    p = twin.pos(gr, label)
    if same:
        assert np.array_equal(p, er), (label, "rows", np.flatnonzero(p != er)[:8].tolist(), gr[p != er][:8].tolist())
        assert np.array_equal(_bits(gs), _bits(es)), (label, "score bits", np.flatnonzero(_bits(gs) != _bits(es))[:8].tolist())
    else:
        assert_topk_parity(gs, p, es, er, truth, label=label)
    if gs.size:
        err = np.abs(gs.astype(np.float64) - truth[p])
        worst = int(np.argmax(err))
        assert err[worst] <= tol, f"{label}: |score - f64| = {err[worst]:.3g} at L row {gr[worst]} (bound {tol})"


def _planted_only(kth, tol, label):
    assert fr.planted_only(kth, tol), f"{label}: the reference's k-th best score {np.min(kth):.4g} does not clear the filler bound"


# ---- the fixture: one dtype resident at a time ------------------------------------------------------------------------
def _windows(lay):
    """[(p, L row of the window's first row, G row of it)]"""
    return [(p, lay.block_start(p) - WING, b * WIN) for b, p in enumerate(fr.POWERS)]


def _build(case):
    import torch
    from svs_amd import DeviceIndex, _native
    t0 = time.time()
    dtype, lay = fr.LAYOUTS[case]
    d, n = lay.dims[dtype], lay.n_rows()
    rows_b = n * lay.row_bytes
    # rows (+ the half shadow the screened case makes) + the f32 filler source + scratch: score rings, columns, lists
    need = rows_b + (rows_b // 2 if lay is fr.SHADOWED else 0) + (4 * n if dtype == "fp8" else 0) + lay.fill_rows * d * 4 + 6 * GIB
    free, total = _native.device_memory(0)
    assert free >= need + 4 * GIB, (f"{case}: the far index needs {need / GIB:.1f} GiB of HBM plus 4 GiB of slack, "
                                   f"{free / GIB:.1f} of {total / GIB:.1f} GiB are free")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(SEED_FILL + d)
    fill = torch.randn((lay.fill_rows, d), device=dev, dtype=torch.float32, generator=g)
    fill /= fill.norm(dim=1, keepdim=True)
    fill *= fr.FILL_SCALE
    planted = fr.planted_rows(dtype, d)
    pt = torch.from_numpy(planted).to(dev)
    L = DeviceIndex.empty(d, dtype=dtype)
    if dtype == "f32":
        L.set_screen(0)                     # before the first append: no shadow is ever asked for
    L.reserve(n)
    torch.cuda.synchronize()
    for a in lay.schedule():
        src = fill if a.kind == "fill" else pt[fr.block_of(a.source)]
        assert L.n == a.row0 and a.count <= src.shape[0]
        L.append_device(src.data_ptr(), a.count)
    torch.cuda.synchronize()
    assert L.shape == (n, d) and L.ld == d
    hbm = L.hbm_bytes
    assert hbm == rows_b + (4 * n if dtype == "fp8" else 0), (dtype, hbm)      # (f32: no shadow)
    # the windows twin's f32 rows: planted blocks from the host, their wings from the filler block on the device
    loc = lay.loc()
    gloc = np.concatenate([w0 + np.arange(WIN, dtype=np.int64) for _, w0, _ in _windows(lay)])
    planted_at = np.isin(gloc, loc)
    gsrc = np.empty((len(gloc), d), dtype=np.float32)
    gsrc[planted_at] = planted
    fsrc = np.array([lay.filler_source(int(r)) for r in gloc[~planted_at]], dtype=np.int64)
    gsrc[~planted_at] = fill[torch.from_numpy(fsrc).to(dev)].cpu().numpy()
    del fill, pt
    torch.cuda.empty_cache()
    qs = fr.queries(dtype, d=d)
    qd64 = _stored(qs, dtype).astype(np.float64)
    S = Twin(planted, loc, dtype, qd64)
    G = Twin(gsrc, gloc, dtype, qd64)
    print(f"\nfar index {case}: n = {n}, hbm_bytes = {hbm} ({hbm / GIB:.2f} GiB), built in {time.time() - t0:.1f} s")
    return SimpleNamespace(case=case, lay=lay, rows_b=rows_b, dtype=dtype, d=d, n=n, L=L, S=S, G=G, loc=loc, gloc=gloc, planted_at=planted_at, qs=qs,
                           t0=t0, peak=hbm, rng=np.random.default_rng(SEED_FILL + d))


@pytest.fixture(scope="module", params=CASES)
def far(request, gpu):
    import torch
    c = _build(request.param)
    yield c
    print(f"\nfar index {c.case}: peak hbm_bytes = {c.peak} ({c.peak / GIB:.2f} GiB), resident for {time.time() - c.t0:.1f} s")
    for idx in (c.L, c.S.idx, c.G.idx):
        idx.release()
    torch.cuda.empty_cache()


def test_tolerances_match():
    import test_far_rows_layout
    assert test_far_rows_layout.WIDEST_TOL == max(list(TOL_BATCH.values()) + list(TOL_SINGLE.values()) + list(TOL_GATHER.values()))


# ---- 1. the image --------------------------------------------------------------------------------------------------------
def test_image(far):
    c = far
    for p, w0, g0 in _windows(c.lay):
        a, b = c.L.stored_rows(w0, WIN), c.G.idx.stored_rows(g0, WIN)
        assert np.array_equal(_bits(a), _bits(b)), (p, "stored_rows", np.argwhere(_bits(a) != _bits(b))[:4].tolist())
        raw = c.L.stored_image("rows", w0, WIN)
        want, scales = ingest_model.image(c.G.src[g0:g0 + WIN], c.dtype, c.L.ld)
        assert np.array_equal(ingest_model.canon_image(raw, c.dtype), ingest_model.canon_image(want, c.dtype)), (p, "image")
        got_scales = None
        if c.dtype == "fp8":
            got_scales = c.L.stored_image("scales", w0, WIN)
            assert np.array_equal(_bits(got_scales), _bits(scales)), (p, "scales")
        assert np.array_equal(_bits(ingest_model.decode(raw, got_scales, c.dtype, c.d)), _bits(a)), (p, "decode")
    for i in (0, fr.MID - 1, fr.MID, fr.MID + 1, fr.BLOCK - 1):          # single-row reads, the straddling row among them
        for b in range(len(fr.POWERS)):
            j = b * fr.BLOCK + i
            assert np.array_equal(_bits(c.L.stored_rows(int(c.loc[j]), 1)), _bits(c.S.idx.stored_rows(j, 1))), (b, i)
    if c.dtype != "f32":
        with pytest.raises(NotImplementedError):
            c.L.stored_image("shadow", 0, 1)
    assert c.L.screen_stats()["shadow"] == 0


# ---- 2. whole-corpus scores ----------------------------------------------------------------------------------------------
def test_scores(far):
    c = far
    kernel = SINGLE_KERNEL[(c.dtype, c.d, 0)]
    filler = np.ones(c.n, dtype=bool)
    filler[c.loc] = False
    for j in (0, 1):
        full = c.L.scores(c.qs[j])
        rec = _launches()
        assert rec == [("gemv", c.n, 1), (kernel, c.n, 1)], rec
        assert full.shape == (c.n,)
        for twin in (c.S, c.G):
            ref = twin.idx.scores(c.qs[j])
            assert _names() == ["gemv", kernel]
            assert np.array_equal(_bits(full[twin.rows]), _bits(ref)), np.flatnonzero(_bits(full[twin.rows]) != _bits(ref))[:8]
            err = np.abs(full[twin.rows].astype(np.float64) - twin.truth[:, j])
            assert err.max() <= TOL_SINGLE[c.dtype], (j, err.max(), int(twin.rows[np.argmax(err)]))
        worst = float(np.abs(full[filler]).max())
        assert worst <= fr.FILL_BOUND, f"a filler row scores {worst}"
        assert np.sort(full[c.loc])[-fr.K] > fr.FILL_BOUND


# ---- 3. top-k routes -----------------------------------------------------------------------------------------------------
def test_search(far):
    c = far
    kernel = SINGLE_KERNEL[(c.dtype, c.d, 0)]
    for j in range(3):
        for k in (1, fr.K):
            _planted_only(np.sort(c.S.truth[:, j])[-k], TOL_SINGLE[c.dtype], f"search q{j} k{k}")
            got = _pairs(c.L.search(c.qs[j], k))
            rec = _launches()
            assert (kernel, c.n, 1) in rec, rec
            exp = _pairs(c.S.idx.search(c.qs[j], k))
            _agree(c.S, got, exp, c.S.truth[:, j], _names(rec) == _names(), TOL_SINGLE[c.dtype], f"search q{j} k{k}")


@pytest.mark.parametrize("nq", [16, 64, 256])
def test_search_batch(far, nq):
    c = far
    tol = TOL_BATCH[c.dtype]
    _planted_only(np.sort(c.S.truth[:, :nq], axis=0)[-fr.K], tol, f"batch {nq}")
    s, r = c.L.search_batch(c.qs[:nq], fr.K)
    rec = _launches()
    main = [x for x in rec if x[1] == c.n]
    assert main and main[0][0] == BATCH_KERNEL[c.dtype][nq], rec
    assert rec[0][1] < c.n, f"a fused search starts with its threshold pass over a sample: {rec}"
    es, er = c.S.idx.search_batch(c.qs[:nq], fr.K)
    same = _names(rec) == _names()
    assert s.shape == (nq, fr.K)
    for j in range(nq):
        _agree(c.S, (s[j], r[j]), (es[j], er[j]), c.S.truth[:, j], same, tol, f"batch {nq} q{j}")


def test_device_entries(far):
    """search_device and search_device_ahead; the run-ahead calls as a backlog of 4 behind a pending event.  Passes are
    shared only where a single-query pass reads half rows (pass_share.h): an f16 index, where one pass must serve all
    four, and an f32 index with a shadow (test_screened_f32).  An fp8 index and an f32 index without a shadow run four
    passes of their own, and their counters stay zero."""
    import torch
    import test_shared_pass_gpu as sp
    c = far
    dev = torch.device("cuda:0")
    q_t = torch.from_numpy(c.qs[:5]).to(dev)
    for j in range(5):
        _planted_only(np.sort(c.S.truth[:, j])[-fr.K], TOL_SINGLE[c.dtype], f"device q{j}")
    exp = sp.plain(torch, dev, c.L, q_t, fr.K)
    rec = _launches()
    for j in range(5):
        ref = _pairs(c.S.idx.search(c.qs[j], fr.K))
        _agree(c.S, (exp[0][j].view(np.float32), exp[1][j]), ref, c.S.truth[:, j], _names(rec) == _names(), TOL_SINGLE[c.dtype],
               f"search_device q{j}")
    st, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    sp.same(sp.warm_up(torch, dev, c.L, q_t[0], fr.K, st), (exp[0][:1], exp[1][:1]), "warm-up")
    got = sp.backlog(torch, dev, c.L, [(q_t[1 + i], fr.K) for i in range(4)], st, feeder)
    sp.same(got, (exp[0][1:], exp[1][1:]), "backlog of 4")
    stats = sp.shared_stats(c.L)
    print(f"{c.case}: shared passes {stats}")
    if c.dtype == "f16":
        assert stats == sp.counters_of(sp.claim_model(sp.backlog_model(4), sp.SHARE_DEFAULT)) and stats["claimed"] == 3, stats
    else:
        assert stats == {"shared_passes": 0, "claimed": 0, "empty_passes": 0}, stats


# ---- 4. gather -----------------------------------------------------------------------------------------------------------
def _gather_kernels(c):
    case = [x for x in GATHER_CASES if x[0] == c.dtype and x[1] == c.d][0]
    return case[3], case[4]


def test_search_within(far):
    c = far
    one, many = _gather_kernels(c)
    perm = c.rng.permutation(c.G.n)
    m = len(perm)
    assert m == fr.BLOCK * len(fr.POWERS) + 2004 and not c.planted_at.all()
    for k in (fr.K, m):
        for nq in (1, 5):
            if nq == 1:
                s, r = (x[None, :] for x in _pairs(c.L.search_within(c.qs[0], k, c.gloc[perm])))
            else:
                s, r = c.L.search_batch_within(c.qs[:nq], k, c.gloc[perm])
            rec = _launches()
            assert [x for x in rec if x[0].startswith("gather_scores_kernel")] == [(one if nq == 1 else many, m, nq)], rec
            assert all(x[1] != c.n for x in rec), f"something ran over the whole corpus: {rec}"
            es, er = c.G.idx.search_batch_within(c.qs[:nq], k, perm)
            same = _names(rec) == _names()
            assert same and s.shape == (nq, k)
            for j in range(nq):
                _agree(c.G, (s[j], r[j]), (es[j], er[j]), c.G.truth[:, j], same, TOL_GATHER[c.dtype], f"within k{k} nq{nq} q{j}")


def test_search_segments(far):
    c = far
    lists = [g0 + c.rng.permutation(WIN) for _, _, g0 in _windows(c.lay)]
    got = c.L.search_segments(c.qs[:len(lists)], fr.K, [c.gloc[x] for x in lists])
    rec = _launches()
    assert rec and all(x[1] != c.n for x in rec), rec
    exp = c.G.idx.search_segments(c.qs[:len(lists)], fr.K, lists)
    same = _names(rec) == _names()
    assert same, (rec, _launches())
    for s, ((gs, gr), (es, er)) in enumerate(zip(got, exp)):
        assert len(gs) == fr.K
        _agree(c.G, (gs, gr), (es, er), c.G.truth[:, s], same, TOL_GATHER[c.dtype], f"segment {s}")


def test_neighbors(far):
    c = far
    sel = np.arange(0, c.S.n, 7)
    md64 = c.S.md.astype(np.float64)
    truth = md64 @ md64[sel].T                       # (2052, 294)
    truth[sel, np.arange(len(sel))] = -np.inf        # the row itself is excluded
    tol = TOL_BATCH[c.dtype]
    _planted_only(np.sort(truth, axis=0)[-10], tol, "neighbors")
    s, r = c.L.neighbors(c.loc[sel], 10)
    rec = _launches()
    es, er = c.S.idx.neighbors(sel, 10)
    same = _names(rec) == _names()
    assert s.shape == (len(sel), 10)
    for j in range(len(sel)):
        assert c.loc[sel[j]] not in r[j]
        _agree(c.S, (s[j], r[j]), (es[j], er[j]), truth[:, j], same, tol, f"neighbors of planted row {sel[j]}")


def test_search_diverse(far):
    c = far
    fetch, take, lam = 64, 10, 0.5
    nq = 4
    _planted_only(np.sort(c.S.truth[:, :nq], axis=0)[-fetch], TOL_SINGLE[c.dtype], "diverse")
    s, r, red = c.L.search_batch_diverse(c.qs[:nq], take, fetch, lam)
    es, er, ered = c.S.idx.search_batch_diverse(c.qs[:nq], take, fetch, lam)
    assert s.shape == (nq, take)
    cand_s, cand_r = c.L.search_batch(c.qs[:nq], fetch)      # the candidates and their score bits: the same batch's search
    for j in range(nq):
        cs, cr = cand_s[j], cand_r[j]
        cp = c.S.pos(cr, f"diverse q{j} candidates")
        assert np.abs(cs.astype(np.float64) - c.S.truth[cp, j]).max() <= TOL_BATCH[c.dtype], j
        picks = [int(np.flatnonzero(cr == x)[0]) for x in r[j]]
        assert np.array_equal(_bits(s[j]), _bits(cs[picks])), j
        near = diverse_model.valid_picks(cs, c.S.md[cp], picks, red[j], lam, c.d)
        if near == 0:
            assert np.array_equal(c.S.pos(r[j]), er[j]), (j, r[j], er[j])


# ---- 5. labels -----------------------------------------------------------------------------------------------------------
def test_labels(far):
    c = far
    L, G = c.L, c.G.idx
    hbm0 = L.hbm_bytes
    glab = np.zeros(c.G.n, dtype=np.uint32)
    for b, (p, w0, g0) in enumerate(_windows(c.lay)):
        lab = np.full(fr.BLOCK, b + 1, dtype=np.uint32)
        L.set_labels(lab, row0=w0 + WING)
        G.set_labels(lab, row0=g0 + WING)
        glab[g0 + WING:g0 + WING + fr.BLOCK] = b + 1
    assert L.hbm_bytes > hbm0
    c.peak = max(c.peak, L.hbm_bytes)
    for b, (p, w0, g0) in enumerate(_windows(c.lay)):
        got = L.labels(w0, WIN)
        assert np.array_equal(got, glab[g0:g0 + WIN]) and np.array_equal(G.labels(g0, WIN), got), p
        assert got[WING - 1] == 0 and got[WING] == b + 1 and got[WING + fr.BLOCK - 1] == b + 1 and got[WING + fr.BLOCK] == 0
    q, truth = c.qs[0], c.G.truth[:, 0]
    # search_labeled: one block at a time, then all six
    for labels, matched_want in [({b + 1}, fr.BLOCK) for b in range(6)] + [(set(range(1, 7)), 6 * fr.BLOCK)]:
        got, matched = L.search_labeled(q, fr.K, labels)
        rec = _launches()
        exp, ematched = G.search_labeled(q, fr.K, labels)
        assert matched == ematched == matched_want, (labels, matched, ematched)
        _agree(c.G, _pairs(got), _pairs(exp), truth, _names(rec) == _names(), TOL_GATHER[c.dtype], f"labeled {sorted(labels)}")
    # search_by_label: label 0 is every filler row of the 64 GiB
    for cut in (None, fr.ABOVE_CUT):
        got = L.search_by_label(q, list(range(7)), min_score=cut)
        rec = _launches()
        exp = G.search_by_label(q, list(range(1, 7)), min_score=cut)
        same = _names(rec) == _names()
        zero = [x for x in got if x[0] == 0]
        if cut is None:
            assert len(zero) == 1 and zero[0][3] == c.n - 6 * fr.BLOCK and abs(zero[0][1]) <= fr.FILL_BOUND, zero
        else:
            assert zero == [], zero                       # no filler row reaches the cut-off
        rest = [x for x in got if x[0] != 0]
        assert [x[0] for x in rest] == [x[0] for x in exp] and [x[3] for x in rest] == [x[3] for x in exp], (rest, exp)
        if cut is None:
            assert [x[3] for x in rest] == [fr.BLOCK] * 6
        _agree(c.G, (np.array([x[1] for x in rest], dtype=np.float32), np.array([x[2] for x in rest], dtype=np.int64)),
               (np.array([x[1] for x in exp], dtype=np.float32), np.array([x[2] for x in exp], dtype=np.int64)),
               truth, same, TOL_GATHER[c.dtype], f"by_label cut {cut}")
    # label_sums over each window: the definition replayed on the twin's stored rows, bit for bit
    for b, (p, w0, g0) in enumerate(_windows(c.lay)):
        labels = [b + 1, 0, 99]
        sums, counts = L.label_sums(labels, row0=w0, nrows=WIN)
        esums, ecounts = label_sums_model.replay(c.G.md[g0:g0 + WIN], glab[g0:g0 + WIN], None, labels)
        assert counts.tolist() == ecounts.tolist() == [fr.BLOCK, 2 * WING, 0], (p, counts)
        assert label_sums_model.same_bits(sums, esums), (p, np.argwhere(sums != esums)[:4].tolist())
    # assign: 65 vectors, each the normalised sum of the block's rows i with i % 65 == j; labels written in place
    ids = np.arange(fr.BLOCK) % 65
    for b, p in enumerate(fr.POWERS):
        blk = c.S.src[fr.block_of(p)].astype(np.float64)
        v = np.stack([blk[ids == j].sum(axis=0) for j in range(65)])
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        vst = _stored(v, c.dtype)
        R = c.S.md[fr.block_of(p)]
        # teeth, on the reference first: at most 1 % of the rows have a second position within tol of the best
        _, tol = assign_model.tolerances(R, vst, c.d)
        assert int((assign_model.margins(R, vst) <= tol).sum()) <= 0.01 * fr.BLOCK
        new = np.arange(100, 165, dtype=np.uint32)
        best, sc, counts = L.assign(v, labels=new, row0=c.lay.block_start(p), nrows=fr.BLOCK)
        assert _names() == ["assign_rows_kernel"]
        near = assign_model.valid_assignment(R, vst, best, sc, counts, d=c.d)
        assert near <= 0.01 * fr.BLOCK and np.array_equal(best, ids), (p, near)
        back = L.labels(c.lay.block_start(p) - 2, fr.BLOCK + 4)
        assert back.tolist() == [0, 0] + new[best].tolist() + [0, 0], p


# ---- 6. columns ----------------------------------------------------------------------------------------------------------
def _set_columns(c):
    """Column 1: the window's p; column 2: a number of its own, odd for every other row; column 3: 97 group values."""
    cols = {1: np.zeros(c.G.n, dtype=np.uint32), 2: np.zeros(c.G.n, dtype=np.uint32), 3: np.zeros(c.G.n, dtype=np.uint32)}
    for p, w0, g0 in _windows(c.lay):
        cols[1][g0:g0 + WIN] = p
        cols[2][g0:g0 + WIN] = g0 + np.arange(WIN) + 1
        cols[3][g0:g0 + WIN] = 1 + (g0 + np.arange(WIN)) % 97
        for col, v in cols.items():
            c.L.set_column(col, v[g0:g0 + WIN], row0=w0)
            c.G.idx.set_column(col, v[g0:g0 + WIN], row0=g0)
    c.peak = max(c.peak, c.L.hbm_bytes)
    return cols


def _collapsed_rows(out, j):
    s, r, v, counts, groups = out[:5]
    n = int(counts[j])
    return s[j, :n], r[j, :n], v[j, :n], int(groups[j])


def test_columns(far):
    c = far
    L, G = c.L, c.G.idx
    cols = _set_columns(c)
    for p, w0, g0 in _windows(c.lay):
        for col in cols:
            got = L.column(col, w0 - 1, WIN + 2)
            assert got[0] == 0 and got[-1] == 0 and np.array_equal(got[1:-1], cols[col][g0:g0 + WIN]), (p, col)
    only36 = [(1, "in", [36])]
    odd = [(2, "any_bits", 1)]
    n_odd = int((cols[2] & 1).sum())
    assert L.count_where(only36) == G.count_where(only36) == WIN
    assert L.count_where(odd) == G.count_where(odd) == n_odd
    assert L.count_where([(1, "not in", [31, 32, 33, 34, 35, 36])]) == c.n - c.G.n
    q, truth = c.qs[0], c.G.truth[:, 0]
    for where, k, matched_want in ((only36, fr.K, WIN), (only36, WIN, WIN), (odd, fr.K, n_odd)):
        got, matched = L.search_where(q, k, where)
        rec = _launches()
        exp, ematched = G.search_where(q, k, where)
        assert matched == ematched == matched_want
        _agree(c.G, _pairs(got), _pairs(exp), truth, _names(rec) == _names(), TOL_GATHER[c.dtype], f"where {where} k{k}")
    # collapsed searches: the numpy models fed with the twin's scores.  A filler row outside the windows carries 0: under
    # zero="single" each is a group of its own (and scores below the bound), under "group" they are one group together.
    nq, k = 2, 50
    gs = [G.scores(c.qs[j]) for j in range(3)]
    scores_kernel = _names()
    outside = c.n - c.G.n
    tol = TOL_SINGLE[c.dtype]
    for zero, extra in (("single", outside), ("group", 1)):
        out = L.search_batch_collapsed(c.qs[:nq], k, 3, zero)
        same = _names()[:2] == scores_kernel
        for j in range(nq):
            es, er, ev, eg = collapse_model.collapsed(gs[j], cols[3], None, zero == "single", k)
            _planted_only(es[-1], tol, f"collapsed {zero} q{j}")
            s, r, v, groups = _collapsed_rows(out, j)
            assert groups == eg + extra and np.array_equal(v, ev), (zero, j, groups, eg)
            _agree(c.G, (s, r), (es, er), c.G.truth[:, j], same, tol, f"collapsed {zero} q{j}")
    # ... under a predicate (the gather family's kernels score the rows in scope)
    out = L.search_batch_collapsed_where(c.qs[:nq], k, odd, 3, "single")
    rec = _launches()
    ref = G.search_batch_collapsed_where(c.qs[:nq], k, odd, 3, "single")
    same = _names(rec) == _names()
    assert out[5] == ref[5] == n_odd
    for j in range(nq):
        es, er, ev, eg, em = collapse_scope_model.collapsed_scoped(gs[j], cols[3], None, (cols[2] & 1) == 1, True, k)
        s, r, v, groups = _collapsed_rows(out, j)
        rs, rr, rv, rgroups = _collapsed_rows(ref, j)
        assert groups == rgroups == eg and em == n_odd and np.array_equal(v, ev) and np.array_equal(c.G.pos(r), er), (j, groups, eg)
        _agree(c.G, (s, r), (rs, rr), c.G.truth[:, j], same, TOL_GATHER[c.dtype], f"collapsed_where q{j}")
    # ... and over a row list
    lst = c.rng.permutation(c.G.n)[:3000]
    in_list = np.zeros(c.G.n, dtype=bool)
    in_list[lst] = True
    out = L.search_batch_collapsed_within(c.qs[:nq], k, c.gloc[lst], 3, "single")
    rec = _launches()
    ref = G.search_batch_collapsed_within(c.qs[:nq], k, lst, 3, "single")
    same = _names(rec) == _names()
    assert out[5] == ref[5] == 3000
    for j in range(nq):
        es, er, ev, eg, em = collapse_scope_model.collapsed_scoped(gs[j], cols[3], None, in_list, True, k)
        s, r, v, groups = _collapsed_rows(out, j)
        rs, rr, rv, rgroups = _collapsed_rows(ref, j)
        assert groups == rgroups == eg and np.array_equal(v, ev) and np.array_equal(c.G.pos(r), er), (j, groups, eg)
        _agree(c.G, (s, r), (rs, rr), c.G.truth[:, j], same, TOL_GATHER[c.dtype], f"collapsed_within q{j}")
    # ... and group-combined: parents ranked by their best chunk per vector
    # (max takes the signed weights.  A planted group's per-vector bests are all positive, so under min a negative weight
    #  turns every planted group negative while the filler rows, groups of their own, sit at about 0, and under sum the
    #  50th group falls inside the filler bound: the reference-first condition rejects both, and they take POSITIVE)
    for op, w, kk in (("max", SIGNED, k), ("sum", POSITIVE, k), ("min", POSITIVE, 10)):
        es, er, ev, eg = collapsed_combined_model.collapsed_combined(gs, w, op, cols[3], None, True, kk)
        fill = fr.FILL_BOUND * float({"max": np.abs(w).max(), "min": np.abs(w).min(), "sum": np.abs(w).sum()}[op])
        assert es[-1] > fill + 3 * tol, (op, es[-1], fill)
        s, r, v, counts, groups = L.search_batch_collapsed_combined(c.qs[None, :3], kk, 3, op, w[None, :], "single")
        n_out = int(counts[0])
        assert n_out == kk and int(groups[0]) == eg + outside, (op, n_out, groups[0], eg)
        p = c.G.pos(r[0, :n_out], f"collapsed_combined {op}")
        assert np.array_equal(p, er) and np.array_equal(v[0, :n_out], ev), (op, p[:8], er[:8])
        assert np.array_equal(_bits(s[0, :n_out]), _bits(es)), (op, np.flatnonzero(_bits(s[0, :n_out]) != _bits(es))[:8])


# ---- 7. threshold and combination ----------------------------------------------------------------------------------------
def test_search_above(far):
    c = far
    for j in range(fr.ABOVE_QUERIES):
        ref = c.S.idx.scores(c.qs[j])
        er, es, etotal = above_model.above(ref, None, fr.ABOVE_CUT, c.S.n)
        assert 50 <= etotal < c.S.n
        got, total = c.L.search_above(c.qs[j], fr.ABOVE_CUT, c.S.n)
        assert total == etotal == len(got), (j, total, etotal)          # the members are the twin's: no filler row, none missing
        _agree(c.S, _pairs(got), (es, er), c.S.truth[:, j], True, TOL_SINGLE[c.dtype], f"above q{j}")
        assert c.L.search_above(c.qs[j], fr.ABOVE_CUT, 0) == ([], etotal)


def test_search_combined(far):
    from svs_amd import _native
    c = far
    v = c.qs[:3]
    ss = [c.S.idx.scores(x) for x in v]
    fused = [x[2] for x in COMBINE_SHAPES if x[0] == c.dtype and x[1] == c.d][0]
    assert fused is not None
    # the combined vector of all 22M rows on both routes: at the planted rows, the model on the twin's scores, bit for bit
    for op in OPS:
        exp = combine_model.combine(ss, MIXED[:3], op)
        for route in (FUSED, PASSES):
            out = np.empty(c.n, dtype=np.float32)
            w = np.ascontiguousarray(MIXED[:3])
            rc = c.L._lib.svs_internal_combined_scores(c.L._handle(), np.ascontiguousarray(v).ctypes.data, 3, c.d, w.ctypes.data,
                                                       OPS[op], route, out.ctypes.data, out.size)
            assert rc == 0, _native.last_error()
            names = _names()
            assert (names == [fused]) if route == FUSED else (names.count("gemv") == 3 and names[-1] == "combine_scores_kernel"), names
            bad = np.flatnonzero(_bits(out[c.loc]) != _bits(exp))
            assert bad.size == 0, (op, route, bad[:5], out[c.loc][bad[:5]], exp[bad[:5]])
    # the public entry (the fused kernel for m = 3): planted-only answers
    for op, w, k in (("max", MIXED[:3], fr.K), ("sum", MIXED[:3], fr.K), ("min", SIGNED, 10)):
        eb, er, ecount = combine_model.top_k(ss, w, op, k)
        fill = fr.FILL_BOUND * float({"max": np.abs(w).max(), "min": np.abs(w).min(), "sum": np.abs(w).sum()}[op])
        assert eb[:ecount].view(np.float32)[-1] > fill + 3 * TOL_SINGLE[c.dtype], (op, eb[:ecount].view(np.float32)[-1], fill)
        s, r, count = c.L.search_batch_combined(v[None], k, op, w[None, :])
        assert _launches() == [(fused, c.n, 3)], _launches()
        assert count == ecount == k
        assert np.array_equal(c.S.pos(r[0], f"combined {op}"), er) and np.array_equal(_bits(s[0]), eb), op


# ---- 8. screened f32 (last but one) --------------------------------------------------------------------------------------
def test_screened_f32(far):
    """Only f32 rows of whole 512-float steps get a half shadow (shadow_eligible in svs_amd.hip), so the 3,072-byte
    indices have none -- pinned here -- and the screened route runs on the second f32 geometry (d = 2048): 64 GiB of rows
    and 32 GiB of halves, whose offsets pass 2^32 bytes, 2^32 halves and 2^31 chunks inside planted blocks
    (test_far_rows_layout.py::test_the_shadowed_geometry).  The shadow stays on for the compaction case."""
    import torch
    import test_shared_pass_gpu as sp
    from test_screen_gpu import FORCE, OFF, screen_kernels
    c = far
    L = c.L
    before_hbm = L.hbm_bytes
    L.set_screen(1)
    if c.lay is not fr.SHADOWED:
        assert L.screen_stats()["shadow"] == 0 and L.hbm_bytes == before_hbm
        with pytest.raises(NotImplementedError):
            L.stored_image("shadow", 0, 1)
        L.set_screen(0)
        return
    assert L.screen_stats()["shadow"] == 1
    assert L.hbm_bytes == before_hbm + c.rows_b // 2
    c.peak = max(c.peak, L.hbm_bytes)
    for p, w0, g0 in _windows(c.lay):
        assert np.array_equal(L.stored_image("shadow", w0, WIN), ingest_model.half_bits(c.G.src[g0:g0 + WIN])), p
    for j in range(3):
        _planted_only(np.sort(c.S.truth[:, j])[-fr.K], TOL_SINGLE["f32"], f"screened q{j}")
        L.set_variant(OFF)
        s0, r0 = L.search_batch(c.qs[j][None, :], fr.K)
        assert not [x for x in _names() if x.startswith("gemv_f16") or x.startswith("rescore")], _names()
        L.set_variant(FORCE)
        before = L.screen_stats()
        s1, r1 = L.search_batch(c.qs[j][None, :], fr.K)
        rec = _launches()
        after = L.screen_stats()
        assert _names(rec) == list(screen_kernels(c.d)) and all(x[1:] == (c.n, 1) for x in rec), rec
        # the candidate-list branch, not the exact whole-corpus fallback
        assert after["screened"] - before["screened"] == 1 and after["fallback"] == before["fallback"], (before, after)
        assert np.array_equal(r0, r1) and np.array_equal(_bits(s0), _bits(s1)), j
        _agree(c.S, (s1[0], r1[0]), _pairs(c.S.idx.search(c.qs[j], fr.K)), c.S.truth[:, j], True, TOL_SINGLE["f32"], f"screened q{j}")
    # the run-ahead entry on the shadow: one shared pass serves a backlog of 4
    dev = torch.device("cuda:0")
    q_t = torch.from_numpy(c.qs[:5]).to(dev)
    exp = sp.plain(torch, dev, L, q_t, fr.K)
    st, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    base = sp.shared_stats(L)
    sp.same(sp.warm_up(torch, dev, L, q_t[0], fr.K, st), (exp[0][:1], exp[1][:1]), "warm-up")
    got = sp.backlog(torch, dev, L, [(q_t[1 + i], fr.K) for i in range(4)], st, feeder)
    sp.same(got, (exp[0][1:], exp[1][1:]), "screened backlog of 4")
    stats = sp.shared_stats(L)
    print(f"{c.case} screened: shared passes {base} -> {stats}")
    assert stats["claimed"] - base["claimed"] == 3, (base, stats)
    for j in range(5):
        _agree(c.S, (exp[0][j].view(np.float32), exp[1][j]), _pairs(c.S.idx.search(c.qs[j], fr.K)), c.S.truth[:, j], True,
               TOL_SINGLE["f32"], f"screened search_device q{j}")
    L.set_variant(0)


# ---- 9. compaction (last: it mutates) ------------------------------------------------------------------------------------
def test_compaction(far):
    c = far
    L, G = c.L, c.G.idx
    first, last = c.lay.spans()[0], c.lay.spans()[-1]
    dead = np.array(sorted([5, 1000, first.row_first - 50]                                  # filler below block 31
                           + [int(c.loc[b * fr.BLOCK + 100 + b]) for b in range(6)]         # a planted row of every block
                           + [last.row_last + 21, c.n - 2]), dtype=np.int64)                # filler above block 36
    in_g = np.isin(dead, c.gloc)
    assert in_g.sum() == 8
    gdead = c.G.pos(dead[in_g])
    L.mask_rows(dead)
    G.mask_rows(gdead)
    t0 = time.time()
    stats = []
    faulthandler.dump_traceback_later(COMPACT_LIMIT_S, exit=True)      # a stuck 64 GiB move ends the process itself
    try:
        row_map = L.compact(stats=stats)
    finally:
        faulthandler.cancel_dump_traceback_later()
    print(f"{c.case}: compact() of {c.n} rows took {time.time() - t0:.2f} s; direct steps, bounce steps, rows moved, bytes moved = {stats}")
    n_new = c.n - len(dead)
    assert L.screen_stats()["shadow"] == (1 if c.lay is fr.SHADOWED else 0)
    assert L.n == n_new and L.n_masked == 0
    assert np.array_equal(row_map, np.delete(np.arange(c.n, dtype=np.int64), dead))
    new_of = lambda rows: np.asarray(rows, dtype=np.int64) - np.searchsorted(dead, rows)   # (for rows that are alive)
    alive = np.ones(c.G.n, dtype=bool)
    alive[gdead] = False
    for p, w0, g0 in _windows(c.lay):
        keep = alive[g0:g0 + WIN]
        at = int(new_of([w0])[0])
        cnt = int(keep.sum())
        a = L.stored_rows(at, cnt)
        assert np.array_equal(_bits(a), _bits(c.G.md[g0:g0 + WIN][keep])), (p, "stored_rows after compact")
        want, scales = ingest_model.image(c.G.src[g0:g0 + WIN][keep], c.dtype, L.ld)
        assert np.array_equal(ingest_model.canon_image(L.stored_image("rows", at, cnt), c.dtype), ingest_model.canon_image(want, c.dtype)), p
        if c.dtype == "fp8":
            assert np.array_equal(_bits(L.stored_image("scales", at, cnt)), _bits(scales)), p
        if c.lay is fr.SHADOWED:                          # compact.h's shadow_chunks moves
            assert np.array_equal(L.stored_image("shadow", at, cnt), ingest_model.half_bits(c.G.src[g0:g0 + WIN][keep])), p
    # searches after the move agree with the twin under the same mask (rows come back in the new numbering)
    gl = np.flatnonzero(alive)
    for j in range(2):
        live_truth = np.where(alive, c.G.truth[:, j], -np.inf)
        _planted_only(np.sort(live_truth)[-fr.K], TOL_SINGLE[c.dtype], f"compacted search q{j}")
        gs, gr = _pairs(L.search(c.qs[j], fr.K))
        rec = _launches()
        exp = _pairs(G.search(c.qs[j], fr.K))
        _agree(c.G, (gs, row_map[gr]), exp, c.G.truth[:, j], _names(rec) == _names(), TOL_SINGLE[c.dtype], f"compacted search q{j}")
        perm = c.rng.permutation(gl)
        s, r = L.search_batch_within(c.qs[j][None, :], len(perm), new_of(c.gloc[perm]))
        rec = _launches()
        es, er = G.search_batch_within(c.qs[j][None, :], len(perm), perm)
        assert s.shape == (1, len(perm))
        _agree(c.G, (s[0], row_map[r[0]]), (es[0], er[0]), c.G.truth[:, j], _names(rec) == _names(), TOL_GATHER[c.dtype],
               f"compacted within q{j}")
