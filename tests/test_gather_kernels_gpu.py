"""GPU: every score kernel of the filtered search (gather_scores_kernel<DT, T, NC, U, G>, svs_amd/csrc/gather.h), each at
the shapes of tests/gather_kernel_table.py, through DeviceIndex.search_within (a lone query: G = 1) and
search_batch_within (a batch: G = 4) with k = the length of the list, so that every score of the list comes back.

Every call asserts that the gather records of svs_internal_last_launches read exactly [(kernel, m, nq)] -- the table's
G = 1 name for one query, its G = 4 name for a batch -- and that nothing scored the whole corpus.  The list is always a
scattered subset of a larger corpus (about a third of its rows, rows 0 and n - 1 among them), passed ascending and
shuffled: a kernel that indexes the corpus, or the fp8 row scales, by list position cannot pass.

For every table row:
  a. f64 closeness on what the index really stores (stored_rows, stored_query), at the bounds of
     test_search_within_gpu.py, at m = 2 B + W + 1 (several workgroups, a partial last wave and a partial group of rows),
     m = 1 and m = W - 1 (every clamped lane re-reads list entry m - 1), for one query and for five (a full group of four
     and a group of one); then rows whose norms span 1e-2 .. 1e2, relative to |row| |q|; for one geometry per dtype
     also m = 2 B and 2 B + 1 (the last wave exactly full, and holding one row), bit-equal to a longer list's scores;
  b. one non-zero per listed row: the row at list position p holds one value, at column p mod d; its score is that
     value times the query's, to the bit (f32, f16);
  c. one row copied n times scores with one bit pattern wherever it is listed;
  d. a query's rows and score bits do not depend on the batch it was scored in (gather.h: "a query's scores are
     bit-identical whatever batch or group it was scored in");
  e. non-finite values in the first and the last column of a row (f32, f16)."""
import zlib

import numpy as np
import pytest

from gather_kernel_table import CASES, case_id, choose_ld, geometry, rows_per_block, rows_per_wave
from oracle import svs_oracle as oracle

pytestmark = pytest.mark.gpu

# |score - f64| on unit-norm rows and queries: test_search_within_gpu.py, test_single_kernels_gpu.py
TOL = {"f32": 2e-6, "f16": 2e-6, "fp8": 5e-6}
BATCH = 5                  # queries of a batch: one full group of four, and a group of one (gq < G)
BLOCK_ELEMS = 1 << 24      # one-hot corpora are uploaded and read back in blocks of at most 64 MiB


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _unit(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _open(m, dtype):
    from svs_amd import DeviceIndex
    idx = DeviceIndex(m, dtype=dtype)
    assert idx.ld == choose_ld(m.shape[1], dtype), (dtype, m.shape[1], idx.ld)
    return idx


def _edge_sizes(kernel):
    w, b = rows_per_wave(kernel), rows_per_block(kernel)
    return sorted({2 * b + w + 1, 1, max(w - 1, 1)}, reverse=True)


def _scattered(rng, n, m):
    """m of n rows, ascending: rows 0 and n - 1 and a random choice of the others (one row: a middle one)."""
    assert 3 * m <= n + 2
    if m == 1:
        return np.array([n // 2], dtype=np.int64)
    inner = rng.choice(np.arange(1, n - 1), m - 2, replace=False)
    return np.sort(np.concatenate([[0], inner, [n - 1]])).astype(np.int64)


def _orders(rng, rows):
    return [("ascending", rows)] + ([("shuffled", rng.permutation(rows))] if len(rows) > 1 else [])


def _search_all(idx, qs, rows, case):
    """Top-m of the m listed rows as the library returns it, (scores (nq, m) f32, rows (nq, m) i64), having asserted
    which kernel scored them.  One query goes through search_within, several through search_batch_within."""
    from svs_amd import _native
    m, nq = len(rows), len(qs)
    if nq == 1:
        got = idx.search_within(qs[0], m, rows)
        s = np.array([[a for a, _ in got]], dtype=np.float32).reshape(1, -1)      # (float(f32) widens exactly)
        r = np.array([[b for _, b in got]], dtype=np.int64).reshape(1, -1)
    else:
        s, r = idx.search_batch_within(qs, m, rows)
    launches = _native.last_launches()
    gathers = [rec for rec in launches if rec[0].startswith("gather_scores_kernel")]
    want = [(case[3] if nq == 1 else case[4], m, nq)]
    assert gathers == want, f"{case_id(case)} ld={idx.ld} n={idx.n}: launched {launches}, the table says {want}"
    assert m != idx.n and all(rec[1] != idx.n for rec in launches), f"{case_id(case)}: something ran over the whole corpus: {launches}"
    assert s.shape == (nq, m) and r.shape == (nq, m), (case_id(case), s.shape, r.shape, m, nq)
    return s, r


def _within(idx, qs, rows, case):
    """scores[j][p] = the score of row rows[p] under query j: the library's answer scattered to list positions."""
    s, r = _search_all(idx, qs, rows, case)
    m, nq = len(rows), len(qs)
    where = np.full(idx.n, -1, dtype=np.int64)
    where[rows] = np.arange(m)
    pos = where[r]
    assert np.array_equal(np.sort(pos, axis=1), np.broadcast_to(np.arange(m), (nq, m))), \
        f"{case_id(case)} m={m} nq={nq}: the returned rows are not the listed rows, each once"
    out = np.empty((nq, m), dtype=np.float32)
    np.put_along_axis(out, pos, s, axis=1)
    return out


def _stored(idx, m, qs):
    """Rows and queries as the kernels see them."""
    md = m if idx.dtype == "f32" else idx.stored_rows()
    return md, np.stack([idx.stored_query(q) for q in qs])


def _check_f64(rng, m, qs, sizes, case, relative=False):
    """Every list size, ascending and shuffled, one query and a batch, against the f64 product of the stored values."""
    dtype = case[0]
    idx = _open(m, dtype)
    try:
        md, qd = _stored(idx, m, qs)
        truth = md.astype(np.float64) @ qd.astype(np.float64).T                    # (n, nq), computed once
        if relative:
            truth_scale = np.linalg.norm(md.astype(np.float64), axis=1)[:, None] * np.linalg.norm(qd.astype(np.float64), axis=1)[None, :]
        for size in sizes:
            for order, rows in _orders(rng, _scattered(rng, idx.n, size)):
                for batch in (qs[:1], qs):
                    got = _within(idx, batch, rows, case)
                    nq = len(batch)
                    err = np.abs(got.astype(np.float64) - truth[rows, :nq].T)
                    if relative:
                        err /= truth_scale[rows, :nq].T
                    j, p = np.unravel_index(np.argmax(err), err.shape)
                    worst = float(err[j, p])
                    print(f"{case_id(case)} m={size} {order} nq={nq}: max |score - f64| {'/ (|row| |q|) ' if relative else ''}= {worst:.3g}")
                    assert np.all(err <= TOL[dtype]), \
                        (f"{case_id(case)} n={idx.n} m={size} {order} nq={nq}: max |score - f64| {'/ (|row| |q|) ' if relative else ''}"
                         f"= {worst:.3g} at list position {p} (row {rows[p]}), query {j}")
    finally:
        idx.release()


# ---- a. edges: several workgroups and a partial last group; one row; one row short of a wave's rows -------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_edges_vs_f64(gpu, case):
    dtype, d, _, kernel, _ = case
    rng = np.random.default_rng(_seed("edges", case_id(case)))
    sizes = _edge_sizes(kernel)
    n = 3 * sizes[0] + 1
    _check_f64(rng, _unit(rng, n, d), _unit(rng, BATCH, d), sizes, case)
    # row norms 1e-2 .. 1e2, query norms 1e-1 .. 1e1: the same numbers, relative to |row| |q| (fp8: a row scale read at
    # the wrong index is off by up to four decades)
    m, qs = _unit(rng, n, d), _unit(rng, BATCH, d)
    m *= (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)[:, None]
    qs *= (10.0 ** rng.uniform(-1, 1, BATCH)).astype(np.float32)[:, None]
    _check_f64(rng, m, qs, sizes[:1], case, relative=True)


# ---- a'. the last wave of the grid exactly full, and holding exactly one row ---------------------------------------------
# (rows of 8 chunks, one zero column at the end: the T = 8 kernels of the table's 6-chunk and 8-chunk rows)
FULL_WAVE_CASES = [(dt, d, "ragged") + next(c[3:5] for c in CASES if c[0] == dt and geometry(c[3]) == (8, 1))
                   for dt, d in (("f32", 31), ("f16", 63), ("fp8", 127))]


@pytest.mark.parametrize("case", FULL_WAVE_CASES, ids=case_id)
def test_last_wave_full_and_one_row(gpu, case):
    """A wave's row count is min(m - base, W) (gather.h).  At m = 2 B the last wave of the grid holds exactly W rows and
    nothing is clamped; at m = 2 B + 1 one more wave holds one row and every other lane of it re-reads that row.  Both
    against f64, and each listed row's score bit-equal to its score inside a longer list, where it sits at another
    position of another wave."""
    dtype, d, _, kernel, _ = case
    w, b = rows_per_wave(kernel), rows_per_block(kernel)
    assert geometry(kernel) == (8, 1) and w == 64 and b == 1024       # U = 8: several rows per lane group
    rng = np.random.default_rng(_seed("fullwave", case_id(case)))
    sizes = [2 * b + 1, 2 * b]
    mat, qs = _unit(rng, 3 * sizes[0], d), _unit(rng, BATCH, d)
    idx = _open(mat, dtype)
    try:
        md, qd = _stored(idx, mat, qs)
        truth = md.astype(np.float64) @ qd.astype(np.float64).T
        for size in sizes:
            rows = _scattered(rng, idx.n, size)
            extra = rng.choice(np.setdiff1d(np.arange(idx.n), rows), w + 3, replace=False)
            longer = np.sort(np.concatenate([rows, extra])).astype(np.int64)
            at = np.searchsorted(longer, rows)
            assert np.count_nonzero(at != np.arange(size)) > size // 2
            for batch in (qs[:1], qs):
                nq = len(batch)
                got = _within(idx, batch, rows, case)
                err = np.abs(got.astype(np.float64) - truth[rows, :nq].T)
                print(f"{case_id(case)} m={size} nq={nq}: max |score - f64| = {float(err.max()):.3g}")
                assert np.all(err <= TOL[dtype]), f"{case_id(case)} m={size} nq={nq}: max |score - f64| = {float(err.max()):.3g}"
                inside = _within(idx, batch, longer, case)[:, at]
                odd = np.argwhere(got.view(np.uint32) != inside.view(np.uint32))
                assert odd.size == 0, (f"{case_id(case)} m={size} nq={nq}: {len(odd)} scores differ in bits from the same rows inside a list "
                                       f"of {len(longer)}, the first query {odd[0][0]}, list position {odd[0][1]}")
    finally:
        idx.release()


# ---- b. one non-zero per listed row ------------------------------------------------------------------------------------
def _away_from_zero(rng, size):
    """Gaussian values with |x| >= 1/64: every value, its half rounding and every product of two are normal numbers, so
    an exact product says where the kernel read, not how a denormal mode is set."""
    x = rng.standard_normal(size, dtype=np.float32)
    return np.copysign(np.maximum(np.abs(x), np.float32(1 / 64)), x)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_nonzero_per_listed_row(gpu, case):
    """Every row but those with r % 8 == 3 is listed, so list positions differ from row numbers from row 4 on; the
    unlisted rows hold a value too, at column r mod d.  Any chunk multiplied against the wrong query chunk, and any
    wrong row, shows."""
    from svs_amd import DeviceIndex
    dtype, d, _, kernel, _ = case
    rng = np.random.default_rng(_seed("onehot", case_id(case)))
    m_min = max(d, 2 * rows_per_block(kernel) + rows_per_wave(kernel) + 1)       # m >= d: every column is some listed row's
    n = (m_min * 8 + 6) // 7 + 8
    listed = np.arange(n) % 8 != 3
    rows = np.flatnonzero(listed).astype(np.int64)
    m = len(rows)
    assert m >= m_min
    col = np.where(listed, (np.cumsum(listed) - 1) % d, np.arange(n) % d)        # listed: list position mod d
    vals = _away_from_zero(rng, n)
    qs = _unit(rng, BATCH, d) if dtype == "fp8" else _away_from_zero(rng, (BATCH, d))
    block = max(BLOCK_ELEMS // d, 1)
    idx = DeviceIndex.empty(d, dtype=dtype, reserve=n)
    try:
        for r0 in range(0, n, block):
            nr = min(block, n - r0)
            blk = np.zeros((nr, d), dtype=np.float32)
            blk[np.arange(nr), col[r0:r0 + nr]] = vals[r0:r0 + nr]
            idx.append(blk)
        assert idx.n == n and idx.ld == choose_ld(d, dtype)
        got1 = _within(idx, qs[:1], rows, case)
        got = _within(idx, qs, rows, case)
        stored = np.empty(n, dtype=np.float32)       # stored[r] = the stored row r at its column
        for r0 in range(0, n, block):
            nr = min(block, n - r0)
            md = vals[r0:r0 + nr, None] if dtype == "f32" else idx.stored_rows(r0, nr)
            if dtype != "f32":
                assert np.count_nonzero(md) == nr, "a stored one-hot row has more than one non-zero"
                md = md[np.arange(nr), col[r0:r0 + nr]]
            stored[r0:r0 + nr] = md.reshape(nr)
        qd = qs if dtype == "f32" else np.stack([idx.stored_query(q) for q in qs])
    finally:
        idx.release()
    stored, col = stored[rows], col[rows]
    for label, g, nq in (("one query", got1, 1), ("a batch", got, BATCH)):
        want = stored[None, :] * qd[:nq, col]                     # one f32 product per listed row and query
        if dtype == "fp8":       # (sum * row scale) * query scale: two more roundings -- the f64 bound, relative to |row| |q|
            err = np.abs(g.astype(np.float64) - stored.astype(np.float64)[None, :] * qd[:nq, col].astype(np.float64))
            err /= np.abs(stored.astype(np.float64))[None, :] * np.linalg.norm(qd[:nq].astype(np.float64), axis=1)[:, None]
            bad = np.argwhere(~(err <= TOL["fp8"]))
        else:                    # adding zeros is exact, and so is a product of two halves in f32
            bad = np.argwhere(g != want)
        assert bad.size == 0, (f"{case_id(case)} n={n} m={m}, {label}: {len(bad)} scores wrong, the first query {bad[0][0]}, list position "
                               f"{bad[0][1]} (row {rows[bad[0][1]]}, column {col[bad[0][1]]}): score {g[tuple(bad[0])]!r}, stored row value x "
                               f"query value = {want[tuple(bad[0])]!r}")


# ---- c. the same row everywhere ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_identical_rows_score_identical_bits(gpu, case):
    dtype, d, _, kernel, _ = case
    rng = np.random.default_rng(_seed("same", case_id(case)))
    sizes = _edge_sizes(kernel)
    row, qs = _unit(rng, 1, d), _unit(rng, BATCH, d)
    idx = _open(np.repeat(row, 3 * sizes[0] + 1, axis=0), dtype)
    try:
        for size in sizes:
            rows = _scattered(rng, idx.n, size)
            alone = _within(idx, qs[:1], rows, case).view(np.uint32)
            batch = _within(idx, qs, rows, case).view(np.uint32)
            for nq, bits in ((1, alone), (BATCH, batch)):
                for j in range(nq):
                    odd = np.flatnonzero(bits[j] != bits[j, 0])
                    assert odd.size == 0, (f"{case_id(case)} m={size} nq={nq} query {j}: {odd.size} copies of one row score other "
                                           f"bits than list position 0 ({bits[j, 0]:#x}), the first at position {odd[0]} ({bits[j, odd[0]]:#x})")
            assert batch[0, 0] == alone[0, 0], f"{case_id(case)} m={size}: query 0 scores other bits in a batch than alone"
    finally:
        idx.release()


# ---- d. a query's bits do not depend on its batch ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batches_score_the_bits_of_single_queries(gpu, case):
    dtype, d, _, kernel, _ = case
    rng = np.random.default_rng(_seed("batches", case_id(case)))
    m = _edge_sizes(kernel)[0]
    idx = _open(_unit(rng, 3 * m + 1, d), dtype)
    qs = _unit(rng, 7, d)
    try:
        rows = _scattered(rng, idx.n, m)
        solo = [_search_all(idx, qs[j:j + 1], rows, case) for j in range(7)]
        for nq in (2, 4, 5, 7):
            s, r = _search_all(idx, qs[:nq], rows, case)
            for j in range(nq):
                assert np.array_equal(r[j], solo[j][1][0]), f"{case_id(case)} m={m}: query {j} ranks other rows in a batch of {nq} than alone"
                odd = np.flatnonzero(s[j].view(np.uint32) != solo[j][0][0].view(np.uint32))
                assert odd.size == 0, (f"{case_id(case)} m={m}: query {j} scores other bits in a batch of {nq} than alone, the first at rank "
                                       f"{odd[0]}: {s[j][odd[0]]!r}, alone {solo[j][0][0][odd[0]]!r}")
    finally:
        idx.release()


# ---- e. non-finite values at both ends of a row ------------------------------------------------------------------------
NONFINITE_CASES = [c for c in CASES if c[0] != "fp8" and (c[2] == "ragged" or geometry(c[3])[1] >= 4)]


@pytest.mark.parametrize("case", NONFINITE_CASES, ids=case_id)
def test_nonfinite_values_at_the_ends_of_a_row(gpu, case):
    """One of +inf, -inf, NaN in column 0 or column d - 1 of single listed rows.  The lanes past the end of a row re-read
    its last chunk and must add exactly nothing, whatever that chunk holds: a row's score is np.dot's on the stored
    values -- +-inf where that is +-inf, NaN only where that is NaN."""
    dtype, d, _, kernel, _ = case
    k = 10
    rng = np.random.default_rng(_seed("nonfinite", case_id(case)))
    w, b = rows_per_wave(kernel), rows_per_block(kernel)
    m = 2 * b + w + 1
    mat, qs = _unit(rng, 3 * m + 1, d), _unit(rng, 2, d)
    rows = _scattered(rng, len(mat), m)
    spots = sorted({0, 1, w, w + 1, b - 1, b, m // 2, m - 2, m - 1})       # list positions: first and last of a wave, a block, the list
    spots = spots[:3] + spots[-3:]
    big = {"f32": np.inf, "f16": 1e5}[dtype]                                # (f16 ingest turns |x| > 65504 into inf)
    plant = [(int(rows[p]), col, val) for p, (val, col) in zip(spots, [(v, c) for v in (big, -big, np.nan) for c in (0, d - 1)])]
    assert len(plant) == 6
    for row, col, val in plant:
        mat[row, col] = val
    qs[0, [0, d - 1]] = (np.abs(qs[0, [0, d - 1]]) + np.float32(1e-3)) * np.array([1, -1], dtype=np.float32)   # non-zero, both signs
    qs[1, d - 1] = 0.0
    idx = _open(mat, dtype)
    try:
        md, qd = _stored(idx, mat, qs)
        for row, col, val in plant:
            assert (np.isnan(md[row, col]) if np.isnan(val) else md[row, col] == np.sign(val) * np.inf), (row, col, md[row, col])
            assert np.count_nonzero(~np.isfinite(md[row])) == 1
        assert qd[1, d - 1] == 0 and np.all(qd[0, [0, d - 1]] != 0)
        sub = md[rows]
        with np.errstate(all="ignore"):
            want = np.dot(sub, qd.T).T                                      # (2, m) f32
            t64 = (sub.astype(np.float64) @ qd.astype(np.float64).T).T
        for label, got, js in [("alone", np.concatenate([_within(idx, qs[j:j + 1], rows, case) for j in range(2)]), (0, 1)),
                               ("as a batch", _within(idx, qs, rows, case), (0, 1))]:
            for j in js:
                what = f"{case_id(case)} ld={idx.ld} m={m} query {j} {label}"
                g, wj = got[j], want[j]
                print(f"{what}: planted rows score {[(p, float(g[p]), float(wj[p])) for p in spots]} (list position, kernel, np.dot)")
                assert np.array_equal(np.isnan(g), np.isnan(wj)), \
                    f"{what}: NaN at list positions {np.flatnonzero(np.isnan(g)).tolist()}, np.dot has it at {np.flatnonzero(np.isnan(wj)).tolist()}"
                inf = np.isinf(wj)
                assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], wj[inf]), \
                    f"{what}: infinities {g[np.isinf(g) | inf].tolist()} at list positions {np.flatnonzero(np.isinf(g) | inf).tolist()}, np.dot {wj[np.isinf(g) | inf].tolist()}"
                fin = np.isfinite(wj)
                err = np.abs(g[fin].astype(np.float64) - t64[j][fin])
                assert err.max() <= TOL[dtype], f"{what}: max |score - f64| over the finite rows = {err.max():.3g}"
        for j in range(2):
            # (test data: the ranks among the finite scores of the top k are decided by more than both roundings)
            lead = np.sort(t64[j][np.isfinite(want[j])])[::-1][:k + 1]
            assert np.min(-np.diff(lead)) > 2 * TOL[dtype], f"{case_id(case)} query {j}: a near tie among the top finite scores of the test data"
            exp = oracle.total_order_top_k(want[j], k)
            top = idx.search_within(qs[j], k, rows)
            assert [i for _, i in top] == [int(rows[p]) for _, p in exp], \
                f"{case_id(case)} query {j}: search_within returns {top}, the total order on np.dot {[(s, int(rows[p])) for s, p in exp]}"
    finally:
        idx.release()
