"""Exact corpora and an exact reference for svs_index_top_pairs: plain numpy, importable without a GPU.

Every entry of a corpus is a small integer, so every dot product is exact in every dtype and in every summation order
(tests/test_pairs_exact_gpu.py then compares without a tolerance):
  * f32 / f16: integers in [-4, 4]; |score| <= 16 d, far below 2^24.
  * fp8: integers in [-7, 7] with at least one +-7 in every row.  The row scale is then exactly 7 / 448 = 2^-6 and the
    stored bytes are 64 x -- all 15 values are e4m3fn numbers.  Products of stored bytes are multiples of 2^12 up to
    448^2, and their f32 sum stays exact up to d = 1024 (49 d < 2^24 in units of 2^12).
check_stored() holds a built index to that: what it stores must equal the input bit for bit.

Exact duplicates (m[j] = m[i]) are planted where the pair-mode index arithmetic has its seams (svs_amd.hip
top_pairs_tiled, gemm_tiled.h tg_epilogue, gemm_phased.h): the corpus ends, the 256-row tiles, the 1024-query chunks, the
first rows of a chunk for each i mod 4, the moved-back last chunk and the prefix block's edge.  Duplicates score |row|^2,
~11 sigma above a random pair, so the top of the list sits on those seams.

reference_top_pairs() is a chunked f64 restatement of get_top_pairs (reference src/svs/util.py:206-233) on the rows:
only columns j > i are formed, a running k-th-best bound filters each chunk, the final order is (score desc, i desc,
j desc) -- the reference's flat upper-triangle index, descending.
"""
import functools

import numpy as np

QC = 1024        # query rows per chunk of the tiled pair path
SEL_KMAX = 2048  # select.h: more results than this take the sort path (and an 8192-row prefix block)
K_MARGIN = 400   # reference entries computed past the nominal k: the tie that k is moved onto lies inside them


def _tiled(bn, eb, bm):
    return f"gemm_tiled_kernel<{bn}, true, {eb}, {bm}>"


def _phased(eb):
    return f"gemm_phased_kernel<true, {eb}, 0, 256>"


# (name, dtype, d, n, nominal k, pair-mode kernel of a 1024-query chunk).  n is no multiple of 4, 256 or 1024 and covers
# n % 4 = 1, 2, 3; the larger d go with the smaller n.  Kernel per batch_route / launch_tiled_eb / phased_ok:
#   f32: 64-query tiles; f16 / fp8: 256-query tiles, the phased kernel when a row is an even number (>= 6) of 128-byte
#   k-tiles, else the tiled kernel at 256 x 256 (fp8: the instantiation that spills).
CASES = [
    ("f32-d96", "f32", 96, 17001, 500, _tiled(64, 4, 128)),         # 3 k-tiles
    ("f16-d64", "f16", 64, 17002, 500, _tiled(256, 2, 256)),        # 1 k-tile
    ("f16-d192", "f16", 192, 16999, 500, _tiled(256, 2, 256)),      # 3 k-tiles (odd)
    ("fp8-d128", "fp8", 128, 17003, 500, _tiled(256, 1, 256)),      # 1 k-tile
    ("f16-d512", "f16", 512, 9501, SEL_KMAX + 1, _phased(2)),       # 8 k-tiles
    ("fp8-d384", "fp8", 384, 9502, SEL_KMAX + 1, _tiled(256, 1, 256)),   # 3 k-tiles (odd)
    ("fp8-d768", "fp8", 768, 9503, SEL_KMAX + 1, _phased(1)),       # 6 k-tiles: the phased kernel's minimum
    ("fp8-d1024", "fp8", 1024, 9499, SEL_KMAX + 1, _phased(1)),     # 8 k-tiles: the longest exact fp8 row
]
CASE_IDS = [c[0] for c in CASES]


def value_limit(dtype):
    return 7 if dtype == "fp8" else 4


def check_exactness_bounds(dtype, d, lim):
    """The conditions under which every score of an integer corpus is exact (module docstring)."""
    assert 1 <= lim <= 7
    assert 49 * d < 2 ** 24                    # |score| <= lim^2 d: an exact f32 integer whatever the summation order
    if dtype == "fp8":
        assert lim == 7 and d <= 1024          # row scale 2^-6 exactly; sums of multiples of 2^12 up to 448^2 d


def check_e4m3_values():
    """All 15 stored values 64 x, x = -7 .. 7, are e4m3fn numbers (torch's CPU cast)."""
    import torch
    v = torch.arange(-7, 8, dtype=torch.float32) * 64
    assert torch.equal(v.to(torch.float8_e4m3fn).to(torch.float32), v)


def integer_rows(seed, n, d, dtype):
    lim = value_limit(dtype)
    check_exactness_bounds(dtype, d, lim)
    rng = np.random.default_rng(seed)
    m = rng.integers(-lim, lim + 1, size=(n, d), dtype=np.int8).astype(np.float32)
    if dtype == "fp8":                          # one +-7 per row: the row's scale is 7 / 448 whatever else it holds
        m[np.arange(n), rng.integers(0, d, size=n)] = 7.0 * rng.choice(np.array([-1.0, 1.0], np.float32), size=n)
    return m


def prefix_rows(n, k):
    """P of top_pairs_tiled on a corpus without tombstones."""
    p = min(n, 8192 if k > SEL_KMAX else 16384)
    while p < n and p * (p - 1) // 2 < k:
        p = min(n, 2 * p)
    return p


def last_chunk(n):
    """(qs, q0) of the moved-back last chunk: it starts at row qs and answers for queries from q0 on."""
    q0 = (n - 2) // QC * QC
    return max(0, min(q0, n - QC)), q0


def pair_chunks(n):
    """[(qs, row_base, q0)] of top_pairs_tiled's query chunks."""
    out = []
    for q0 in range(0, n - 1, QC):
        qs = max(0, min(q0, n - QC))
        out.append((qs, (qs + 1) & ~3, q0))
    return out


def planted_pairs(n, P):
    """The duplicate pairs (i, j), i < j, of a corpus of n rows whose prefix block holds P rows."""
    pairs = [(0, 1), (0, n - 1), (n - 2, n - 1)]                       # chains: (1, n - 1), (0, n - 2), ... tie with them
    t = 1
    for r in (0, 255):                                                  # row tiles: j - i around 256, i at a tile's edges
        for delta in (1, 255, 256, 257):
            i = 256 * (4 * t + 1) + r                                   # tiles 5, 9, ...: clear of the multiples of 1024
            pairs.append((i, i + delta))
            t += 1
    for c in range(QC, n, QC):                                          # both sides of every multiple of 1024
        pairs.append((c - 1, c))
    for r in range(4):                                                  # i mod 4 just after a chunk start
        i = QC * (2 + r) + r
        pairs += [(i, i + 1), (i, i + 2), (i, i + 3)]
    qs, q0 = last_chunk(n)
    pairs += [(qs - 7, qs), (qs, qs + 5), (qs + 1, n - 3)]              # the moved-back last chunk: rows it re-reads
    pairs += [(q0 - 1, q0), (q0 - 2, q0 + 2), (q0, q0 + 3)]             # ... and the first it answers for
    if P < n:
        pairs += [(P - 1, P), (P - 3, P + 2)]                           # both sides of the prefix block's edge
    pairs = sorted(set(pairs))
    assert all(0 <= i < j < n for i, j in pairs)
    return pairs


def plant(m, pairs):
    """m[j] = m[i] for every pair, in place: rows linked by a chain of pairs all become the chain's lowest row."""
    parent = list(range(len(m)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in pairs:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for i, j in pairs:
        for x in (i, j):
            m[x] = m[find(x)]
    return m


def reference_top_pairs(rows, k, chunk=QC):
    """The k best pairs (i < j) of rows.rows^T in f64: [(score, i, j)] ordered (score desc, i desc, j desc)."""
    m = np.asarray(rows, dtype=np.float64)
    n = m.shape[0]
    ks, ki, kj = np.empty(0, np.float64), np.empty(0, np.int64), np.empty(0, np.int64)
    for r0 in range(0, n - 1, chunk):
        r1 = min(n, r0 + chunk)
        s = m[r0:r1] @ m[r0:].T                                        # columns r0 .. n - 1 only
        s[:, :r1 - r0][np.tri(r1 - r0, dtype=bool)] = -np.inf          # j <= i inside the diagonal block
        if ks.size >= k:
            bound = ks[-1]                                              # the running k-th best
        else:                                                           # no bound yet: the chunk's own k-th best, ties kept
            live = int(np.isfinite(s).sum())
            bound = np.partition(s.ravel(), -k)[-k] if live >= k else -np.inf
        a, c = np.nonzero(s >= bound if np.isfinite(bound) else np.isfinite(s))
        ks = np.concatenate([ks, s[a, c]])
        ki = np.concatenate([ki, r0 + a])
        kj = np.concatenate([kj, r0 + c])
        order = np.lexsort((-kj, -ki, -ks))[:k]                         # score desc, i desc, j desc
        ks, ki, kj = ks[order], ki[order], kj[order]
    return [(float(a), int(b), int(c)) for a, b, c in zip(ks, ki, kj)]


def tie_cut_k(ref, nominal):
    """The first k >= nominal with ref[k - 1] and ref[k] tied: a top-k that cuts a tie group."""
    for k in range(max(nominal, 1), len(ref)):
        if ref[k - 1][0] == ref[k][0]:
            return k
    raise AssertionError(f"no tie from rank {nominal} to {len(ref)}: raise K_MARGIN")


class PairCase:
    """One corpus, its planted pairs and its expected answer (the reference is computed on first use, once)."""

    def __init__(self, name, dtype, d, n, nominal_k, kernel):
        self.name, self.dtype, self.d, self.n, self.nominal_k, self.kernel = name, dtype, d, n, nominal_k, kernel
        self.P = prefix_rows(n, nominal_k + K_MARGIN)                   # (the same for every k the case can end up with)
        assert self.P == prefix_rows(n, nominal_k) and self.P < n
        self.planted = planted_pairs(n, self.P)
        self.rows = plant(integer_rows(1000 + n + d, n, d, dtype), self.planted)
        self._ref = None

    @property
    def reference(self):
        if self._ref is None:
            self._ref = reference_top_pairs(self.rows, self.nominal_k + K_MARGIN)
        return self._ref

    @property
    def k(self):
        return tie_cut_k(self.reference, self.nominal_k)

    @property
    def expected(self):
        return self.reference[:self.k]


@functools.lru_cache(maxsize=None)
def build_case(name):
    """The case of that name, built once per process (its rows are shared: leave them unchanged)."""
    return PairCase(*CASES[CASE_IDS.index(name)])


def reference_on_live(rows, dead, k):
    """reference_top_pairs over the rows that are not in `dead`, with the original row numbers."""
    live = np.setdiff1d(np.arange(len(rows)), np.asarray(sorted(dead), dtype=np.int64))
    ref = reference_top_pairs(rows[live], k)
    return [(s, int(live[i]), int(live[j])) for s, i, j in ref]


def identical_rows(n, d, dtype):
    """n copies of one integer row, and that row's |row|^2."""
    row = integer_rows(77 + d, 1, d, dtype)[0]
    return np.tile(row, (n, 1)), float(np.dot(row.astype(np.float64), row.astype(np.float64)))


def all_tied_expected(n, k, score):
    """The first k of all n (n - 1) / 2 pairs at one score: (n-2, n-1), (n-3, n-1), (n-3, n-2), ... (i desc, j desc)."""
    out = []
    for i in range(n - 2, -1, -1):
        for j in range(n - 1, i, -1):
            out.append((score, i, j))
            if len(out) == k:
                return out
    return out


def exact_scores(queries, rows, block=16384):
    """queries.rows^T in f64, a block of rows at a time."""
    q = np.asarray(queries, dtype=np.float64)
    return np.concatenate([q @ rows[r:r + block].astype(np.float64).T for r in range(0, len(rows), block)], axis=1)


def check_stored(idx, rows):
    """What the index holds equals the input bit for bit (an inexact corpus fails here, not in a comparison later)."""
    got = idx.stored_rows()
    assert got.dtype == np.float32 and got.shape == rows.shape
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(rows, dtype=np.float32).view(np.uint32))


def assert_exact(got, exp, row_offset=0):
    """got (the library's [(score, i, j)]) equals exp position by position: the same pairs, score bits == float32(exp)."""
    assert len(got) == len(exp)
    gp = [(i, j) for _, i, j in got]
    assert all(i < j for i, j in gp)
    assert len(set(gp)) == len(gp), "a pair is returned twice"
    ep = [(i + row_offset, j + row_offset) for _, i, j in exp]
    wrong = [t for t in range(len(gp)) if gp[t] != ep[t]]
    assert not wrong, (len(wrong), wrong[:5], [got[t] for t in wrong[:5]], [exp[t] for t in wrong[:5]])
    gs = np.array([s for s, _, _ in got], dtype=np.float32).view(np.uint32)
    es = np.array([s for s, _, _ in exp], dtype=np.float64).astype(np.float32).view(np.uint32)
    bad = np.nonzero(gs != es)[0]
    assert bad.size == 0, (bad.size, [(got[t], exp[t]) for t in bad[:5]])
