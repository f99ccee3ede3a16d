"""The far layout of tests/test_far_rows_gpu.py: an index of just over 64 GiB whose interesting rows lie on the
32-bit offset boundaries of a row buffer, and filler everywhere else.  Pure arithmetic and numpy: no GPU, no library.

Rows are ROW_BYTES = 3,072 bytes for every dtype (f32 d = 768, f16 d = 1536, fp8 d = 3072; ld = d for each), so one
layout serves all three.  3,072 divides no power of two, so a row STRADDLES every boundary.

Planted rows: six blocks of BLOCK = 342 unit-norm Gaussian rows.  Block p (p = 31 .. 36) is centred on byte offset 2^p
of the row buffer: its middle row (position MID = 171 of the block) is the row that contains byte 2^p.  In other units
the same six bytes are

    p    bytes   f32 elements   f16 elements   16-byte chunks
    31   2^31    2^29           2^30           2^27
    32   2^32    2^30           2^31           2^28
    33   2^33    2^31           2^32           2^29
    34   2^34    2^32           2^33           2^30
    35   2^35    2^33           2^34           2^31    (a signed 32-bit chunk offset turns negative)
    36   2^36    2^34           2^35           2^32    (row * ld16 as a 32-bit unsigned product wraps)

Filler: one block of FILL_ROWS unit-norm Gaussian rows scaled by FILL_SCALE = 2^-7 (about 1 GiB as stored), appended
again and again from its first row; the appends between two planted blocks take as many of its leading rows as fit.
The index ends TAIL = 1,027 rows after block 36, so n is no multiple of 4, 64 or 1,024."""
from collections import namedtuple

import numpy as np

ROW_BYTES = 3072
CHUNK_BYTES = 16
LD16 = ROW_BYTES // CHUNK_BYTES                 # 192 chunks per row
DIMS = {"f32": 768, "f16": 1536, "fp8": 3072}   # ld == d for each (single_kernel_table.choose_ld)
ELEM_BYTES = {"f32": 4, "f16": 2, "fp8": 1}
POWERS = (31, 32, 33, 34, 35, 36)
BLOCK = 342
MID = BLOCK // 2
TAIL = 1027
FILL_ROWS = (1 << 30) // ROW_BYTES              # 349,525 rows: the last whole row below 1 GiB
FILL_SCALE = 2.0 ** -7
# |<filler row, query>| <= |filler row| |query| (Cauchy-Schwarz) = 2^-7 for unit vectors; each 1.0625 allows for the fp8
# rounding of one operand (e4m3 keeps 3 mantissa bits: a relative error of at most 2^-4 per element, so of the norm)
FILL_BOUND = FILL_SCALE * 1.0625 ** 2

SEED_ROWS = 20280          # numpy seed of the planted rows (one per d: SEED_ROWS + d)
SEED_QUERIES = 20281       # ... of the queries
NQ = 256                   # queries drawn per d (each case takes the first few)
K = 100                    # the k of the whole-corpus top-k cases
ABOVE_CUT = 0.02           # search_above's cut-off: above FILL_BOUND plus any tolerance the project holds a kernel to
ABOVE_QUERIES = 4          # the threshold cases use the first queries only

Append = namedtuple("Append", "row0 count kind source")   # kind "fill": filler rows [0, count); "plant": block `source`
Span = namedtuple("Span", "p row_first row_last byte_first byte_last chunk_first chunk_last")


class Layout:
    """The far layout for rows of ``row_bytes`` bytes (a multiple of 16).  ``FAR`` below is the 3,072-byte layout every
    dtype shares; ``SHADOWED`` is the f32-only second geometry, rows of 8 KiB (d = 2048), the shortest-lived way to a
    far index that HAS a half shadow (an f32 row must be whole 512-float steps for one).  Its rows start exactly on each
    boundary instead of straddling it; the planted blocks around each 2^p exercise every wrap all the same."""

    def __init__(self, row_bytes: int, dims):
        assert row_bytes % CHUNK_BYTES == 0
        self.row_bytes, self.dims = row_bytes, dict(dims)
        self.ld16 = row_bytes // CHUNK_BYTES
        self.fill_rows = (1 << 30) // row_bytes         # at most 1 GiB as stored

    def block_start(self, p: int) -> int:
        """The index row of block p's first row: its MID-th row is the one that holds byte 2^p."""
        return (1 << p) // self.row_bytes - MID

    def n_rows(self) -> int:
        return self.block_start(POWERS[-1]) + BLOCK + TAIL

    def schedule(self):
        """The appends that build the index, in order: Append(row0, count, kind, source).  Filler appends never exceed
        fill_rows rows and always start at the filler block's row 0; a planted block is one append of its own."""
        out, at = [], 0

        def fill(upto):
            nonlocal at
            while at < upto:
                c = min(self.fill_rows, upto - at)
                out.append(Append(at, c, "fill", 0))
                at += c

        for p in POWERS:
            fill(self.block_start(p))
            out.append(Append(at, BLOCK, "plant", p))
            at += BLOCK
        fill(self.n_rows())
        return out

    def loc(self) -> np.ndarray:
        """The index row of each planted row, i64: planted row i = block i // BLOCK, position i % BLOCK."""
        return np.concatenate([self.block_start(p) + np.arange(BLOCK, dtype=np.int64) for p in POWERS])

    def spans(self):
        """Per planted block: its first and last index row, the first byte of the first row, the LAST byte of the last
        row, and the same two in 16-byte chunks.  (Element offsets of a dtype are byte offsets // ELEM_BYTES[dtype].)"""
        out = []
        for p in POWERS:
            r0 = self.block_start(p)
            r1 = r0 + BLOCK - 1
            out.append(Span(p, r0, r1, r0 * self.row_bytes, (r1 + 1) * self.row_bytes - 1, r0 * self.ld16, (r1 + 1) * self.ld16 - 1))
        return out

    def filler_source(self, row: int) -> int:
        """The row of the filler block that index row `row` is a copy of; ValueError for a planted row."""
        for a in self.schedule():
            if a.row0 <= row < a.row0 + a.count:
                if a.kind != "fill":
                    raise ValueError(f"row {row} is a planted row of block {a.source}")
                return a.source + row - a.row0
        raise ValueError(f"row {row} is outside the index")

    def boundary_fillers(self):
        """Filler rows on both sides of every boundary: the row just below and the row just above each planted block,
        and the rows MID + 2 further out (i64, ascending)."""
        rows = []
        for s in self.spans():
            rows += [s.row_first - MID - 2, s.row_first - 1, s.row_last + 1, s.row_last + MID + 2]
        return np.array(rows, dtype=np.int64)

    def wrapped_row(self, row: int, bits: int = 32, unit=None, signed: bool = False) -> float:
        """Where a kernel lands that computes row * unit in `bits` bits (unit: chunks per row by default): the offset it
        addresses, in rows of the buffer (fractional inside a row; negative for a signed wrap below the buffer)."""
        unit = self.ld16 if unit is None else unit
        off = (row * unit) & ((1 << bits) - 1)
        if signed and off >= 1 << (bits - 1):
            off -= 1 << bits
        return off / unit


FAR = Layout(ROW_BYTES, DIMS)
SHADOWED = Layout(8192, {"f32": 2048})
LAYOUTS = {"fp8": ("fp8", FAR), "f16": ("f16", FAR), "f32": ("f32", FAR), "f32-shadowed": ("f32", SHADOWED)}   # case -> (dtype, layout)

block_start, n_rows, schedule, loc, spans = FAR.block_start, FAR.n_rows, FAR.schedule, FAR.loc, FAR.spans
filler_source, boundary_fillers, wrapped_row = FAR.filler_source, FAR.boundary_fillers, FAR.wrapped_row


def block_of(p: int) -> slice:
    """Block p's rows among the planted rows (and in the near twin)."""
    b = POWERS.index(p)
    return slice(b * BLOCK, (b + 1) * BLOCK)


def planted_rows(dtype: str, d=None) -> np.ndarray:
    """The 2,052 planted rows of a dtype's dimension (or of ``d``), f32 unit-norm Gaussian."""
    d = DIMS[dtype] if d is None else d
    x = np.random.default_rng(SEED_ROWS + d).standard_normal((len(POWERS) * BLOCK, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def queries(dtype: str, nq: int = NQ, d=None) -> np.ndarray:
    d = DIMS[dtype] if d is None else d
    q = np.random.default_rng(SEED_QUERIES + d).standard_normal((NQ, d), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q[:nq]


def planted_only(kth_scores, tol: float) -> bool:
    """The condition of every case that ranks the whole corpus, judged on the REFERENCE's k-th best scores alone: each
    exceeds what any filler row can score plus the case's tolerance, so the answer holds planted rows only."""
    return bool(np.all(np.asarray(kth_scores, dtype=np.float64) > FILL_BOUND + tol))
