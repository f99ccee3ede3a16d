"""TEST DOUBLE for the CPU suite only: fake_backend.OracleIndex with DeviceIndex's columns -- ``set_column`` /
``column`` / ``set_labels`` (column 0) / ``search_where`` / ``search_labeled`` / ``search_within`` -- whose filter is
the numpy model of tests/where_model.py and whose arithmetic is the oracle's."""
import numpy as np

from fake_backend import OracleIndex
from oracle import svs_oracle as oracle
from where_model import where_mask

COLUMNS = 4


class ColumnOracleIndex(OracleIndex):
    """State [matrix, dead mask, columns (COLUMNS, n) u32], shared by every owner like the HBM copy."""

    dtype = "f32"
    set_calls = []      # (column, local row0, number of values) of every write, all instances

    def __init__(self, matrix, device=0, row_offset=0, _shared=None):
        super().__init__(matrix, device, row_offset, _shared=_shared)
        if len(self._st) == 2:
            self._st.append(np.zeros((COLUMNS, self.n), dtype=np.uint32))

    def share(self):
        self._check()
        return ColumnOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def append(self, rows):
        super().append(rows)
        grown = np.zeros((COLUMNS, self.n), dtype=np.uint32)
        grown[:, :self._st[2].shape[1]] = self._st[2]
        self._st[2] = grown

    def set_column(self, c, values, row0=None):
        self._check()
        val = np.asarray(values, dtype=np.uint32).reshape(-1)
        r0 = 0 if row0 is None else int(row0) - self.row_offset
        if not 0 <= c < COLUMNS or r0 < 0 or r0 + len(val) > self.n:
            raise ValueError("column or rows outside the index")
        ColumnOracleIndex.set_calls.append((c, r0, len(val)))
        self._st[2][c, r0:r0 + len(val)] = val

    def set_labels(self, labels, row0=None):
        self.set_column(0, labels, row0)

    def column(self, c, row0=None, nrows=None):
        self._check()
        r0 = 0 if row0 is None else int(row0) - self.row_offset
        return self._st[2][c, r0:(self.n if nrows is None else r0 + nrows)].copy()

    def _top(self, q, n, S):
        assert isinstance(n, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        top = oracle.total_order_top_k(oracle.cpu_scores(self._m[S], q), min(max(n, 0), len(S))) if len(S) else []
        return [(s, int(S[p]) + self.row_offset) for s, p in top]

    def search_where(self, q, n, where):
        self._check()
        cols = {c: self._st[2][c] for c in range(COLUMNS)}
        S = np.flatnonzero(where_mask(cols, [(c, op, list(arg) if op in ("in", "not in") else arg) for c, op, arg in where], self.n)
                           & ~self._st[1])
        return self._top(q, n, S), len(S)

    def search_labeled(self, q, n, labels):
        return self.search_where(q, n, [(0, "in", list(labels))])

    def search_within(self, q, n, rows):
        self._check()
        S = np.unique(np.asarray(rows, dtype=np.int64)) - self.row_offset
        return self._top(q, n, S[~self._st[1][S]])
