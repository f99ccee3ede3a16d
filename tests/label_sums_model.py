"""The model of svs_index_label_sums (per-label row sums).  Not a test module: tests/test_label_sums_model.py tests it on
the CPU, the GPU and host tests use it.

Definition (include/svs_amd.h): for each position j of ``labels``, the LIVE rows with lab[r] == labels[j] in ascending
order are cut into chunks of 256; a chunk's partial sum is one chain of f64 additions over its rows from +0.0, the
label's sum one chain over its partials from +0.0.  ``replay`` performs exactly these additions, in this order, so a
device answer is compared BIT FOR BIT; ``exact`` is the correctly rounded true sum (math.fsum), which the definition
equals whenever every partial sum is representable."""
import math

import numpy as np

CHUNK = 256


def _rows_of(lab, live, label):
    lab = np.asarray(lab)
    sel = lab == label
    if live is not None:
        sel = sel & np.asarray(live, dtype=bool)
    return np.flatnonzero(sel)


def chain(rows64, start=None):
    """(((start + rows64[0]) + rows64[1]) + ...) column-wise, one IEEE f64 addition at a time; start: +0.0."""
    acc = np.zeros(rows64.shape[1], dtype=np.float64) if start is None else start
    for row in rows64:
        acc = acc + row          # (never np.sum: it adds pairwise)
    return acc


def replay(stored, lab, live, labels, chunk=CHUNK, order=None):
    """(sums f64 (L, d), counts i64 (L,)): the definition, row by row.  ``stored``: the range's rows as stored (f32);
    ``lab``: their labels; ``live``: a boolean per row, or None; ``chunk``: rows per partial sum (None: one chain over
    all rows); ``order``: a function applied to each label's ascending row list (tests of other orders)."""
    x = np.asarray(stored, dtype=np.float64)     # (the widening is exact)
    labels = list(np.asarray(labels).reshape(-1).tolist())
    sums = np.zeros((len(labels), x.shape[1]), dtype=np.float64)
    counts = np.zeros(len(labels), dtype=np.int64)
    for j, label in enumerate(labels):
        rows = _rows_of(lab, live, label)
        if order is not None:
            rows = order(rows)
        counts[j] = len(rows)
        step = max(len(rows), 1) if chunk is None else chunk
        total = np.zeros(x.shape[1], dtype=np.float64)
        for a in range(0, len(rows), step):
            total = total + chain(x[rows[a:a + step]])
        sums[j] = total
    return sums, counts


def exact(stored, lab, live, labels):
    """(sums, counts) with every element the correctly rounded true sum (math.fsum per column)."""
    x = np.asarray(stored, dtype=np.float64)
    labels = list(np.asarray(labels).reshape(-1).tolist())
    sums = np.zeros((len(labels), x.shape[1]), dtype=np.float64)
    counts = np.zeros(len(labels), dtype=np.int64)
    for j, label in enumerate(labels):
        rows = _rows_of(lab, live, label)
        counts[j] = len(rows)
        if len(rows):
            sums[j] = [math.fsum(col) for col in x[rows].T.tolist()]
    return sums, counts


def means(sums, counts):
    """The f64 means; a label with count 0 gets zeros (DeviceIndex.label_means before its cast)."""
    out = np.zeros(sums.shape, dtype=np.float64)
    has = counts > 0
    out[has] = sums[has] / counts[has, None].astype(np.float64)
    return out


def same_bits(a, b):
    """Bit equality of two f64 arrays (so -0.0 != +0.0 and NaNs compare by payload)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def wide(rng, n, d):
    """Unit-norm Gaussian rows each scaled by 2^e, e uniform in -20 .. 20: sums whose rounding depends on the order."""
    e = rng.integers(-20, 21, size=n)
    return (unit(rng, n, d).astype(np.float64) * np.exp2(e)[:, None]).astype(np.float32)
