#!/usr/bin/env python3
"""Per-label row sums (svs_index_label_sums): host-call time of DeviceIndex.label_sums over a 1M x 1536 corpus built on
the device, with random row labels over c = 16, 256 and 1,024 labels (the call's row_labels, so 4 bytes per row go up),
beside -- in the same process, the calls alternating --
  (i)   kernel   the chunk-sum and fold kernels alone, from HIP events around them (svs_index_set_timing), in calls of
                 their own: their time and the corpus bytes per second (n ld bytes, every row read once).
  (ii)  pass     the score kernel of a single-query search over the same index (unscreened), from the search's own
                 timing: the corpus read once, the HBM-read floor the sums are compared against.
  (iii) count    a count-only call (sums=False): the histogram alone.
  (iv)  kmeans   one k-means iteration (DeviceIndex.kmeans(c, iterations=1, init=...): one assign, one label_sums).
  (v)   host     the alternative without the entry: ``stored_rows()`` of ``host_rows`` rows plus a numpy f64 reduction per
                 label, at a size that fits; also scaled linearly to n rows.
Statistic: the p50 of ``reps`` warmed calls ((i): of 5; (iv), (v): of ``slow_reps``).  Nothing is asserted but that the
sums of the first host_rows rows agree with the host alternative to 1e-9 relative: the figures are what the run shows.
Writes a table and one JSON line.
  usage: label_sums_time.py [n=1000000] [d=1536] [dtypes=f32,f16,fp8] [reps=10] [slow_reps=3] [host_rows=100000]
                            [out=profiles/label_sums_time.txt]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from svs_amd import DeviceIndex, _native
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16,fp8").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
slow_reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
host_rows = min(int(sys.argv[6]) if len(sys.argv) > 6 else 100_000, n)
out_path = sys.argv[7] if len(sys.argv) > 7 else os.path.join(ROOT, "profiles", "label_sums_time.txt")
CS = [16, 256, 1024]
ESZ = {"f32": 4, "f16": 2, "fp8": 1}
lib = _native.load()


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def p50(v):
    return round(float(np.percentile(v, 50)), 4)


def kernel_ms(idx, ids, rl):
    """The chunk-sum and fold kernels alone: the HIP events of one timed call."""
    idx.set_timing(1)
    try:
        idx.label_sums(ids, row_labels=rl)
        ms = C.c_double(-1.0)
        _native.check(lib.svs_internal_label_sums_kernel_ms(C.byref(ms)))
    finally:
        idx.set_timing(0)
    assert ms.value > 0, "no kernel time was recorded"
    return ms.value


def pass_ms(idx, q):
    """The score kernel of one single-query search, from the search's own events."""
    idx.set_timing(1)
    try:
        s0, _, l0 = idx.get_timing()
        idx.search(q, 10)
        s1, _, l1 = idx.get_timing()
    finally:
        idx.set_timing(0)
    assert l1 > l0, "the search recorded no time"
    return (s1 - s0) / (l1 - l0)


def host_sums(idx, rl, c, rows_n):
    """(v): the rows out of HBM, then one f64 reduction per label."""
    rows = idx.stored_rows(0, rows_n)
    order = np.argsort(rl[:rows_n], kind="stable")
    starts = np.searchsorted(rl[:rows_n][order], np.arange(c))
    sums = np.zeros((c, rows.shape[1]), dtype=np.float64)
    has = np.diff(np.append(starts, rows_n)) > 0
    sums[has] = np.add.reduceat(rows[order], starts[has], axis=0, dtype=np.float64)
    return sums


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(17)
rng = np.random.default_rng(17)
out = {"n": n, "d": d, "csrc_sha16": csrc_sha16(), "reps": reps, "slow_reps": slow_reps, "host_rows": host_rows}
lines = []
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    _native.check(lib.svs_index_set_screen(idx._handle(), 0))      # (ii) reads the corpus itself, not an f16 shadow
    q = torch.randn(d, generator=torch.Generator().manual_seed(3)).numpy()
    q /= np.linalg.norm(q)
    corpus_bytes = n * idx.ld * ESZ[dtype]
    res = {}
    for c in CS:
        ids = np.arange(c, dtype=np.uint32)
        rl = rng.integers(0, c, size=n).astype(np.uint32)
        sums, counts = idx.label_sums(ids, row_labels=rl)       # (warm afterwards)
        assert int(counts.sum()) == n and np.array_equal(counts, np.bincount(rl, minlength=c))
        hs = host_sums(idx, rl, c, host_rows)
        part, _ = idx.label_sums(ids, row_labels=rl[:host_rows], row0=0, nrows=host_rows)
        err = float(np.abs(part - hs).max() / max(np.abs(hs).max(), 1e-300))
        assert err <= 1e-9, f"{dtype} c={c}: the device sums differ from the host's by {err:.3g} relative"
        idx.search(q, 10)
        init = idx.stored_rows(0, c)      # (iv): the first centroids, fetched outside the timed call
        times = {"call": [], "count": [], "kmeans": [], "host": []}
        passes = []
        for rep in range(reps):       # alternating, so that drift hits all alike
            times["call"].append(timed(lambda: idx.label_sums(ids, row_labels=rl)))
            times["count"].append(timed(lambda: idx.label_sums(ids, row_labels=rl, sums=False)))
            passes.append(pass_ms(idx, q))
            if rep < slow_reps:
                times["kmeans"].append(timed(lambda: idx.kmeans(c, iterations=1, init=init)))
                times["host"].append(timed(lambda: host_sums(idx, rl, c, host_rows)))
                idx.label_sums(ids, row_labels=rl)      # (untimed: the GPU idled while the host added rows)
        kern = p50([kernel_ms(idx, ids, rl) for _ in range(5)])
        call, cnt, ps, km, host = p50(times["call"]), p50(times["count"]), p50(passes), p50(times["kmeans"]), p50(times["host"])
        host_n = round(host * n / host_rows, 1)
        res[str(c)] = {"call_ms": call, "kernel_ms": kern, "pass_kernel_ms": ps, "kernel_over_pass": round(kern / ps, 2),
                       "call_over_pass": round(call / ps, 2), "kernel_tbps": round(corpus_bytes / kern / 1e9, 3), "count_only_ms": cnt,
                       "kmeans_iteration_ms": km, "kmeans_over_pass": round(km / ps, 2), "host_ms_at_host_rows": host,
                       "host_ms_scaled_to_n": host_n, "host_over_call": round(host_n / call, 1), "max_rel_err_vs_host": err}
        lines.append(f"{dtype:5s} {c:5d} {call:9.3f} {kern:9.3f} {ps:9.3f} {kern / ps:7.2f} {call / ps:7.2f} {corpus_bytes / kern / 1e9:6.2f} "
                     f"{cnt:9.3f} {km:9.3f} {km / ps:7.2f} {host:10.1f} {host_n:11.1f} {host_n / call:8.1f}")
        print(f"[label_sums_time] {lines[-1]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
head = [
    "Per-label row sums: DeviceIndex.label_sums(arange(c), row_labels=random labels) over the whole index (c x d f64 sums and the counts",
    "back, 4 bytes of label per row up) against (i) its chunk-sum and fold kernels alone from HIP events, (ii) the score kernel of one",
    "single-query search of the same index (unscreened: the corpus read once, the HBM-read floor), (iii) a count-only call, (iv) one k-means",
    "iteration (kmeans(c, iterations=1, init=...): one assign + one label_sums) and (v) the host alternative, stored_rows() + a numpy f64 reduction",
    f"per label, measured at {host_rows} rows and scaled linearly to n (tools/label_sums_time.py, MI355X, one process, the calls alternating).",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls ((i): of 5; (iv), (v): of {slow_reps}), csrc_sha16 {out['csrc_sha16']}",
    "times in ms.  k/(ii), call/(ii), km/(ii): the kernels, the whole call and the k-means iteration over the corpus pass.  (v)/call: the host",
    "alternative (scaled to n) over the call.",
    "",
    f"{'dtype':5s} {'c':>5s} {'call':>9s} {'(i) kern':>9s} {'(ii) pass':>9s} {'k/(ii)':>7s} {'call/(ii)':>7s} {'TB/s':>6s} {'(iii) cnt':>9s} {'(iv) km':>9s} "
    f"{'km/(ii)':>7s} {'(v) host':>10s} {'(v) at n':>11s} {'(v)/call':>8s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)
