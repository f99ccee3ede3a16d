#!/usr/bin/env python3
"""Nearest-vector assignment (svs_index_assign): host-call time of DeviceIndex.assign over a 1M x 1536 corpus built on the
device, for c = 16, 64, 256 and 1,024 vectors, with and without the write of the label column, beside -- in the same
process, the calls alternating --
  (i)   swap     the role-swapped alternative, what a caller can do without the entry: a c-row DeviceIndex of the same
                 dtype, the stored rows read out (``stored_rows``) and pushed back as host queries,
                 ``search_batch(block, 1)`` in blocks of 65,536 rows.  The read-out is included, and also reported alone.
  (ii)  scores   one ``scores()`` pass of the same index: the corpus read once, the HBM floor.
  (iii) compute  2 n ld c FLOP at 155 TFLOP/s, the f32-MFMA rate: the compute floor (no call: arithmetic).
  (iv)  kernel   assign_rows_kernel alone, from HIP events around it (svs_index_set_timing), in calls of their own: its
                 time, the useful TFLOP/s (2 n ld c FLOP) and the corpus bytes per second (n ld bytes, read once).
Statistic: the p50 of ``reps`` warmed calls ((i): of ``swap_reps`` calls -- each moves the whole corpus over PCIe twice).
The tool checks ONE condition: at every (dtype, c) both modes of assign are faster than (i).  It also checks that the
swap's positions agree with assign's on at least 99 % of the rows (the two accumulate in different orders and break ties
differently: near ties may fall either way).
Writes a table and one JSON line.
  usage: assign_time.py [n=1000000] [d=1536] [dtypes=f32,f16,fp8] [reps=20] [swap_reps=3] [out=profiles/assign_time.txt]"""
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
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
swap_reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
out_path = sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "assign_time.txt")
CS = [16, 64, 256, 1024]
BLOCK = 65_536
MFMA_F32_TFLOPS = 155.0
ESZ = {"f32": 4, "f16": 2, "fp8": 1}
lib = _native.load()


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def p50(v):
    return round(float(np.percentile(v, 50)), 4)


def kernel_ms(idx, vecs):
    """assign_rows_kernel alone: the HIP events of one timed call."""
    idx.set_timing(1)
    try:
        idx.assign(vecs)
        ms = C.c_double(-1.0)
        _native.check(lib.svs_internal_assign_kernel_ms(C.byref(ms)))
    finally:
        idx.set_timing(0)
    assert ms.value > 0, "no kernel time was recorded"
    return ms.value


def swap(idx, small, parts):
    """(i): every stored row as a host query against the c-row index; parts gets the read-out's share."""
    a = time.perf_counter()
    rows = idx.stored_rows()
    parts.append((time.perf_counter() - a) * 1e3)
    best = np.empty(len(rows), dtype=np.int64)
    for r0 in range(0, len(rows), BLOCK):
        best[r0:r0 + BLOCK] = small.search_batch(rows[r0:r0 + BLOCK], 1)[1][:, 0]
    return best


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(17)
out = {"n": n, "d": d, "csrc_sha16": csrc_sha16(), "reps": reps, "swap_reps": swap_reps, "mfma_f32_tflops": MFMA_F32_TFLOPS}
lines, failed = [], []
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    pool = torch.randn((max(CS), d), device=dev, generator=g)
    pool = (pool / pool.norm(dim=1, keepdim=True)).cpu().numpy()
    q = pool[0]
    ld = idx.ld
    corpus_bytes = n * ld * ESZ[dtype]
    res = {}
    for c in CS:
        vecs = np.ascontiguousarray(pool[:c])
        labels = np.arange(c, dtype=np.uint32) + 1
        small = DeviceIndex(vecs, dtype=dtype)
        # the answers agree (and every call is warm afterwards)
        best, sc, counts = idx.assign(vecs)
        b2, _, c2 = idx.assign(vecs, labels=labels)
        assert np.array_equal(best, b2) and np.array_equal(counts, c2) and int(counts.sum()) == n
        idx.scores(q)
        small.search_batch(vecs[:2], 1)
        swapped = []
        times = {"assign": [], "assign_labels": [], "scores": [], "swap": []}
        parts = []
        for rep in range(reps):       # alternating, so that drift hits all alike
            times["assign"].append(timed(lambda: idx.assign(vecs)))
            times["assign_labels"].append(timed(lambda: idx.assign(vecs, labels=labels)))
            times["scores"].append(timed(lambda: idx.scores(q)))
            if rep < swap_reps:
                times["swap"].append(timed(lambda: swapped.append(swap(idx, small, parts))))
                idx.assign(vecs)      # (untimed: the GPU idled while the host moved rows)
        agree = float((swapped.pop() == best).mean())
        del swapped
        assert agree >= 0.99, f"{dtype} c={c}: the role-swapped search agrees on {agree:.5f} of the rows"
        kern = p50([kernel_ms(idx, vecs) for _ in range(5)])
        small.release()
        a, al, s, sw, ro = p50(times["assign"]), p50(times["assign_labels"]), p50(times["scores"]), p50(times["swap"]), p50(parts)
        flop = 2.0 * n * ld * c
        comp = round(flop / (MFMA_F32_TFLOPS * 1e12) * 1e3, 4)
        nearer = "HBM" if s >= comp else "compute"      # (the larger floor is the nearer one)
        ok = a < sw and al < sw
        if not ok:
            failed.append(f"{dtype} c={c}")
        res[str(c)] = {"assign_ms": a, "assign_labels_ms": al, "swap_ms": sw, "swap_readout_ms": ro, "scores_ms": s, "compute_floor_ms": comp,
                       "kernel_ms": kern, "kernel_tflops": round(flop / kern / 1e9, 2), "kernel_tbps": round(corpus_bytes / kern / 1e9, 3),
                       "kernel_over_scores": round(kern / s, 2), "kernel_over_compute": round(kern / comp, 2), "nearer_floor": nearer,
                       "swap_over_assign": round(sw / a, 1), "swap_agreement": round(agree, 6), "faster_than_swap": ok}
        lines.append(f"{dtype:5s} {c:5d} {a:9.3f} {al:9.3f} {sw:10.1f} {ro:10.1f} {s:8.3f} {comp:8.3f} {kern:9.3f} {flop / kern / 1e9:7.1f} "
                     f"{corpus_bytes / kern / 1e9:6.2f} {kern / s:7.2f} {kern / comp:7.2f} {nearer:>7s} {sw / a:8.1f}")
        print(f"[assign_time] {lines[-1]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
out["condition_assign_faster_than_swap"] = not failed
out["condition_failed_at"] = failed
head = [
    "Nearest-vector assignment: DeviceIndex.assign over the whole index (best, scores and counts back; 'labels': also the write of the label",
    "column) against (i) the role-swapped alternative -- a c-row index of the same dtype searched with search_batch(stored_rows block, 1) in",
    "blocks of 65,536 rows, the stored_rows() read-out included and also shown alone -- (ii) one scores() pass of the same index (the HBM floor:",
    "the corpus read once), (iii) the compute floor 2 n ld c FLOP at 155 TFLOP/s (f32 MFMA), and (iv) assign_rows_kernel alone from HIP events:",
    "its time, useful TFLOP/s and corpus TB/s (tools/assign_time.py, MI355X, one process, the calls alternating).",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls ((i): of {swap_reps}; (iv): of 5), csrc_sha16 {out['csrc_sha16']}",
    "times in ms.  k/(ii), k/(iii): the kernel over each floor; nearer: the floor the kernel sits nearer to.  (i)/a: the alternative over assign.",
    f"condition (assign, with and without labels, faster than (i) at every point): {'holds' if not failed else 'FAILS at ' + ', '.join(failed)}",
    "",
    f"{'dtype':5s} {'c':>5s} {'assign':>9s} {'labels':>9s} {'(i) swap':>10s} {'(read-out)':>10s} {'(ii) scr':>8s} {'(iii) cmp':>8s} {'(iv) kern':>9s} {'TFLOP/s':>7s} "
    f"{'TB/s':>6s} {'k/(ii)':>7s} {'k/(iii)':>7s} {'nearer':>7s} {'(i)/a':>8s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)
sys.exit(0 if not failed else 1)
