#!/usr/bin/env python3
"""Neighbours of stored rows (svs_index_neighbors): host-call time per block of 1024 source rows, beside what a caller
could do for the same answer without it, in ONE process on ONE index:
  (A) idx.neighbors(block, k)
  (B) idx.search_batch(idx.stored_rows(r0, 1024), k + 1) plus the numpy self-removal (rows pulled out with
      svs_index_debug_dequant, pushed back as host queries, self stripped on the host).
After a warm-up the two alternate A, B, A, B, ... in runs of `blocks` consecutive blocks (at least 3 alternations);
medians and min-max over all timed blocks of each side.  Prints one JSON line, with the projected whole-graph time
n / 1024 x A.  `graph=1` also times ONE idx.neighbors call over all n rows (outputs: n x k x 12 bytes of host memory).
  usage: neighbors_time.py [n=1000000] [d=1536] [dtype=f16] [k=100] [alternations=3] [blocks=20] [graph=0]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from svs_amd import DeviceIndex
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
dtype = sys.argv[3] if len(sys.argv) > 3 else "f16"
k = int(sys.argv[4]) if len(sys.argv) > 4 else 100
alternations = max(int(sys.argv[5]) if len(sys.argv) > 5 else 3, 3)
blocks = int(sys.argv[6]) if len(sys.argv) > 6 else 20
graph = bool(int(sys.argv[7])) if len(sys.argv) > 7 else False
BLOCK = 1024

dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(17)
idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
for r0 in range(0, n, 250_000):
    rows = min(250_000, n - r0)
    v = torch.randn((rows, d), device=dev, generator=g)
    v /= v.norm(dim=1, keepdim=True)
    idx.append_device(v.contiguous().data_ptr(), rows)
    del v
torch.cuda.synchronize()
torch.cuda.empty_cache()


def side_a(r0):
    return idx.neighbors(np.arange(r0, r0 + BLOCK), k)


def side_b(r0):
    s, r = idx.search_batch(idx.stored_rows(r0, BLOCK), k + 1)
    src = np.arange(r0, r0 + BLOCK)[:, None]
    keep = r != src
    keep[keep.all(axis=1), -1] = False          # self absent: drop the last entry
    return s[keep].reshape(BLOCK, k), r[keep].reshape(BLOCK, k)


starts = [(i * BLOCK) % max(n - BLOCK, 1) for i in range(alternations * blocks)]
# warm-up: buffers grown, and the two sides agree
for r0 in starts[:2]:
    (sa, ra), (sb, rb) = side_a(r0), side_b(r0)
    assert np.array_equal(ra, rb) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), "A and B disagree"
t = {"A": [], "B": []}
for a in range(alternations):
    for name, fn in (("A", side_a), ("B", side_b)):
        for r0 in starts[a * blocks:(a + 1) * blocks]:
            t0 = time.perf_counter()
            fn(r0)
            t[name].append(time.perf_counter() - t0)


def stats(x):
    x = np.array(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)}


out = {"n": n, "d": d, "dtype": dtype, "k": k, "block": BLOCK, "alternations": alternations, "blocks_per_run": blocks,
       "csrc_sha16": csrc_sha16(), "A_neighbors": stats(t["A"]), "B_search_batch_of_stored_rows": stats(t["B"])}
out["graph_projected_s"] = round(n / BLOCK * out["A_neighbors"]["median_ms"] / 1e3, 3)
if graph:
    t0 = time.perf_counter()
    s, r = idx.neighbors(np.arange(n), k)
    out["graph_measured_s"] = round(time.perf_counter() - t0, 3)
    assert r.shape == (n, k) and not (r == np.arange(n)[:, None]).any()
idx.release()
print(json.dumps(out), flush=True)
