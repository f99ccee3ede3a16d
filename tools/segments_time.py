#!/usr/bin/env python3
"""Segmented filtered search (svs_index_search_segments): host-call time of DeviceIndex.search_segments over many row
lists of a 1M x 1536 corpus, beside -- in the same process, alternating call by call --
  loop   the loop of DeviceIndex.search_within over the same lists (what the segmented call replaces), and
  union  ONE search_within over the union of the lists (the same listed bytes: the floor).
Shapes: (segments x rows per segment) of random rows; `one query` for all segments (the drill-down) and one query per
segment (per-request scopes).  Prints one JSON line: per dtype and shape the medians in ms, the loop's run-to-run spread
(its 25th-75th percentile range), loop / segmented and segmented / union, and the listed-row bytes.  Under
`rocprofv3 --kernel-trace --stats` the two kernels' time per launch comes from the trace (pass reps=3 then).
  usage: segments_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=30] [shapes=256x400,64x1600,1024x100,16x20000]"""
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
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
k = 10
SHAPES = [tuple(int(x) for x in s.split("x")) for s in
          (sys.argv[5] if len(sys.argv) > 5 else "256x400,64x1600,1024x100,16x20000").split(",")]


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(12)
rng = np.random.default_rng(12)
out = {"n": n, "d": d, "k": k, "csrc_sha16": csrc_sha16(), "reps": reps}
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    row_bytes = idx.ld * {"f32": 4, "f16": 2, "fp8": 1}[dtype]
    res = {"row_bytes": row_bytes}
    for nseg, m in SHAPES:
        lists = [np.sort(rng.choice(n, m, replace=False)) for _ in range(nseg)]
        union = np.unique(np.concatenate(lists))
        Q = torch.randn((nseg, d), device=dev, generator=g)
        Q = (Q / Q.norm(dim=1, keepdim=True)).cpu().numpy()
        for mode in ("one_query", "query_per_segment"):
            if mode == "one_query":
                qs, sq = Q[:1], [0] * nseg
            else:
                qs, sq = Q, None
            calls = {
                "segments": lambda: idx.search_segments(qs, k, lists, sq),
                "loop": lambda: [idx.search_within(qs[0 if sq else s], k, lists[s]) for s in range(nseg)],
                "union": lambda: idx.search_within(qs[0], k, union),
            }
            for fn in calls.values():   # warm: scratch grown, kernels loaded
                fn()
            t = {name: [] for name in calls}
            for _ in range(reps):       # alternating, so that drift hits all three alike
                for name, fn in calls.items():
                    t[name].append(timed(fn))
            med = {name: float(np.median(v)) for name, v in t.items()}
            q25, q75 = np.percentile(t["loop"], [25, 75])
            rec = {"listed_bytes": nseg * m * row_bytes, "union_rows": int(len(union)),
                   "segments_ms": round(med["segments"], 4), "loop_ms": round(med["loop"], 4), "union_ms": round(med["union"], 4),
                   "loop_spread_ms": round(float(q75 - q25), 4),
                   "segments_spread_ms": round(float(np.subtract(*np.percentile(t["segments"], [75, 25]))), 4),
                   "loop_over_segments": round(med["loop"] / med["segments"], 2),
                   "segments_over_union": round(med["segments"] / med["union"], 2)}
            res[f"{nseg}x{m}_{mode}"] = rec
            print(f"[segments_time] {dtype} {nseg} x {m} {mode}: {rec}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
print(json.dumps(out), flush=True)
