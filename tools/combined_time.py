#!/usr/bin/env python3
"""Combined search (svs_index_search_combined): host-call time of DeviceIndex.search_batch_combined for ONE combined query
(op max, k = 100) of m = 1, 2, 4, 8 vectors over a 1M x 1536 corpus built on the device, per dtype, in one process, the
calls alternating call by call:
  (a) fused    the fused route (svs_internal_tune(8, 1)): one corpus pass, one selection
  (b) passes   the same call forced onto the m-passes route (svs_internal_tune(8, 2)): m single-query passes + combine
  (c) single   DeviceIndex.search_batch of ONE query, k = 100, under variant 11 (never screened): one plain pass
  (d) host     the alternative without the entry: m x DeviceIndex.scores + numpy maximum + argpartition
Every call ends in the library's own stream synchronise.  Writes a table -- p50 in ms, the 25th-75th percentile spread,
(a)/(b) and (a)/(c) -- and one JSON line.
  usage: combined_time.py [n=1000000] [d=1536] [dtypes=f32,f16,fp8] [reps=30] [out=profiles/combined_time.txt]"""
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
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "combined_time.txt")
K = 100
MS = [1, 2, 4, 8]
lib = _native.load()


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def routed(route, fn):
    def call():
        assert lib.svs_internal_tune(8, route) == 0
        try:
            return fn()
        finally:
            assert lib.svs_internal_tune(8, 0) == 0
    return call


def host_alternative(idx, vecs, k):
    s = idx.scores(vecs[0])
    for v in vecs[1:]:
        s = np.maximum(s, idx.scores(v))
    top = np.argpartition(s, s.size - k)[-k:]
    top = top[np.lexsort((top, s[top]))[::-1]]
    return s[top], top


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(15)
out = {"n": n, "d": d, "k": K, "csrc_sha16": csrc_sha16(), "reps": reps, "device": torch.cuda.get_device_name(0)}
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
    idx.set_variant(11)   # (c) unscreened, as a combined search always is: the same rows are read in all four
    q = torch.randn((8, d), device=dev, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    calls = {"single_1": lambda: idx.search_batch(q[:1], K)}
    for m in MS:
        calls[f"fused_{m}"] = routed(1, lambda m=m: idx.search_batch_combined(q[None, :m], K, "max"))
        calls[f"passes_{m}"] = routed(2, lambda m=m: idx.search_batch_combined(q[None, :m], K, "max"))
        calls[f"host_{m}"] = lambda m=m: host_alternative(idx, q[:m], K)
    for m in MS:          # the three agree (and the calls are warm afterwards)
        s1, r1, _ = calls[f"fused_{m}"]()
        assert [e[0][:9] for e in _native.last_launches()] == ["combine_f"], _native.last_launches()
        s2, r2, _ = calls[f"passes_{m}"]()
        assert _native.last_launches()[-1][0] == "combine_scores_kernel", _native.last_launches()
        s3, r3 = calls[f"host_{m}"]()
        assert r1[0].tolist() == r2[0].tolist() == r3.tolist() and s1[0].tolist() == s2[0].tolist() == s3.tolist(), (dtype, m)
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(reps):       # alternating, so that drift hits all alike
        for name, fn in calls.items():
            times[name].append(timed(fn))
    res = {}
    for name, v in times.items():
        q25, q50, q75 = np.percentile(v, [25, 50, 75])
        res[name] = {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4)}
        print(f"[combined_time] {dtype} {name}: {res[name]}", file=sys.stderr, flush=True)
    single = res["single_1"]["p50_ms"]
    lines.append(f"{dtype:5s} {'-':>2s} {'':>9s} {'':>9s} {single:9.4f} {'':>9s} {'':>8s} {'':>8s}")
    for m in MS:
        a, b, h = res[f"fused_{m}"]["p50_ms"], res[f"passes_{m}"]["p50_ms"], res[f"host_{m}"]["p50_ms"]
        sp = max(res[f"fused_{m}"]["spread_ms"], res[f"passes_{m}"]["spread_ms"])
        lines.append(f"{dtype:5s} {m:2d} {a:9.4f} {b:9.4f} {'':>9s} {h:9.4f} {a / b:8.3f} {a / single:8.3f}   (spread {sp:.4f})")
    out[dtype] = res
    idx.release()
head = [
    "Combined search: DeviceIndex.search_batch_combined, one combined query of m vectors, op max, k = 100 (tools/combined_time.py,",
    f"MI355X -- torch names it '{out['device']}' --, one process, the calls alternating call by call).  (a) the fused route; (b) the same call forced onto m",
    "single-query passes + combine_scores_kernel; (c) search_batch of one query under variant 11 (one plain unscreened pass);",
    "(d) m x DeviceIndex.scores + numpy maximum + argpartition on the host.",
    f"n = {n}, d = {d}, p50 of {reps} warmed host calls (each ends in a stream synchronise), csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the calls, the larger of (a)'s and (b)'s.  times in ms.",
    "",
    f"{'dtype':5s} {'m':>2s} {'(a) fused':>9s} {'(b) pass.':>9s} {'(c) single':>9s} {'(d) host':>9s} {'(a)/(b)':>8s} {'(a)/(c)':>8s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print("\n".join(head + lines), flush=True)
print(json.dumps(out), flush=True)
