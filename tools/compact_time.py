#!/usr/bin/env python3
"""In-place compaction (svs_index_compact) against what it replaces and against the copy roofline.  A figure, no gate.

Cases, each run once on a 1M x 1536 index built from device blocks:
  f32 (with its half shadow), 25 % random rows dead;  the same in f16;  f32 with ONE dead row at row 0 -- every step
  goes through the bounce buffer, the worst case.
Per case: the time of compact(); bytes moved per second beside a hipMemcpy device-to-device copy of the same byte
count in the same process (the yardstick: it reads and writes each byte once, like a DIRECT step); the single-query
search time before (tombstones in place) and after.  Last, the rebuild from SQLite that the KB mirror used to do
instead (tools/kb_latency.py's cold start) at a row count that can be inserted in reasonable time, as seconds per
million rows.  Run on the GPU box:  python tools/compact_time.py [rows] [sqlite_rows]"""
import ctypes as C
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import svs_amd
from svs_amd import DeviceIndex, _native

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
N_SQL = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000
D, BLOCK = 1536, 50_000


def hip_runtime():
    _native.load()
    for name in (os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"), "libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("no HIP runtime to call hipMemcpy through")


def d2d_seconds(hip, nbytes):
    """hipMemcpy device-to-device of nbytes, second of two runs."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.fill_(1)
    best = None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = hip.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(nbytes), 3)
        hip.hipDeviceSynchronize()
        best = time.perf_counter() - t0
        assert rc == 0, rc
    del src, dst
    torch.cuda.empty_cache()
    return best


def build(dtype):
    idx = DeviceIndex.empty(D, device=0, dtype=dtype, reserve=N)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for r0 in range(0, N, BLOCK):
        rows = min(BLOCK, N - r0)
        t = torch.randn((rows, D), device="cuda", generator=g)
        t /= t.norm(dim=1, keepdim=True)
        idx.append_device(t.data_ptr(), rows)
    return idx


def query_ms(idx, q):
    idx.search(q, 100)
    lat = []
    for _ in range(30):
        t0 = time.perf_counter()
        idx.search(q, 100)
        lat.append(time.perf_counter() - t0)
    return float(np.median(lat)) * 1e3


def case(hip, name, dtype, dead):
    idx = build(dtype)
    q = np.random.default_rng(2).standard_normal(D).astype(np.float32)
    q /= np.linalg.norm(q)
    idx.mask_rows(dead)
    before = query_ms(idx, q)
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    row_map = idx.compact(stats=stats)
    dt = time.perf_counter() - t0
    assert len(row_map) == N - len(dead) == idx.n
    after = query_ms(idx, q)
    idx.release()
    torch.cuda.empty_cache()
    moved = stats[3]
    copy = d2d_seconds(hip, moved) if moved else float("nan")
    print(f"{name}: n={N} d={D} {dtype}, {len(dead)} dead rows -> compact() {dt * 1e3:.2f} ms "
          f"({stats[0]} DIRECT + {stats[1]} BOUNCE steps, {stats[2]} rows, {moved / 1e9:.3f} GB moved = {moved / dt / 1e12:.3f} TB/s; "
          f"hipMemcpy D2D of the same bytes {copy * 1e3:.2f} ms = {moved / copy / 1e12:.3f} TB/s; ratio {copy / dt:.2f}); "
          f"single query {before:.3f} ms with tombstones -> {after:.3f} ms compacted", flush=True)


def rebuild_rate():
    from svs_amd.kb import embedding_to_bytes
    rng = np.random.default_rng(3)

    async def ef(texts):
        raise AssertionError("no embedding call expected")

    with tempfile.TemporaryDirectory() as td:
        kb = svs_amd.KB(os.path.join(td, "kb.sqlite"), ef)
        with kb.db.transaction():
            for r0 in range(0, N_SQL, 10_000):
                v = rng.standard_normal((min(10_000, N_SQL - r0), D))
                v /= np.linalg.norm(v, axis=1, keepdims=True)
                for row in v.astype(np.float32):
                    kb.db.set_doc_embedding(kb.db.add_doc("x", None, None), embedding_to_bytes(row))
        t0 = time.perf_counter()
        kb.load()
        dt = time.perf_counter() - t0
        assert kb.embeddings_matrix.index.n == N_SQL
        kb.close()
    print(f"rebuild from SQLite (cold start, the path compaction replaces): {dt:.3f} s for {N_SQL} rows x {D} "
          f"= {dt / N_SQL * 1e6:.2f} s per million rows", flush=True)


if __name__ == "__main__":
    hip = hip_runtime()
    quarter = np.sort(np.random.default_rng(4).choice(N, N // 4, replace=False))
    case(hip, "f32+shadow, 25% dead", "f32", quarter)
    case(hip, "f16, 25% dead", "f16", quarter)
    case(hip, "f32+shadow, row 0 dead (all BOUNCE)", "f32", np.array([0]))
    rebuild_rate()
