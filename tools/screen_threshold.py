"""Screened against unscreened single-query search, same process, same index, interleaved: the table behind
SCREEN_MIN_ROWS (svs_amd/csrc/svs_amd.hip; DESIGN.md, "Screened search").

    python tools/screen_threshold.py [--dims 512,1536,3072,4096] [--rows 8192,...,1000000] [--rounds 5] [--queries 200]

Per (d, n): unit Gaussian rows generated on the device, `queries` distinct queries enqueued back to back through
svs_index_search_device (top-100) and drained once; `rounds` rounds of variant 11 (never screen) and variant 12
(always screen) alternate.  Prints the median and the spread (max - min) of the per-query time of each, in us."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from svs_amd import DeviceIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="512,1536,3072,4096")
    ap.add_argument("--rows", default="8192,16384,32768,65536,131072,262144,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--k", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"{'d':>5} {'n':>8} {'off us':>9} {'spread':>7} {'on us':>9} {'spread':>7} {'on/off':>7}")
    for d in [int(x) for x in args.dims.split(",")]:
        for n in [int(x) for x in args.rows.split(",")]:
            if n * d * 4 > (12 << 30):
                continue
            g = torch.Generator(device=dev)
            g.manual_seed(n + d)
            rows = torch.randn((n, d), device=dev, generator=g)
            rows /= rows.norm(dim=1, keepdim=True)
            idx = DeviceIndex.from_device_pointer(rows.data_ptr(), n, d, device=0)
            del rows
            qs = torch.randn((args.queries, d), device=dev, generator=g)
            qs /= qs.norm(dim=1, keepdim=True)
            out_s = torch.empty((args.queries, args.k), device=dev)
            out_r = torch.empty((args.queries, args.k), device=dev, dtype=torch.int64)
            st = torch.cuda.current_stream().cuda_stream
            t = {11: [], 12: []}
            for rnd in range(args.rounds + 1):          # (round 0 warms both up)
                for variant in (11, 12):
                    idx.set_variant(variant)
                    torch.cuda.synchronize()
                    a = time.perf_counter()
                    for j in range(args.queries):
                        idx.search_device(qs[j].data_ptr(), 1, d, args.k, out_s[j].data_ptr(), out_r[j].data_ptr(), stream=st)
                    torch.cuda.synchronize()
                    if rnd:
                        t[variant].append((time.perf_counter() - a) / args.queries * 1e6)
            off, on = np.array(t[11]), np.array(t[12])
            print(f"{d:>5} {n:>8} {np.median(off):>9.1f} {off.max() - off.min():>7.1f} {np.median(on):>9.1f} "
                  f"{on.max() - on.min():>7.1f} {np.median(on) / np.median(off):>7.3f}", flush=True)
            idx.release()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
