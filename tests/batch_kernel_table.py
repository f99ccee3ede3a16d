"""The batched score kernels and the shapes that reach them: plain data, importable without a GPU.

One row per case: (dtype, d, n, nq, k, form, kernel).  `kernel` is the kernel of the MAIN pass (the launch over all n
rows) as svs_internal_last_launches and c++filt spell it; "gemv" is the per-query loop of the single-query kernels.
`form`:
  * "materialised": search_batch(Q, k = n) -- full ranking, never fused; the whole (nq, n) score matrix is checked
    against f64 (tests/test_batch_kernels_gpu.py);
  * "materialised+norms": the same, on a corpus whose row norms span 1e-2 .. 1e2 (relative bound);
  * "fused": the fused top-k epilogue (n >= 131,072, nq >= 16, k <= 256) on a corpus with planted rows in every tile.

The dispatch rules these rows follow (svs_amd/csrc/svs_amd.hip: batch_route decides family, query tile and staging once
per call; launch_batch, launch_q16, launch_tiled_eb and phased_ok pick each pass's kernel from that route; plan_search
decides fused or not; tests/test_batch_route.py asks the same dispatch for these names without a device):
  * f32: 2-16 queries and ld % 128 == 0, ld <= 2304 -> gemm_q16r_kernel<F, 4, ...>; otherwise 17-32 queries -> the
    tiled kernel at 32-query tiles, more -> 64-query tiles; rows that are not whole 128-byte lines -> gemv.
  * f16: 2-16 queries and ld % 256 == 0, ld <= 4608 -> gemm_q16r_kernel<F, 2, ...>; otherwise tiled at 32 / 64 queries;
    65-128 queries -> gemm_phased_kernel<., 2, ., 128> when a row is an even number (>= 6) of 128-byte k-tiles, else
    gemm_tiled_kernel<128, ., 2, 256>; more -> gemm_phased_kernel<., 2, ., 256> / gemm_tiled_kernel<256, ., 2, 256>.
  * fp8: as f16 without the 16-query kernel (EB = 1).
  * fused phased, 256-query tiles: EXP 20 for at most 256 queries (one query tile), EXP 0 beyond.

choose_ld pads rows: f32 d = 2305 -> ld 2560, d = 1100 -> 1120; f16 d = 4609 -> 5120, d = 100 -> 104; fp8 d = 100 -> 112.
"""

MAT, NORMS, FUSED = "materialised", "materialised+norms", "fused"

Q16_F32 = "gemm_q16r_kernel<{}, 4, 4, 2>"
Q16_F16 = "gemm_q16r_kernel<{}, 2, 4, 2>"


def _q16(dtype, fused):
    return (Q16_F32 if dtype == "f32" else Q16_F16).format("true" if fused else "false")


def _tiled(bn, fused, eb, bm):
    return f"gemm_tiled_kernel<{bn}, {'true' if fused else 'false'}, {eb}, {bm}>"


def _phased(fused, eb, exp, qt):
    return f"gemm_phased_kernel<{'true' if fused else 'false'}, {eb}, {exp}, {qt}>"


# fused corpora: 131,329 rows = 514 row tiles (the last holds one row); 162,500 rows = 635 row tiles = 5 x 127 (the
# scattered tile order of the fused kernels steps by a prime that does not divide the tile count: 31 here, not 127)
NF1, NF2 = 131_329, 162_500

CASES = [
    # ---- f32 ----------------------------------------------------------------------------------------------------
    ("f32", 128, 1, 2, 1, MAT, _q16("f32", False)),                 # one row
    ("f32", 1536, 255, 15, 255, MAT, _q16("f32", False)),           # fewer rows than one tile
    ("f32", 2304, 4097, 16, 4097, MAT, _q16("f32", False)),         # the longest q16 row; n % 256 == 1
    ("f32", 128, 5119, 17, 5119, MAT, _tiled(32, False, 4, 128)),   # n % 256 == 255
    ("f32", 1536, 3000, 32, 3000, MAT, _tiled(32, False, 4, 128)),
    ("f32", 2305, 2000, 2, 2000, MAT, _tiled(32, False, 4, 128)),   # ld 2560: past the q16 kernel's LDS
    ("f32", 1100, 2000, 16, 2000, MAT, _tiled(32, False, 4, 128)),  # ld 1120: not a whole 128-float step
    ("f32", 128, 3001, 33, 3001, MAT, _tiled(64, False, 4, 128)),
    ("f32", 1536, 2000, 65, 2000, MAT, _tiled(64, False, 4, 128)),
    ("f32", 128, 1500, 257, 1500, MAT, _tiled(64, False, 4, 128)),  # five query tiles, the last with one query
    ("f32", 100, 1000, 3, 1000, MAT, "gemv"),                       # ld 100: no batched kernel
    ("f32", 1536, 3000, 16, 3000, NORMS, _q16("f32", False)),
    # ---- f16 ----------------------------------------------------------------------------------------------------
    ("f16", 256, 1, 2, 1, MAT, _q16("f16", False)),
    ("f16", 512, 4097, 16, 4097, MAT, _q16("f16", False)),
    ("f16", 4608, 1500, 15, 1500, MAT, _q16("f16", False)),         # the longest q16 row
    ("f16", 256, 3000, 17, 3000, MAT, _tiled(32, False, 2, 128)),
    ("f16", 1664, 2000, 2, 2000, MAT, _tiled(32, False, 2, 128)),   # ld 1664: odd number of 256-byte steps
    ("f16", 4609, 1000, 16, 1000, MAT, _tiled(32, False, 2, 128)),  # ld 5120: past the q16 kernel's LDS
    ("f16", 448, 5119, 33, 5119, MAT, _tiled(64, False, 2, 128)),
    ("f16", 640, 3000, 64, 3000, MAT, _tiled(64, False, 2, 128)),
    ("f16", 256, 3000, 65, 3000, MAT, _tiled(128, False, 2, 256)),  # 4 k-tiles: not the phased kernel's
    ("f16", 448, 2000, 128, 2000, MAT, _tiled(128, False, 2, 256)),  # 7 k-tiles (odd)
    ("f16", 256, 2000, 129, 2000, MAT, _tiled(256, False, 2, 256)),
    ("f16", 448, 1000, 257, 1000, MAT, _tiled(256, False, 2, 256)),
    ("f16", 512, 3000, 65, 3000, MAT, _phased(False, 2, 0, 128)),   # 8 k-tiles
    ("f16", 640, 255, 128, 255, MAT, _phased(False, 2, 0, 128)),    # 10 k-tiles, fewer rows than one tile
    ("f16", 384, 40001, 513, 40001, MAT, _phased(False, 2, 0, 256)),  # 6 k-tiles; 157 x 3 output tiles: > CUs, no multiple
    ("f16", 4608, 2000, 129, 2000, MAT, _phased(False, 2, 0, 256)),   # 72 k-tiles
    ("f16", 1664, 4097, 256, 4097, MAT, _phased(False, 2, 0, 256)),   # 26 k-tiles
    ("f16", 4609, 1000, 257, 1000, MAT, _phased(False, 2, 0, 256)),   # ld 5120: 80 k-tiles
    ("f16", 100, 1000, 3, 1000, MAT, "gemv"),                         # ld 104
    # ---- fp8 ----------------------------------------------------------------------------------------------------
    ("fp8", 128, 1, 2, 1, MAT, _tiled(32, False, 1, 128)),
    ("fp8", 256, 4097, 16, 4097, MAT, _tiled(32, False, 1, 128)),
    ("fp8", 3072, 1000, 32, 1000, MAT, _tiled(32, False, 1, 128)),
    ("fp8", 896, 3000, 33, 3000, MAT, _tiled(64, False, 1, 128)),
    ("fp8", 1024, 2000, 64, 2000, MAT, _tiled(64, False, 1, 128)),
    ("fp8", 128, 5119, 65, 5119, MAT, _tiled(128, False, 1, 256)),  # 1 k-tile
    ("fp8", 896, 255, 128, 255, MAT, _tiled(128, False, 1, 256)),   # 7 k-tiles (odd)
    ("fp8", 256, 3000, 129, 3000, MAT, _tiled(256, False, 1, 256)),  # 2 k-tiles
    ("fp8", 896, 1000, 513, 1000, MAT, _tiled(256, False, 1, 256)),
    ("fp8", 768, 3000, 65, 3000, MAT, _phased(False, 1, 0, 128)),   # 6 k-tiles
    ("fp8", 1024, 4097, 128, 4097, MAT, _phased(False, 1, 0, 128)),  # 8 k-tiles
    ("fp8", 1280, 2000, 129, 2000, MAT, _phased(False, 1, 0, 256)),  # 10 k-tiles
    ("fp8", 4096, 2000, 256, 2000, MAT, _phased(False, 1, 0, 256)),  # 32 k-tiles
    ("fp8", 768, 20001, 257, 20001, MAT, _phased(False, 1, 0, 256)),  # 6 k-tiles, two query tiles
    ("fp8", 100, 1000, 3, 1000, MAT, "gemv"),                         # ld 112
    ("fp8", 1024, 3000, 129, 3000, NORMS, _phased(False, 1, 0, 256)),
    # ---- fused top-k epilogue -------------------------------------------------------------------------------------
    ("f32", 128, NF1, 16, 256, FUSED, _q16("f32", True)),
    ("f32", 128, NF1, 17, 256, FUSED, _tiled(32, True, 4, 128)),
    ("f32", 128, NF1, 65, 64, FUSED, _tiled(64, True, 4, 128)),
    ("f16", 256, NF2, 16, 256, FUSED, _q16("f16", True)),
    ("f16", 256, NF2, 17, 256, FUSED, _tiled(32, True, 2, 128)),
    ("f16", 256, NF2, 33, 128, FUSED, _tiled(64, True, 2, 128)),
    ("f16", 256, NF2, 65, 64, FUSED, _tiled(128, True, 2, 256)),
    ("f16", 256, NF2, 300, 64, FUSED, _tiled(256, True, 2, 256)),
    ("f16", 384, NF2, 65, 64, FUSED, _phased(True, 2, 20, 128)),
    ("f16", 384, NF2, 129, 64, FUSED, _phased(True, 2, 20, 256)),
    ("f16", 384, NF2, 257, 64, FUSED, _phased(True, 2, 0, 256)),
    ("fp8", 256, NF1, 16, 256, FUSED, _tiled(32, True, 1, 128)),
    ("fp8", 256, NF1, 33, 128, FUSED, _tiled(64, True, 1, 128)),
    ("fp8", 256, NF1, 65, 64, FUSED, _tiled(128, True, 1, 256)),
    ("fp8", 256, NF1, 129, 64, FUSED, _tiled(256, True, 1, 256)),
    ("fp8", 768, NF1, 128, 64, FUSED, _phased(True, 1, 20, 128)),
    ("fp8", 768, NF1, 256, 64, FUSED, _phased(True, 1, 20, 256)),
    ("fp8", 768, NF1, 513, 64, FUSED, _phased(True, 1, 0, 256)),
]

# Instantiations in the library that only an A/B variant (svs_index_set_variant) reaches: kernel -> variant.
AB_ONLY = {
    "gemm_f32_q16_kernel<false, 2, 8, false>": 3,
    "gemm_f32_q16_kernel<false, 2, 8, true>": 3,
    **{_tiled(bn, f, eb, 128): 4 for bn in (128, 256) for f in (False, True) for eb in (1, 2)},
    **{_phased(True, eb, exp, 256): {30: 8, 31: 9}[exp] for eb in (1, 2) for exp in (30, 31)},
}


def _ab_shape(kernel):
    """(dtype, d, n, nq) that reaches `kernel` under its A/B variant (svs_amd.hip: launch_q16 variant 3,
    launch_tiled_eb variants 4 / 8 / 9)."""
    args = kernel[kernel.index("<") + 1:-1].split(", ")
    if kernel.startswith("gemm_f32_q16_kernel"):
        return "f32", 128, NF1 if args[3] == "true" else 3000, 16
    if kernel.startswith("gemm_tiled_kernel"):      # rows of 2 k-tiles: not the phased kernel's
        bn, fused, eb = int(args[0]), args[1] == "true", int(args[2])
        return "f16" if eb == 2 else "fp8", 256, NF1 if fused else 3000, 65 if bn == 128 else 129
    eb = int(args[1])                                # phased EXP 30 / 31: fused, 256-query tiles
    return "f16" if eb == 2 else "fp8", 768, NF1, 129


def case_id(case):
    dtype, d, n, nq, k, form, _ = case
    return f"{dtype}-d{d}-n{n}-q{nq}-k{k}-{form}"
