"""The single-query score kernels and the shapes that reach them: plain data, importable without a GPU.

One row per instantiation: (dtype, d, variant, kernel).  `kernel` is what svs_internal_last_launches records behind the
"gemv" entry of a scores call, spelled as c++filt prints it in the build's resource report; `variant` is the
svs_index_set_variant value under which an index of that dtype and dimension launches it (0: the default rules).

The dispatch rules these rows follow (svs_amd/csrc/svs_amd.hip: choose_ld, single_route, launch_route, launch_rows,
launch_unrolled, for_f16_oneshot, for_fp8_oneshot, for_row_geometry, for_width; tests/test_single_route.py asks the
library for the route of every row without a device):
  * choose_ld pads a row to whole 1 KiB wave loads (64 chunks of 16 bytes) when that costs at most an eighth more
    bytes, else to whole 128-byte lines (8 chunks) on the same condition, else to whole chunks.  Below, c = ld in chunks.
  * f32, c % 64 == 0, c <= 1024 (ld = NSTEP * 256): gemv_f32_oneshot_kernel<NSTEP, R, WPB, NT, false, false>, by default
    R x WPB = 4 x 16 (NSTEP <= 2), 2 x 16 (<= 4), 1 x 16 (<= 6), 1 x 8 beyond, nontemporal; variant 3: 2 x 16, variant 4:
    1 x 16 with temporal loads, variant 5: 1 x 8; variants 1 / 2: gemv_f32_rows_kernel<NSTEP, 1, 4, false, false> /
    <NSTEP, 2, 4, true, false>, the persistent grid.
  * f16, c % 64 == 0, c <= 512 (ld = NSTEP * 512): gemv_f16_oneshot_kernel<NSTEP, R, WPB>, R = 4 (NSTEP 1), 2 (<= 3),
    1 beyond; WPB = 16 (NSTEP <= 6), 8 beyond.  No variant changes it.
  * fp8, ld in {512, 1024, 1536, 2048, 3072, 4096}: gemv_fp8_oneshot_kernel<NSTEP, LB, R, 16>.  No variant changes it.
  * every other row of c <= 1024: gemv_unrolled_kernel<T, NC, U, Dot>: T = the smallest power of two >= c (NC = 1) up
    to c = 64, then T = 64 with NC = 2, 3, 4, 6, 8, 12, 16 chunks per lane (the smallest that covers c); U = 8, 4, 2, 2, 1 ...
    Variant 4 sends these rows to the loop kernels instead.
  * the loop kernels, gemv_f32_generic_kernel<T> / gemv_f16_generic_kernel<T> / gemv_fp8_kernel<T>: T as above, 64 for
    every c > 64.  By default they take only rows of c > 1024 (T = 64).

An f32 row of more than 512 chunks is always padded to whole wave loads (the next multiple of 64 chunks is less than an
eighth away), and those are the one-shot kernel's up to 1024 chunks: no f32 index launches gemv_unrolled_kernel<64, 12,
1, svs::DotF32> or <64, 16, 1, svs::DotF32>, under any variant.  They are in the library (for_row_geometry instantiates
every geometry for every Dot) and are listed in NO_SHAPE; test_kernel_resources.py proves the claim from choose_ld below.
"""

PER16 = {"f32": 4, "f16": 8, "fp8": 16}      # elements per 16-byte chunk
DOT = {"f32": "svs::DotF32", "f16": "svs::DotF16", "fp8": "svs::DotFp8"}
LOOP = {"f32": "gemv_f32_generic_kernel<{}>", "f16": "gemv_f16_generic_kernel<{}>", "fp8": "gemv_fp8_kernel<{}>"}


def choose_ld(d, dtype):
    """Row stride in elements, as svs_amd.hip's choose_ld."""
    align = PER16[dtype]
    tight = (d + align - 1) // align * align
    wave, line = 64 * align, 8 * align
    waved, lined = (d + wave - 1) // wave * wave, (d + line - 1) // line * line
    if waved * 8 <= tight * 9:
        return waved
    if lined * 8 <= tight * 9:
        return lined
    return tight


def _b(flag):
    return "true" if flag else "false"


def _f32_oneshot(nstep, r, wpb, nt):
    return f"gemv_f32_oneshot_kernel<{nstep}, {r}, {wpb}, {_b(nt)}, false, false>"


def _f32_default(nstep):
    r, wpb = (4, 16) if nstep <= 2 else (2, 16) if nstep <= 4 else (1, 16) if nstep <= 6 else (1, 8)
    return _f32_oneshot(nstep, r, wpb, True)


def _f16_oneshot(nstep):
    return f"gemv_f16_oneshot_kernel<{nstep}, {4 if nstep <= 1 else 2 if nstep <= 3 else 1}, {16 if nstep <= 6 else 8}>"


def unrolled_u(nc):
    return 8 if nc <= 1 else 4 if nc <= 2 else 2 if nc <= 4 else 1


def _unrolled(t, nc, dtype):
    return f"gemv_unrolled_kernel<{t}, {nc}, {unrolled_u(nc)}, {DOT[dtype]}>"


# gemv_unrolled_kernel geometries: (T, NC, row length in chunks).  Every length but 1 and 2 leaves lanes past the row;
# none is one that choose_ld would pad, and none is an exact geometry of a one-shot kernel (576 and 832 chunks are whole
# wave loads, but past the f16 one-shot kernel's 512 and not among the fp8 one-shot kernel's lengths).
UNROLLED = [(1, 1, 1), (2, 1, 2), (4, 1, 3), (8, 1, 6), (16, 1, 12), (32, 1, 24), (64, 1, 40),
            (64, 2, 104), (64, 3, 160), (64, 4, 224), (64, 6, 280), (64, 8, 392), (64, 12, 576), (64, 16, 832)]
# loop kernels under variant 4: (T, row length in chunks); T = 64 takes two trips, the second with 8 lanes
LOOPS = [(1, 1), (2, 2), (4, 3), (8, 6), (16, 12), (32, 24), (64, 72)]
FP8_HOT = {512: (1, 8, 4), 1024: (1, 16, 4), 1536: (3, 8, 2), 2048: (2, 16, 2), 3072: (3, 16, 1), 4096: (4, 16, 1)}

CASES = []
# ---- f32 rows of whole wave loads: 52 one-shot geometries, 32 persistent ---------------------------------------------
for _n in range(1, 17):
    CASES.append(("f32", 256 * _n, 0, _f32_default(_n)))
    for _v, _k in ((3, _f32_oneshot(_n, 2, 16, True)), (4, _f32_oneshot(_n, 1, 16, False)), (5, _f32_oneshot(_n, 1, 8, True))):
        if _k != _f32_default(_n):      # (variant 3 at NSTEP 3, 4 and variant 5 from NSTEP 7 are the default geometry)
            CASES.append(("f32", 256 * _n, _v, _k))
    CASES.append(("f32", 256 * _n, 1, f"gemv_f32_rows_kernel<{_n}, 1, 4, false, false>"))
    CASES.append(("f32", 256 * _n, 2, f"gemv_f32_rows_kernel<{_n}, 2, 4, true, false>"))
# ---- f16 and fp8 rows of whole wave loads ----------------------------------------------------------------------------
CASES += [("f16", 512 * _n, 0, _f16_oneshot(_n)) for _n in range(1, 9)]
CASES += [("fp8", _ld, 0, "gemv_fp8_oneshot_kernel<{}, {}, {}, 16>".format(*_g)) for _ld, _g in sorted(FP8_HOT.items())]
# ---- every other row: gemv_unrolled_kernel by default, the loop kernels under variant 4 (d = one short of the padded
#      row, so the row's last chunk ends in a zero column) ---------------------------------------------------------------
for _dt in ("f32", "f16", "fp8"):
    CASES += [(_dt, _c * PER16[_dt] - 1, 0, _unrolled(_t, _nc, _dt)) for _t, _nc, _c in UNROLLED
              if not (_dt == "f32" and _nc >= 12)]
    CASES += [(_dt, _c * PER16[_dt] - 1, 4, LOOP[_dt].format(_t)) for _t, _c in LOOPS]

# Instantiations that no index can launch (the docstring's last paragraph): kernel -> why
NO_SHAPE = {_unrolled(64, _nc, "f32"): "choose_ld pads every f32 row of more than 512 chunks to whole wave loads"
            for _nc in (12, 16)}

# Rows of more than 16 KiB: the loop kernels' default use (T = 64, 17 trips).  Further cases of kernels CASES already
# holds: the GPU tests run their edge and identical-row checks on these too.
LONG_ROWS = [(_dt, 1088 * PER16[_dt] - 1, 0, LOOP[_dt].format(64)) for _dt in ("f32", "f16", "fp8")]


def _args(kernel):
    return kernel[kernel.index("<") + 1:-1].split(", ")


def rows_per_wave(kernel):
    """G: rows a wave takes per pass."""
    a = _args(kernel)
    if kernel.startswith(("gemv_f32_oneshot_kernel", "gemv_f16_oneshot_kernel", "gemv_f32_rows_kernel")):
        return int(a[1])
    if kernel.startswith("gemv_fp8_oneshot_kernel"):
        return int(a[2])
    if kernel.startswith("gemv_unrolled_kernel"):
        return 64 // int(a[0]) * int(a[2])
    assert kernel.startswith(("gemv_f32_generic_kernel", "gemv_f16_generic_kernel", "gemv_fp8_kernel")), kernel
    return 64 // int(a[0])


def rows_per_block(kernel):
    """B: rows per workgroup."""
    a, g = _args(kernel), rows_per_wave(kernel)
    if kernel.startswith(("gemv_f32_oneshot_kernel", "gemv_f16_oneshot_kernel")):
        return g * int(a[2])
    if kernel.startswith("gemv_fp8_oneshot_kernel"):
        return g * int(a[3])
    if kernel.startswith("gemv_unrolled_kernel"):
        return 16 * g
    return 4 * g        # the loop kernels and the persistent kernel: four waves


def case_id(case):
    dtype, d, variant, kernel = case
    return f"{dtype}-d{d}-v{variant}-{kernel}".replace(" ", "").replace("svs::", "")
