"""The score kernels of a filtered search and the shapes that reach them: plain data, importable without a GPU.

gather_scores_kernel<DT, T, NC, U, G> (svs_amd/csrc/gather.h) is the score stage of svs_index_search_rows, i.e. of
DeviceIndex.search_within / search_batch_within and KB.retrieve_within.  One row per (dtype, d):
(dtype, d, shape, kernel of a lone query, kernel of a batch).  The names are what svs_internal_last_launches records
(kGatherName) and what c++filt prints in the build's resource report.

The dispatch rules these rows follow (svs_amd/csrc/svs_amd.hip: choose_ld, launch_gather_dt, for_row_geometry, gather_u;
gather.h: gather_wpb, GATHER_G):
  * DT is 0, 1, 2 for f32, f16, fp8.  No variant and no row count changes the kernel: only the row length does.
  * choose_ld pads the row (single_kernel_table.choose_ld); below, c = the padded row in 16-byte chunks, at most 1024.
  * T lanes share a row: the smallest power of two >= c up to c = 64 (NC = 1), then T = 64 with NC = 2, 3, 4, 6, 8, 12, 16
    chunks per lane, the smallest that covers c.
  * a lane group takes U rows per pass: 8, 6, 4, 3, 2, 2, 1, 1 for NC = 1, 2, 3, 4, 6, 8, 12, 16, so a wave takes
    (64 / T) U rows; a workgroup has 16 waves, 8 for NC >= 12.
  * G = 1 for a lone query; G = 4 for every batch (nq >= 2): groups of four queries staged in LDS, the last group of a
    batch may hold fewer.

Two shapes per (dtype, geometry):
  ragged  d = c PER16 - 1 at the chunk counts of single_kernel_table.UNROLLED: every length but 1 and 2 leaves lanes past
          the row, and the row's last chunk ends in a zero column;
  exact   d = T NC PER16: no lane past the row.  These are the workload's own row lengths (f32 d = 1536 is c = 384), and
          c = 1024 stages 4 x 16 KiB = 65,536 bytes of LDS for a batch.
"""
from single_kernel_table import PER16, UNROLLED, choose_ld  # noqa: F401  (choose_ld: for the tests that import this table)

DT = {"f32": 0, "f16": 1, "fp8": 2}
GATHER_G = 4


def gather_u(nc):
    return 8 if nc <= 1 else 6 if nc <= 2 else 4 if nc <= 3 else 3 if nc <= 4 else 2 if nc <= 8 else 1


def gather_wpb(nc):
    return 8 if nc >= 12 else 16


def _gather(dtype, t, nc, g):
    return f"gather_scores_kernel<{DT[dtype]}, {t}, {nc}, {gather_u(nc)}, {g}>"


CASES = []
for _dt in ("f32", "f16", "fp8"):
    for _t, _nc, _c in UNROLLED:
        for _shape, _d in (("ragged", _c * PER16[_dt] - 1), ("exact", _t * _nc * PER16[_dt])):
            CASES.append((_dt, _d, _shape, _gather(_dt, _t, _nc, 1), _gather(_dt, _t, _nc, GATHER_G)))


def _args(kernel):
    return [int(a) for a in kernel[kernel.index("<") + 1:-1].split(", ")]


def geometry(kernel):
    """(T, NC) of a kernel name."""
    a = _args(kernel)
    return a[1], a[2]


def rows_per_wave(kernel):
    """W: rows a wave takes."""
    _, t, _, u, _ = _args(kernel)
    return 64 // t * u


def rows_per_block(kernel):
    """B: rows per workgroup."""
    return rows_per_wave(kernel) * gather_wpb(_args(kernel)[2])


def case_id(case):
    dtype, d, shape, kernel, _ = case
    t, nc = geometry(kernel)
    return f"{dtype}-d{d}-{shape}-t{t}-nc{nc}"
