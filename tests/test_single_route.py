"""CPU: the route of a single query (svs_amd/csrc/svs_amd.hip: single_route, launch_route) through
svs_internal_single_route -- pure host code that walks the dispatch that launches, in its name-only mode.  For every
row of tests/single_kernel_table.py the route names that row's kernel; tests/test_single_kernels_gpu.py asserts that
the kernel ran."""
import ctypes as C
import re

import pytest

from single_kernel_table import CASES, LONG_ROWS, case_id
from svs_amd import _native

DTYPE = {"f32": _native.DTYPE_F32, "f16": _native.DTYPE_F16, "fp8": _native.DTYPE_FP8}
SHARES, QUERY_PADDED = 1, 2
SHARE_NSTEP_MAX = 7      # gemv_f16.h: F16_SHARE_NSTEP_MAX


def route(dtype, d, variant=0, screen=0):
    """(kernel, flags), or None where the hook refuses the shape."""
    name, flags = C.create_string_buffer(96), C.c_int32(-1)
    rc = _native.load().svs_internal_single_route(DTYPE[dtype], d, variant, screen, name, len(name), C.byref(flags))
    return (name.value.decode(), flags.value) if rc == _native.SVS_OK else None


def _f16_oneshot_nstep(kernel):
    m = re.match(r"gemv_f16_oneshot_kernel<(\d+),", kernel)
    return int(m.group(1)) if m else None


@pytest.mark.parametrize("case", CASES + LONG_ROWS, ids=case_id)
def test_route_names_the_tables_kernel(case):
    dtype, d, variant, kernel = case
    got = route(dtype, d, variant)
    assert got is not None, _native.last_error()
    assert got[0] == kernel
    nstep = _f16_oneshot_nstep(kernel)
    assert bool(got[1] & SHARES) == (nstep is not None and nstep <= SHARE_NSTEP_MAX), (case, got)


def test_the_table_holds_every_f16_oneshot_geometry():
    """... so that the test above has seen `shares` on both sides of the bound."""
    assert sorted(_f16_oneshot_nstep(k) for _, _, _, k in CASES if _f16_oneshot_nstep(k)) == list(range(1, 9))


@pytest.mark.parametrize("d", range(512, 4097, 512))
def test_screened_f32_takes_the_f16_oneshot_over_the_shadow(d):
    kernel, flags = route("f32", d, 0, screen=1)
    assert _f16_oneshot_nstep(kernel) == d // 512
    assert bool(flags & SHARES) == (d <= 3584)
    assert flags & QUERY_PADDED
    # unscreened, the same index takes the f32 one-shot kernel, which shares nothing and reads the query the same way
    plain, plain_flags = route("f32", d, 0)
    assert plain.startswith("gemv_f32_oneshot_kernel<%d," % (d // 256)) and plain_flags == QUERY_PADDED


def test_query_staging_flag():
    """Copied when the rows are padded: every kernel that reads ld f32 query floats, not the loop kernel (d floats) and
    not the routes that convert the query (f16 off the one-shot geometry, fp8)."""
    assert route("f32", 1000)[1] == QUERY_PADDED                    # 1024-float rows, one-shot
    assert route("f32", 23)[1] == QUERY_PADDED                      # gemv_unrolled_kernel
    assert route("f32", 23, 4)[1] == 0                              # variant 4: the loop kernel
    assert route("f16", 1000)[1] == QUERY_PADDED | SHARES
    assert route("f16", 47)[1] == 0
    assert route("fp8", 1024)[1] == 0


def test_hook_refuses_what_no_index_has():
    assert route("f32", 100, screen=1) is None          # no shadow: not a geometry of the f16 one-shot kernel
    assert route("f16", 512, screen=1) is None          # only an f32 index has a shadow
    assert route("f32", 512, variant=99) is None
    assert route("f32", 0) is None
