"""CPU: the route of a batch of two or more queries (svs_amd/csrc/svs_amd.hip: batch_route, launch_batch) through
svs_internal_batch_route -- pure host code that walks the dispatch that launches, in its name-only mode.  For every row
of tests/batch_kernel_table.py the route names that row's kernel (tests/test_batch_kernels_gpu.py asserts that the kernel
ran), and over a sweep of shapes and variants what the call decides once -- family, queries per tile, rows of the staged
query image -- fits the kernel every pass is given."""
import ctypes as C
import re

import pytest

from batch_kernel_table import AB_ONLY, CASES, FUSED, _ab_shape, case_id
from svs_amd import _native

DTYPE = {"f32": _native.DTYPE_F32, "f16": _native.DTYPE_F16, "fp8": _native.DTYPE_FP8}
LOOP, Q16, TILED_F32, TILED_EB = range(4)
FUSED_FLAG, PAIRS_FLAG = 1, 2


def route(dtype, d, nq, n_rows, variant=0, flags=0):
    """(kernel, family, queries per tile, staged rows), or None where the hook refuses."""
    name, info = C.create_string_buffer(96), (C.c_int32 * 3)(-1, -1, -1)
    rc = _native.load().svs_internal_batch_route(DTYPE[dtype], d, variant, nq, n_rows, flags, name, len(name), info)
    return (name.value.decode(), *info) if rc == _native.SVS_OK else None


def _unfused(kernel):
    """The non-fused form of a fused kernel's family (the phased kernels' EXP belongs to the fused epilogue)."""
    m = re.fullmatch(r"gemm_phased_kernel<true, (\d+), \d+, (\d+)>", kernel)
    return "gemm_phased_kernel<false, %s, 0, %s>" % m.groups() if m else kernel.replace("true", "false")


def _is_fused(kernel):
    """FUSE is a bool template argument of every batched kernel, and their only one that can be true."""
    return "true" in kernel


def _prefix_rows(n):
    return (max(16384, n // 64) + 255) // 256 * 256


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_route_names_the_tables_kernel(case):
    dtype, d, n, nq, _, form, kernel = case
    got = route(dtype, d, nq, n, flags=FUSED_FLAG if form == FUSED else 0)
    assert got is not None, _native.last_error()
    assert got[0] == kernel
    if form == FUSED:   # the threshold pass: fewer rows, materialised, the same family at the same query tile
        pre = route(dtype, d, nq, _prefix_rows(n))
        assert pre is not None, _native.last_error()
        assert pre[0] == _unfused(kernel)
        assert pre[1:] == got[1:]


@pytest.mark.parametrize("kernel", sorted(AB_ONLY))
def test_ab_only_kernels_named_under_their_variant(kernel):
    dtype, d, n, nq = _ab_shape(kernel)
    fused = _is_fused(kernel)
    got = route(dtype, d, nq, n, AB_ONLY[kernel], FUSED_FLAG if fused else 0)
    assert got is not None, _native.last_error()
    assert got[0] == kernel
    assert route(dtype, d, nq, n, 0, FUSED_FLAG if fused else 0)[0] != kernel   # ... and only under it


def _tile_in_name(kernel):
    m = re.fullmatch(r"gemm_tiled_kernel<(\d+), .*>", kernel) or re.fullmatch(r"gemm_phased_kernel<.*, (\d+)>", kernel)
    return int(m.group(1)) if m else None


@pytest.mark.parametrize("d", [100, 128, 256, 384, 448, 1100, 1536, 2304, 2305, 4608, 4609])
@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_what_the_call_decides_fits_every_pass(dtype, d):
    for variant in range(13):
        assert route(dtype, d, 1, 1000, variant) is None          # one query is single_route's
        for nq in range(2, 601):
            for n_rows, flags in ((1000, 0), (200_000, FUSED_FLAG)):
                got = route(dtype, d, nq, n_rows, variant, flags)
                assert got is not None, (variant, nq, flags, _native.last_error())
                kernel, family, tile, rows = got
                where = (dtype, d, variant, nq, flags, got)
                if variant == 7:
                    assert kernel == "gemv", where
                assert (family == LOOP) == (kernel == "gemv"), where
                if family == LOOP:
                    assert (tile, rows) == (1, nq), where
                    continue
                # the staged image is the batch rounded up to the queries per tile, and the kernel reads it at that tile
                assert rows % tile == 0 and nq <= rows < nq + tile, where
                assert (tile == 16) == ("q16" in kernel) == (family == Q16), where
                if family != Q16:
                    assert _tile_in_name(kernel) == tile, where
                    assert (family == TILED_F32) == (dtype == "f32"), where
                assert _is_fused(kernel) == bool(flags & FUSED_FLAG), where
            # pair mode: refused exactly where the family is the 16-query one
            pairs = route(dtype, d, nq, 1000, variant, FUSED_FLAG | PAIRS_FLAG)
            assert (pairs is None) == (family == Q16), (dtype, d, variant, nq, pairs)


def test_hook_refuses_what_no_index_has():
    assert route("f16", 512, 1, 1000) is None
    assert route("f16", 512, 0, 1000) is None
    assert route("f16", 0, 16, 1000) is None
    assert route("f16", 512, 16, 1000, variant=13) is None
    assert route("f16", 512, 16, 1000, variant=-1) is None
    assert route("f16", 512, 16, 0) is None
    assert route("f16", 512, 16, 1000, flags=4) is None
    assert _native.load().svs_internal_batch_route(7, 512, 0, 16, 1000, 0, C.create_string_buffer(96), 96, (C.c_int32 * 3)()) != _native.SVS_OK
    assert route("f16", 512, 16, 1000) is not None
