"""CPU: the shared passes of the run-ahead pipeline (svs_amd/csrc/pass_share.h) -- the reach rule that keeps a pass from
writing a context a selection may still read, and what hipcc made of the score kernel once it loops over a plan's
queries (the build's own resource report, as tests/test_kernel_resources.py reads it)."""
import re

import pytest

from test_kernel_resources import _demangle, _resources, build_reports  # noqa: F401  (the fixture builds when the reports are missing)
from test_shared_pass_gpu import GROUP, LAG, MAILBOX_SIZE, RING, SHARE_DEFAULT, SHARE_MAX, SHARE_NSTEP_MAX, S, claim_model, reach_of


def test_constants():
    assert 1 <= SHARE_DEFAULT <= SHARE_MAX <= 4
    assert MAILBOX_SIZE >= 1024 and MAILBOX_SIZE & (MAILBOX_SIZE - 1) == 0
    assert RING == 8


def waits_in_front_of(i):
    """The selections the pass stream has waited for when pass i starts: those the calls 0 .. i enqueued there (a wait a
    LATER call enqueues is behind pass i).  Written out from the rule, not through covered_before."""
    return {j - LAG for j in range(i + 1) if j >= LAG and j % GROUP == 0}


def test_reach_never_lets_a_pass_write_a_context_in_use():
    """Exhaustively over ring positions and backlog lengths: pass i serves i .. i + c - 1 as the model claims them; the
    context of search s was last used by search s - RING, whose selection must be over -- the caller's stream is in
    order, so that is: at most the newest selection the pass stream has waited for in front of pass i."""
    for limit in range(1, SHARE_MAX + 1):
        for start in range(0, 3 * RING):             # searches in front of the backlog, each served by its own pass
            for length in range(1, 3 * RING + 4):
                searches = [S(b) for b in range(start)] + [S(10_000)] * length
                served, hist = 0, claim_model(searches, limit)
                assert sum(c * h for c, h in enumerate(hist)) == len(searches)      # every search is served exactly once
                for i in range(len(searches)):
                    if served > i:
                        continue
                    c = 1
                    while c < limit and i + c < len(searches) and i + c <= reach_of(i) and i >= start:
                        c += 1
                    newest = max(waits_in_front_of(i), default=-1)
                    for s in range(i, i + c):
                        assert s - RING <= newest, (limit, start, length, i, s)
                    served = i + c


def test_steady_state_reaches_share_max():
    """Behind the ring's first round every pass, wherever it sits in its group, may serve SHARE_MAX searches."""
    for i in range(LAG, 6 * RING):
        assert reach_of(i) >= i + SHARE_MAX - 1, i
        assert reach_of(i) - RING < i                  # ... and never a search whose previous user has not been enqueued
    for i in range(LAG):
        assert reach_of(i) == RING - 1                 # (a drained ring: every context is free)


def _f16_oneshot(table):
    names = _demangle([n for n in table if "gemv_f16_oneshot_kernel" in n])
    out = {}
    for mangled, pretty in names.items():
        nstep = int(re.search(r"gemv_f16_oneshot_kernel<(\d+),", pretty).group(1))
        out[nstep] = table[mangled]
    return out


def _occupancy(vgpr):
    """Waves per SIMD of a gfx950 kernel without AGPRs: 512 registers per lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgpr // 8) * 8))


# registers of the kernel before it looped over a plan (the same build flags), per 512-half step of the row
PARENT_VGPRS = {1: 32, 2: 40, 3: 54, 4: 52, 5: 60, 6: 67, 7: 71, 8: 64}


def test_plan_kernel_uses_no_scratch(build_reports):  # noqa: F811
    kernels = _f16_oneshot(_resources(build_reports[0]))
    assert sorted(kernels) == list(range(1, 9))
    for nstep, r in kernels.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (nstep, r)


def test_plan_kernel_keeps_the_occupancy_where_sharing_is_on(build_reports):  # noqa: F811
    kernels = _f16_oneshot(_resources(build_reports[0]))
    for nstep, r in kernels.items():
        if nstep <= SHARE_NSTEP_MAX:
            assert r["agpr"] == 0 and _occupancy(r["vgpr"]) == _occupancy(PARENT_VGPRS[nstep]), (nstep, r)
        else:       # the plan is compiled out: the kernel is the one it was
            assert r["vgpr"] == PARENT_VGPRS[nstep], (nstep, r)


def test_claim_kernel_is_no_score_kernel(build_reports):  # noqa: F811
    """Its name must not put it among the kernels the tables of tests/test_kernel_resources.py account for."""
    table = _resources(build_reports[0])
    claim = [n for n in _demangle([n for n in table if "pass_claim_kernel" in n]).values()]
    assert len(claim) == 1 and not re.search(r"gemv_|gemm_|gather_", claim[0]), claim
