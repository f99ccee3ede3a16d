"""CPU: thin grids of the run-ahead pipeline's shared passes (svs_amd/csrc/pass_share.h, enqueue_ahead) -- the host's
prediction of which searches an earlier pass will serve, restated here and held against the claim model of
tests/test_shared_pass_gpu.py, and what hipcc made of the score kernel now that the plan's queries live in LDS."""
import random
import re

from test_kernel_resources import ISA, _demangle, _resources, build_reports  # noqa: F401  (the fixture builds when the reports are missing)
from test_shared_pass_gpu import RING, SHARE_MAX, SHARE_NSTEP_MAX, S, claim_model, reach_of


def host_prediction(searches, limit):
    """enqueue_ahead's copy of the claim rule, given that no claim kernel of the search's own batch has run when the
    search is enqueued (and every one of an earlier batch has): -> per search, True where its pass gets the thin grid.
    The host keeps ONE owner: the last shareable search it did not predict as claimed."""
    thin, owner = [], None
    for i, s in enumerate(searches):
        if not s["share"]:
            owner = None                      # (publishes nothing: ends every run)
            thin.append(False)
            continue
        joins = (owner is not None and i == owner["next"] and owner["next"] - owner["num"] < limit and s["claimable"] and
                 i <= owner["reach"] and s["key"] == owner["key"])
        if joins and owner["batch"] == s["batch"]:      # the owner's claim kernel has not run: it will find this search
            owner["next"] += 1
            thin.append(True)
        else:
            owner = {"num": i, "next": i + 1, "reach": reach_of(i), "key": s["key"], "batch": s["batch"]}
            thin.append(False)
    return thin


def served_by_an_earlier_pass(searches, limit):
    """Per search, from claim_model alone: its pass is an empty one exactly when the model's count of empty passes
    grows with it (what serves search i never depends on the searches behind i)."""
    out, before = [], 0
    for i in range(len(searches)):
        empty = claim_model(searches[:i + 1], limit)[0]
        out.append(empty > before)
        before = empty
    return out


def backlogs():
    """The table of tests/test_shared_pass.py (searches in front, each of a batch of its own, then one backlog), and
    seeded mixtures of everything that ends a run: a search that does not share, one that is not claimable, another
    key, another batch."""
    for start in range(0, 3 * RING):
        for length in range(1, 3 * RING + 4):
            yield [S(b) for b in range(start)] + [S(10_000)] * length
    rng = random.Random(9)
    for _ in range(400):
        n, batch, out = rng.randrange(1, 5 * RING), 0, []
        for _ in range(n):
            batch += rng.random() < 0.15
            out.append(S(batch, share=rng.random() < 0.9, claimable=rng.random() < 0.8, key=int(rng.random() < 0.1)))
        yield out


def test_prediction_is_the_claim_model():
    cases = 0
    for searches in backlogs():
        for limit in range(1, SHARE_MAX + 1):
            assert host_prediction(searches, limit) == served_by_an_earlier_pass(searches, limit), (limit, searches)
            cases += 1
    assert cases > 4000


def test_benchmark_pattern_three_of_four():
    """Every fourth search timed (never claimable), all of one batch: three thin passes for every four searches."""
    searches = [S(0)] + [S(1, claimable=i % 4 != 0) for i in range(200)]
    thin = host_prediction(searches, SHARE_MAX)
    assert sum(thin) == 150 and not any(thin[1 + i] for i in range(0, 200, 4))


def _f16_oneshot(table, pattern):
    out = {}
    for mangled, pretty in _demangle([n for n in table if "gemv_f16_oneshot_kernel" in n]).items():
        out[int(re.search(r"gemv_f16_oneshot_kernel<(\d+),", pretty).group(1))] = pattern(mangled)
    return out


def test_oneshot_kernels_have_no_static_lds_and_no_scratch(build_reports):  # noqa: F811
    """The plan's queries live in DYNAMIC LDS -- the launch asks for share_limit * ld * 2 bytes, nothing under
    plan == nullptr -- so the kernels' own (static) LDS stays 0: what a launch asks for is all a workgroup takes."""
    with open(build_reports[0]) as f:
        txt = f.read()
    table = _resources(build_reports[0])

    def lds(mangled):
        block = txt[txt.index("Function Name: " + mangled):]
        return int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1))
    static = _f16_oneshot(table, lds)
    scratch = _f16_oneshot(table, lambda m: table[m]["scratch"])
    assert sorted(static) == list(range(1, 9))
    for nstep in range(1, 9):
        assert static[nstep] == 0 and scratch[nstep] == 0, (nstep, static[nstep], scratch[nstep])
    # the most a launch asks for: 28 KB; two workgroups of 16 waves (four of 8) fit a CU's 160 KB many times over
    assert SHARE_MAX * SHARE_NSTEP_MAX * 512 * 2 == 28 * 1024


def test_queries_go_through_lds_where_sharing_is_on(build_reports):  # noqa: F811
    """The ISA: one 16-byte LDS write per rounded slice and 16-byte reads in the loop over the plan's queries for
    1 .. F16_SHARE_NSTEP_MAX steps, one barrier; the kernel without a plan (8 steps) touches no LDS."""
    with open(build_reports[1]) as f:
        isa = f.read()
    table = _resources(build_reports[0])
    bodies = _f16_oneshot(table, lambda m: isa[isa.index("\n" + m + ":"):isa.index(".Lfunc_end", isa.index("\n" + m + ":"))])
    for nstep, body in bodies.items():
        reads, writes, barriers = body.count("ds_read_b128"), body.count("ds_write_b128"), body.count("s_barrier")
        if nstep <= SHARE_NSTEP_MAX:
            assert reads == nstep and writes >= 1 and barriers == 1, (nstep, reads, writes, barriers)
        else:
            assert reads == writes == barriers == 0 and "ds_" not in body, (nstep, reads, writes, barriers)
