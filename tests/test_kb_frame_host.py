"""CPU: the protocol every ``AsyncKB`` retrieval follows -- SQL and the reference to the index under the lock, the
embedding and the native call outside it, the documents under the lock again -- checked on all nine of them: the lock
is free while the native call runs, and a call that fails in its SQL, in the embedding function or in the native
call leaves neither a reference nor the lock behind.  The index is a numpy double (tests/fake_backend.py)."""
import asyncio
import threading

import numpy as np
import pytest

from fake_backend import OracleIndex
from test_compact_host import CompactingOracleIndex
from test_neighbors_host import NeighborsOracleIndex

import svs_amd

N_DOCS, DIM = 40, 8
UNKNOWN = 987654


class EmbedDown(Exception):
    pass


class NativeDown(Exception):
    pass


class FrameOracleIndex(NeighborsOracleIndex):
    """All seven native searches, each behind ``_park()``: the gate of ``CompactingOracleIndex``, and ``boom`` makes
    the NEXT native call of any owner raise instead."""

    boom = False

    def share(self):
        self._check()
        return FrameOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    @staticmethod
    def _park():
        if FrameOracleIndex.boom:
            FrameOracleIndex.boom = False
            raise NativeDown("device error")
        CompactingOracleIndex._park()


def _table():
    rng = np.random.default_rng(59)
    vecs = rng.standard_normal((N_DOCS + 4, DIM))
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    names = [f"doc {i}" for i in range(N_DOCS)] + [f"q {i}" for i in range(4)]
    return {t: [float(x) for x in v] for t, v in zip(names, vecs)}


TABLE = _table()
EMBED = {"down": False}


async def _ef(texts):
    if EMBED["down"]:
        raise EmbedDown("no embeddings today")
    return [TABLE[t] for t in texts]


A, B = list(range(3, 30, 2)), [40, 1, 17, 1, 22]   # doc ids (doc id == i + 1)

# name -> (the call, the call with a doc id nobody has [None: no SQL phase], whether it embeds)
CALLS = {
    "retrieve": (lambda k: k.retrieve("q 0", 5), None, True),
    "retrieve_within": (lambda k: k.retrieve_within("q 0", 5, A), lambda k: k.retrieve_within("q 0", 5, A + [UNKNOWN]), True),
    "retrieve_above": (lambda k: k.retrieve_above("q 1", 0.2, 30), None, True),
    "retrieve_many": (lambda k: k.retrieve_many(["q 0", "q 1", "q 2"], 4), None, True),
    "retrieve_many_within": (lambda k: k.retrieve_many_within(["q 2", "q 3"], 4, [A, B]),
                             lambda k: k.retrieve_many_within(["q 2", "q 3"], 4, [A, [UNKNOWN]]), True),
    "retrieve_within_each": (lambda k: k.retrieve_within_each("q 3", 3, [A, B, []]),
                             lambda k: k.retrieve_within_each("q 3", 3, [A, [2, UNKNOWN]]), True),
    "retrieve_similar": (lambda k: k.retrieve_similar(7, 6), lambda k: k.retrieve_similar(UNKNOWN, 6), False),
    "document_neighbors": (lambda k: k.document_neighbors(3, B), lambda k: k.document_neighbors(3, [4, UNKNOWN]), False),
    "document_top_pairwise_scores": (lambda k: k.document_top_pairwise_scores(9), None, False),
}

FAILURES = [(name, point) for name, (_, bad_sql, embeds) in CALLS.items()
            for point in ("sql", "embedding", "native")
            if (point != "sql" or bad_sql is not None) and (point != "embedding" or embeds)]


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """(path of a KB file of N_DOCS docs, {name: what the sync KB answers}) -- computed once, never changed."""
    path = str(tmp_path_factory.mktemp("frame") / "kb.sqlite")
    kb = svs_amd.KB(path, _ef, index_factory=FrameOracleIndex)
    with kb.bulk_add_docs() as add_doc:
        for i in range(N_DOCS):
            add_doc(f"doc {i}", meta={"i": i})
    want = {name: call(kb) for name, (call, _, _) in CALLS.items()}
    kb.close()
    assert OracleIndex.live == 0
    return path, want


@pytest.mark.parametrize("name", list(CALLS))
def test_lock_is_free_while_the_search_runs(stored, name):
    path, want = stored
    call = CALLS[name][0]

    async def run():
        loop = asyncio.get_running_loop()
        akb = svs_amd.AsyncKB(path, _ef, index_factory=FrameOracleIndex)
        await akb.load()
        entered, go = threading.Event(), threading.Event()
        CompactingOracleIndex.gate = (entered, go)
        task = asyncio.ensure_future(call(akb))
        try:
            assert await loop.run_in_executor(None, entered.wait, 30)     # (the loop keeps running meanwhile)
            assert not task.done()
            assert await asyncio.wait_for(akb.count(), 10) == N_DOCS      # the lock is free: the native call is parked
        finally:
            go.set()
        got = await task
        await akb.close()
        return got

    try:
        assert asyncio.run(run()) == want[name]
    finally:
        CompactingOracleIndex.gate = None
    assert OracleIndex.live == 0


@pytest.mark.parametrize("name,point", FAILURES)
def test_failed_call_leaves_no_reference_and_no_lock(stored, name, point):
    path, want = stored
    call, bad_sql, _ = CALLS[name]

    async def run():
        akb = svs_amd.AsyncKB(path, _ef, index_factory=FrameOracleIndex)
        await akb.load()
        live = OracleIndex.live
        assert live == 1
        if point == "sql":
            with pytest.raises(KeyError) as e:
                await bad_sql(akb)
            assert e.value.args == (UNKNOWN,)
        elif point == "embedding":
            EMBED["down"] = True
            with pytest.raises(EmbedDown):
                await call(akb)
            EMBED["down"] = False
        else:
            FrameOracleIndex.boom = True
            with pytest.raises(NativeDown):
                await call(akb)
            assert not FrameOracleIndex.boom                              # (it was the native call that raised)
        assert OracleIndex.live == live                                   # no reference survives
        assert await asyncio.wait_for(akb.count(), 10) == N_DOCS          # no lock survives
        got = await call(akb)
        assert OracleIndex.live == live
        await akb.close()
        return got

    try:
        assert asyncio.run(run()) == want[name]
    finally:
        EMBED["down"] = False
        FrameOracleIndex.boom = False
    assert OracleIndex.live == 0
