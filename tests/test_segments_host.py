"""CPU: segmented filtered retrieval above the kernel -- ``KB`` / ``AsyncKB.retrieve_many_within`` (one query and one doc
list per request) and ``retrieve_within_each`` (one query, many doc lists) on a small document tree, through a numpy
double of DeviceIndex whose ``search_segments`` is the oracle per segment.  Every element must equal
``retrieve_within`` on the same (query, list)."""
import asyncio
import logging

import numpy as np
import pytest

from fake_backend import OracleIndex
from oracle import svs_oracle as oracle

import svs_amd


class SegmentsOracleIndex(OracleIndex):
    """OracleIndex that also answers ``search_within`` and ``search_segments``: the oracle on the sub-matrix of each
    segment's live listed rows, positions mapped back to rows."""
    calls = []   # (nq, number of segments, seg_query) of every search_segments call

    def share(self):
        self._check()
        return SegmentsOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_within(self, q, n, rows):
        self._check()
        assert isinstance(n, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        local = np.unique(np.asarray(rows, dtype=np.int64)) - self.row_offset
        if len(local) and (local[0] < 0 or local[-1] >= self.n):
            raise ValueError("row out of range")
        s = local[~self._st[1][local]]
        return [(sc, int(s[p]) + self.row_offset) for sc, p in oracle.cpu_search(self._m[s], q, n)]

    def search_segments(self, queries, n, row_lists, seg_query=None):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        row_lists = list(row_lists)
        SegmentsOracleIndex.calls.append((len(q), len(row_lists), None if seg_query is None else list(seg_query)))
        if seg_query is None:
            if len(row_lists) != len(q):
                raise ValueError("one row list per query")
            seg_query = range(len(q))
        out = []
        for rows, j in zip(row_lists, seg_query):
            res = self.search_within(q[j], n, rows)
            out.append((np.array([a for a, _ in res], dtype=np.float32), np.array([b for _, b in res], dtype=np.int64)))
        return out


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _tree_kb(tmp_path, name, n_parents=4, per_parent=30, d=16, seed=3):
    rng = np.random.default_rng(seed)
    texts = [f"parent {p}" for p in range(n_parents)] + \
            [f"child {p}.{c}" for p in range(n_parents) for c in range(per_parent)] + [f"q {i}" for i in range(8)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}
    embed_calls = []

    async def ef(ts):
        embed_calls.append(list(ts))
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=SegmentsOracleIndex)
    parents, children = [], {}
    with kb.bulk_add_docs() as add_doc:
        for p in range(n_parents):
            parents.append(add_doc(f"parent {p}"))
        for p in range(n_parents):
            children[parents[p]] = [add_doc(f"child {p}.{c}", parent_id=parents[p]) for c in range(per_parent)]
    return kb, ef, embed_calls, parents, children


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def _lists(parents, children):
    """Doc lists of every kind: whole families, one level, a shuffled list with duplicates, one doc, none, two families."""
    c = [children[p] for p in parents]
    return [c[0], parents, c[1][:7][::-1] + c[1][:7], c[2][5:6], [], c[3] + c[0], c[1]]


def test_retrieve_within_each_equals_retrieve_within(tmp_path, caplog):
    kb, ef, embed_calls, parents, children = _tree_kb(tmp_path, "e.sqlite")
    lists = _lists(parents, children)
    for n in (5, 1, 100, 0):
        want = [_got(kb.retrieve_within("q 0", n, ids)) for ids in lists]
        del embed_calls[:], SegmentsOracleIndex.calls[:]
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            caplog.clear()
            got = kb.retrieve_within_each("q 0", n, lists)
        assert [_got(g) for g in got] == want, n
        assert embed_calls == [["q 0"]]                                             # one embedding call
        assert SegmentsOracleIndex.calls == [(1, len(lists), [0] * len(lists))]     # one native call, one query
        lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
        listed = sum(len(set(ids)) for ids in lists)
        assert lines == [f"retrieving {n} documents within each of {len(lists)} document lists with query string: q 0",
                         "got embedding for query!", f"computed {listed} cosine similarities",
                         f"retrieved top {n} documents for {len(lists)} lists"], lines
    # same result shape as retrieve_within()
    one = kb.retrieve_within("q 0", 1, lists[0])
    each = kb.retrieve_within_each("q 0", 1, lists)
    assert set(each[0][0]) == set(one[0]) and set(each[0][0]["doc"]) == set(one[0]["doc"])
    assert kb.retrieve_within_each("q 1", 3, []) == []
    assert kb.retrieve_within_each("q 1", 3, [[], []]) == [[], []]
    kb.close()
    assert OracleIndex.live == 0


def test_retrieve_many_within_equals_retrieve_within(tmp_path, caplog):
    kb, ef, embed_calls, parents, children = _tree_kb(tmp_path, "m.sqlite")
    lists = _lists(parents, children)
    queries = [f"q {i}" for i in range(len(lists))]
    queries[3] = queries[0]   # the same query string twice, with different lists
    for n in (4, 100):
        want = [_got(kb.retrieve_within(q, n, ids)) for q, ids in zip(queries, lists)]
        del embed_calls[:], SegmentsOracleIndex.calls[:]
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            caplog.clear()
            got = kb.retrieve_many_within(queries, n, lists)
        assert [_got(g) for g in got] == want, n
        assert embed_calls == [queries]
        assert SegmentsOracleIndex.calls == [(len(queries), len(lists), None)]
        lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
        listed = sum(len(set(ids)) for ids in lists)
        assert lines == [f"retrieving {n} documents for each of {len(queries)} query strings, each within its own documents",
                         "got embeddings for the queries!", f"computed {listed} cosine similarities",
                         f"retrieved top {n} documents for {len(queries)} queries"], lines
    assert kb.retrieve_many_within([], 3, []) == []
    with pytest.raises(ValueError):
        kb.retrieve_many_within(["q 0"], 3, [])
    kb.close()
    assert OracleIndex.live == 0


def test_queries_are_embedded_in_chunks(tmp_path, monkeypatch):
    from svs_amd import kb as kb_mod
    kb, ef, embed_calls, parents, children = _tree_kb(tmp_path, "c.sqlite")
    monkeypatch.setattr(kb_mod, "BULK_EMBEDDING_CHUNK_SIZE", 3)
    queries = [f"q {i}" for i in range(8)]
    lists = [children[parents[i % 4]][i:i + 9] for i in range(8)]
    want = [_got(kb.retrieve_within(q, 4, ids)) for q, ids in zip(queries, lists)]
    del embed_calls[:]
    assert [_got(g) for g in kb.retrieve_many_within(queries, 4, lists)] == want
    assert embed_calls == [queries[0:3], queries[3:6], queries[6:8]]
    kb.close()


def test_unknown_doc_and_docs_without_embedding(tmp_path):
    kb, ef, embed_calls, parents, children = _tree_kb(tmp_path, "u.sqlite")
    fam = children[parents[0]]
    for call in (lambda: kb.retrieve_within_each("q 0", 5, [fam[:3], [fam[0], 987654]]),
                 lambda: kb.retrieve_many_within(["q 0", "q 1"], 5, [fam[:3], [fam[0], 987654]])):
        with pytest.raises(KeyError) as e:
            call()
        assert e.value.args == (987654,)
    bare = fam[0]
    with kb.db.transaction():
        kb.db.conn.execute("UPDATE docs SET embedding = NULL WHERE id = ?", (bare,))
    lists = [fam[:6], [bare], children[parents[1]][:4]]
    want = [_got(kb.retrieve_within("q 1", 10, ids)) for ids in lists]
    assert [len(w) for w in want] == [5, 0, 4]
    assert [_got(g) for g in kb.retrieve_within_each("q 1", 10, lists)] == want
    want = [_got(kb.retrieve_within(f"q {i}", 10, ids)) for i, ids in enumerate(lists)]
    got = kb.retrieve_many_within(["q 0", "q 1", "q 2"], 10, lists)
    assert [_got(g) for g in got] == want and bare not in [r["doc"]["id"] for r in got[0]]
    kb.close()


def test_after_deletes_the_tombstoned_rows_drop_out(tmp_path):
    kb, ef, embed_calls, parents, children = _tree_kb(tmp_path, "d.sqlite")
    kb.load()
    first = kb.embeddings_matrix.index
    gone = children[parents[3]][::4]
    with kb.bulk_del_docs() as del_doc:
        for d in gone:
            del_doc(d)
    assert kb.embeddings_matrix.index is first            # tombstoned, not rebuilt
    live = [d for d in children[parents[3]] if d not in gone]
    lists = [live, children[parents[0]], live[:3]]
    want = [_got(kb.retrieve_within("q 4", 100, ids)) for ids in lists]
    assert [_got(g) for g in kb.retrieve_within_each("q 4", 100, lists)] == want
    with pytest.raises(KeyError):
        kb.retrieve_within_each("q 4", 5, [live, gone[:1]])
    kb.close()


def test_async_twins_equal_sync(tmp_path, caplog):
    kb, ef, embed_calls, parents, children = _tree_kb(tmp_path, "a.sqlite")
    path = kb.db.path
    lists = _lists(parents, children)
    queries = [f"q {i}" for i in range(len(lists))]
    want_each = [_got(g) for g in kb.retrieve_within_each("q 5", 6, lists)]
    want_many = [_got(g) for g in kb.retrieve_many_within(queries, 6, lists)]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=SegmentsOracleIndex)
        del embed_calls[:], SegmentsOracleIndex.calls[:]
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            caplog.clear()
            each = await akb.retrieve_within_each("q 5", 6, lists)
            lines_each = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb" and "cached vectors" not in r.getMessage()]
            caplog.clear()
            many = await akb.retrieve_many_within(queries, 6, lists)
            lines_many = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb" and "cached vectors" not in r.getMessage()]
        assert embed_calls == [["q 5"], queries]
        assert SegmentsOracleIndex.calls == [(1, len(lists), [0] * len(lists)), (len(queries), len(lists), None)]
        both = await asyncio.gather(akb.retrieve_within_each("q 5", 6, lists), akb.retrieve_many_within(queries, 6, lists))
        with pytest.raises(KeyError):
            await akb.retrieve_within_each("q 0", 3, [[424242]])
        with pytest.raises(KeyError):
            await akb.retrieve_many_within(["q 0"], 3, [[424242]])
        with pytest.raises(ValueError):
            await akb.retrieve_many_within(["q 0", "q 1"], 3, [[]])
        assert await akb.retrieve_within_each("q 0", 3, []) == [] and await akb.retrieve_many_within([], 3, []) == []
        await akb.close()
        return each, many, both, lines_each, lines_many

    each, many, both, lines_each, lines_many = asyncio.run(run())
    assert [_got(g) for g in each] == want_each and [_got(g) for g in many] == want_many
    assert [_got(g) for g in both[0]] == want_each and [_got(g) for g in both[1]] == want_many
    listed = sum(len(set(ids)) for ids in lists)
    assert lines_each == [f"retrieving 6 documents within each of {len(lists)} document lists with query string: q 5",
                          "got embedding for query!", f"computed {listed} cosine similarities",
                          f"retrieved top 6 documents for {len(lists)} lists"], lines_each
    assert lines_many == [f"retrieving 6 documents for each of {len(queries)} query strings, each within its own documents",
                          "got embeddings for the queries!", f"computed {listed} cosine similarities",
                          f"retrieved top 6 documents for {len(queries)} queries"], lines_many
    assert OracleIndex.live == 0
