"""The pinned lifecycle schedules of the sparse-vector index (spv_lifecycle.py) replayed on GpuSparseIndex, and a short life of a
VectorStore with enable_sparse(): after every step ids, order, distance bits, counts and statistics equal the model's."""
import numpy as np
import pytest

import spv_data as S
import spv_lifecycle as L

pytestmark = pytest.mark.gpu
U32, F32, U64 = np.uint32, np.float32, np.uint64


class GpuAdapter:
    def __init__(self, vdb):
        self.vdb, self.ix, self.table = vdb, vdb.GpuSparseIndex(), vdb.MetaTable(0)
        self.table.set_present(0, L.ID_LIMIT, True)

    def bulk(self, ids, vecs):
        self.ix.add_bulk(ids, vecs)

    def remove(self, i):
        self.ix.remove(int(i))

    def flush(self):
        self.ix.flush()

    def set_cap(self, nbytes):
        self.ix.debug_set_workspace_cap(nbytes)

    def __len__(self):
        return len(self.ix)

    def stats(self):
        return dict(len=len(self.ix), **self.ix.stats())

    def read(self, queries, ks, on, compiled=False):
        try:
            if on is not None and compiled:
                self.table.set_codes(0, 0, on.astype(np.int32))
                with self.table.compile([(self.vdb.MetaTable.EQ, 0, 1)], L.ID_LIMIT) as cm:
                    ids, d, counts = self.ix.search_batch_arrays(queries, ks, compiled_mask=cm)
            elif on is not None:
                ids, d, counts = self.ix.search_batch_arrays(queries, ks, id_mask=L.mask_words(on), mask_bits=L.ID_LIMIT)
            else:
                ids, d, counts = self.ix.search_batch_arrays(queries, ks)
        except self.vdb.NanDistance:
            raise L.Predicted("nan")
        return [(ids[b, :counts[b]], d[b, :counts[b]]) for b in range(len(queries))]


@pytest.mark.parametrize("j", range(len(L.PROFILES)))
def test_pinned_schedule(vdb, j):
    L.run(L.pinned()[j], GpuAdapter(vdb))


# ------------------------------------------------------------------ store level
def test_vector_store_life_with_sparse_vectors(vdb):
    """inserts with and without sparse=, upserts that drop and that change the sparse vector, delete, compact() of the dense index,
    the device filter on and off: after each step search_sparse, search_sparse_batch and search_hybrid under no filter, a string
    filter and a numeric one equal search_csr over the internal ids (and rrf_fuse over the dense list the store itself returns)."""
    F = vdb.MetadataFilter
    rng = np.random.default_rng(9)
    store = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    store.enable_sparse()
    log, name_of, meta_of, present = [], {}, {}, {}      # log[internal] = the sparse vector or None

    def put(name, sparse=True):
        internal = len(log)
        old = [i for i, n in name_of.items() if n == name and present[i]]
        for i in old:
            present[i] = False
        vec = L.vectors_of(9, internal, 1, 30, None)[0] if sparse else None
        meta = {"c": "ab"[internal % 2], "price": float(internal % 7)}
        store.insert_with_metadata(name, vdb.Vector(rng.random(8, dtype=F32)), vdb.Metadata(meta), sparse=vec)
        log.append(vec)
        name_of[internal], meta_of[internal], present[internal] = name, meta, True

    def delete(name):
        store.delete(name)
        for i, n in name_of.items():
            if n == name:
                present[i] = False

    filters = [(None, lambda m: True), (F.Eq("c", "a"), lambda m: m["c"] == "a"), (F.Ge("price", 3.0), lambda m: m["price"] >= 3.0)]
    queries = L.queries_of(9, 1, 3, 30, False)
    dq = vdb.Vector(rng.random(8, dtype=F32))

    def check():
        none = (np.zeros(0, U32), np.zeros(0, F32))
        offsets, indices, values = S.csr_of([v if v is not None else none for v in log])
        ids = np.arange(len(log), dtype=U64)
        live = np.array([present[i] and log[i] is not None for i in range(len(log))])
        for flt, pred in filters:
            elig = np.array([pred(meta_of[i]) for i in range(len(log))])
            want = [S.search_csr(ids, offsets, indices, values, live, q, 10, elig) for q in queries]
            got = store.search_sparse_batch(queries, 10, flt)
            one = store.search_sparse(queries[0], 10, flt)
            assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[0]]
            for (wi, wd), g in zip(want, [one] + got[1:]):
                assert [r.id for r in g] == [name_of[int(i)] for i in wi]
                assert np.array_equal(np.array([r.distance for r in g], F32).view(U32), wd.view(U32))
            deep, _ = S.search_csr(ids, offsets, indices, values, live, queries[0], 100, elig)
            dense = store._masked(flt, lambda m, b, cm: store._index.search_batch([(dq, 100)], id_mask=m, mask_bits=b, compiled_mask=cm))[0]
            fused = vdb.sparse_index.rrf_fuse([[i for i, _ in dense], [int(i) for i in deep]], 10)
            assert store.search_hybrid(dq, queries[0], 10, flt) == [(name_of[i], s) for i, s in fused]

    steps = [lambda: [put("v%d" % i, sparse=i % 4 != 3) for i in range(60)],
             lambda: put("v5", sparse=False),            # an upsert that drops the sparse vector
             lambda: put("v6"),                          # ... and one that changes it
             lambda: put("v7"),                          # (v7 had none)
             lambda: delete("v8"),
             lambda: store.set_device_filter(True),
             lambda: [put("v%d" % i) for i in (9, 61, 62)],
             lambda: store.compact(),                    # the dense index reclaims its dead rows: sparse answers stay
             lambda: delete("v61"),
             lambda: store.set_device_filter(False),
             lambda: put("v5")]
    for step in steps:
        step()
        check()
