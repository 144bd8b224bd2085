"""The sparse-vector index on the device (vdb_spv_*, csrc/kernels_spv.hip) against the numpy restatement of its definition
(spv_data.py): ids, order, distance BITS and counts must be equal, at the cases where the kernels can go wrong."""
import numpy as np
import pytest

import spv_data as S

pytestmark = pytest.mark.gpu
BITS = 18000                                             # every small id of the corpus is below it; the huge ones are not


@pytest.fixture(scope="module")
def data():
    return S.corpus()


def build(vdb, data):
    ix = vdb.GpuSparseIndex()
    ix.add_bulk(data[0], S.vectors(data[1], data[2]))
    return ix


@pytest.fixture(scope="module")
def index(vdb, data):
    return build(vdb, data)


def check(ix, data, queries, k, eligible=None, mask=None):
    ids, X, P = data
    out_ids, out_d, counts = ix.search_batch_arrays(queries, k, id_mask=mask, mask_bits=BITS if mask is not None else 0)
    ks = np.full(len(queries), k) if np.isscalar(k) else k
    for b, q in enumerate(queries):
        ei, ed = S.search(ids, X, P, q, int(ks[b]), eligible)
        assert counts[b] == ei.size, (b, counts[b], ei.size)
        assert np.array_equal(out_ids[b, :ei.size], ei), b
        assert np.array_equal(out_d[b, :ei.size].view(np.uint32), ed.view(np.uint32)), b
    return out_ids, out_d, counts


def row_query(data, row):
    return np.flatnonzero(data[2][row]).astype(np.uint32), data[1][row][data[2][row]]


def batch(seed, nq):
    rng = np.random.default_rng(seed)
    qs = []
    for _ in range(nq):
        idx = rng.choice(500, size=rng.integers(1, 41), replace=False).astype(np.uint32)   # unsorted; some indices no row has
        qs.append((idx, rng.standard_normal(idx.size).astype(np.float32)))
    return qs, rng.integers(0, 60, size=nq).astype(np.uintp)


WIDE = (np.arange(0, 40, dtype=np.uint32), np.linspace(-1.0, 1.0, 40, dtype=np.float32))   # indices 7, 8, 9 and 37 more
CASES = {
    # index 7 is in ~2640 rows: its list takes three strides of the 1024 threads; also the one-non-zero query
    "one_long_list": ([(np.array([7], np.uint32), np.array([-1.5], np.float32))], 10),
    # index 100: below the vocabulary bound, no row has it; 490 and 2^24 - 1: above the bound (471)
    "absent_and_above": ([(np.array([(1 << 24) - 1, 100, 490, 7], np.uint32), np.array([1, 2, 3, 0.5], np.float32))], 25),
    "only_absent": ([(np.array([100, 490], np.uint32), np.array([1, 2], np.float32))], 5),
    "overflow_k10": ([WIDE], 10),
    "overflow_k1024": ([WIDE], 1024),
    # ten rows hold index 470: count < k, and the 5990 rows without overlap never come back
    "count_below_k": ([(np.array([470], np.uint32), np.array([2.0], np.float32))], 50),
}


@pytest.mark.parametrize("name", CASES)
def test_cases(index, data, name):
    queries, k = CASES[name]
    check(index, data, queries, k)
    if name.startswith("overflow"):
        assert index.stats()["candidates"] > 4096        # more than the select buffer holds: it was pruned on the way


def test_ties_by_id_across_2_pow_32(index, data):
    out_ids, _, _ = check(index, data, [row_query(data, 10)], 8)
    assert set(data[0][10:14].tolist()) <= set(out_ids[0].tolist())     # rows 10-13 are identical: one score, four ids


def test_id_mask_negative_weights_and_explicit_zero(index, data):
    ids = data[0]
    eligible = (np.arange(ids.size) % 5 == 0)
    out_ids, out_d, counts = check(index, data, [CASES["one_long_list"][0][0], WIDE], 1024, eligible & (ids < BITS),
                                   S.id_mask(ids, eligible, BITS))
    at = np.flatnonzero(out_ids[0, :counts[0]] == ids[20])
    assert at.size == 1 and out_d[0, at[0]].view(np.uint32) == 0x80000000    # -1.5 * 0.0 = -0.0, s = +0.0, distance -0.0


@pytest.mark.parametrize("nq", [1, 7, 33])
def test_batches_with_per_query_k(index, data, nq):
    qs, ks = batch(nq, nq)
    check(index, data, qs, ks)
    walked = sum(int(data[2][:, d].sum()) for q, _ in qs for d in q if d < S.VOCAB)
    assert index.stats()["entries_walked"] == walked and index.stats()["chunks"] == 1


def test_lowered_workspace_cap_takes_several_chunks(vdb, data):
    ix = build(vdb, data)
    ix.debug_set_workspace_cap(4 * data[0].size * 5)     # five accumulator slots
    qs, ks = batch(33, 33)
    check(ix, data, qs, ks)
    assert ix.stats()["chunks"] == 7


def test_accumulators_are_clean_after_every_call(vdb, index, data):
    (qa, ka), (qb, kb) = batch(101, 7), batch(102, 7)
    qa = qa + [WIDE]
    ka = np.append(ka, 1024).astype(np.uintp)
    first = check(index, data, qa, ka)
    again = check(index, data, qa, ka)
    then = check(index, data, qb, kb)
    fresh = build(vdb, data)
    for got, want in ((again, first), (then, fresh.search_batch_arrays(qb, kb)), (first, fresh.search_batch_arrays(qa, ka))):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_removed_and_overwritten_ids(vdb, data):
    ids, X, P = data[0], data[1].copy(), data[2].copy()
    ix = build(vdb, data)
    assert ix.stats()["rebuilds"] == 0
    q = [row_query(data, 6), row_query(data, 5), CASES["count_below_k"][0][0]]
    check(ix, data, q, 20)
    ix.remove(int(ids[5]))
    ix.remove(12345678)                                  # absent: fine
    ix.add(int(ids[6]), [470], [3.0])                    # no longer overlaps its old self
    ix.add(int(ids[7]), [3, 1, 2], [1.0, -2.0, 0.5])
    X[6], P[6], X[7], P[7] = 0, False, 0, False
    X[6, 470], P[6, 470] = 3.0, True
    X[7, [3, 1, 2]], P[7, [3, 1, 2]] = [1.0, -2.0, 0.5], True
    alive = np.ones(ids.size, dtype=bool)
    alive[5] = False
    check(ix, (ids, X, P), q + [(np.array([1, 2, 3], np.uint32), np.ones(3, np.float32))], 20, alive)
    st = ix.stats()
    assert len(ix) == ids.size - 1 and st["rows"] == ids.size + 2 and st["dead_rows"] == 3 and st["rebuilds"] == 2


def test_nan_only_from_an_eligible_row(vdb):
    inf = np.float32(np.inf)
    ix = vdb.GpuSparseIndex()
    ids = np.array([1, 2, 3], dtype=np.uint64)
    X = np.zeros((3, S.VOCAB), np.float32)
    P = np.zeros((3, S.VOCAB), bool)
    X[0, [1, 2]], X[1, [1, 2]], X[2, 2] = [inf, -inf], [inf, inf], 4.0
    P[:2, [1, 2]] = True
    P[2, 2] = True
    ix.add_bulk(ids, S.vectors(X, P))
    q = [(np.array([1, 2], np.uint32), np.ones(2, np.float32))]
    with pytest.raises(vdb.NanDistance):                 # row 0: inf - inf
        ix.search_batch_arrays(q, 3)
    elig = np.array([False, True, True])
    check(ix, (ids, X, P), q, 3, elig, S.id_mask(ids, elig, BITS))      # masked out: +inf scores are ordinary
    ix.remove(1)
    check(ix, (ids, X, P), q, 3, elig)


def test_refusals(vdb, index):
    one = np.array([1.0], np.float32)
    for bad in ([(np.array([3, 3], np.uint32), np.ones(2, np.float32))], [(np.array([1 << 24], np.uint32), one)],
                [(np.arange(1025, dtype=np.uint32), np.ones(1025, np.float32))]):
        with pytest.raises(vdb.IndexError_):
            index.search_batch_arrays(bad, 1)
    with pytest.raises(vdb.IndexError_):
        index.search_batch_arrays([(np.array([1], np.uint32), one)], 1025)
    with pytest.raises(vdb.IndexError_):
        index.add(1, [5, 5], [1.0, 2.0])


def test_vector_store_sparse_and_hybrid(vdb, data):
    ids, X, P = data
    n, rng = 300, np.random.default_rng(5)
    dense = rng.random((n + 1, 16), dtype=np.float32)
    vs = S.vectors(X[:n], P[:n])
    store = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    store.enable_sparse()
    store.insert_batch([vdb.BatchInsertItem(f"v{i}", vdb.Vector(dense[i]), vdb.Metadata({"c": "a" if i % 3 else "b"}), sparse=vs[i])
                        for i in range(n)])
    store.insert_with_metadata("v4", vdb.Vector(dense[n]), vdb.Metadata({"c": "a"}), sparse=vs[8])   # upsert: internal id n
    store.delete("v5")
    flt = vdb.MetadataFilter.Eq("c", "a")
    name = {i: f"v{i}" for i in range(n)}
    name[n] = "v4"
    internal = np.arange(n + 1, dtype=np.uint64)
    Xs, Ps = np.vstack([X[:n], X[8:9]]), np.vstack([P[:n], P[8:9]])
    elig = np.array([i % 3 != 0 for i in range(n)] + [True])
    elig[[4, 5]] = False
    q = (WIDE[0], WIDE[1])
    ei, ed = S.search(internal, Xs, Ps, q, 10, elig)
    got = store.search_sparse(q, 10, flt)
    assert [r.id for r in got] == [name[int(i)] for i in ei]
    assert np.array_equal(np.array([r.distance for r in got], np.float32).view(np.uint32), ed.view(np.uint32))
    si, _ = S.search(internal, Xs, Ps, q, 100, elig)
    dq = vdb.Vector(dense[17])
    di = [store._id_to_internal[r.id] for r in store.search_batch_prefiltered([(dq, 100)], flt)[0]]
    want = vdb.sparse_index.rrf_fuse([di, [int(i) for i in si]], 10)
    assert store.search_hybrid(dq, q, 10, flt) == [(name[i], s) for i, s in want]
