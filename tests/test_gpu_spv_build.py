"""The sparse-vector index's BUILD (csrc/kernels_spv.hip: histogram, scan, scatter; csrc/vdb_spv.cpp: the append log) at the
shapes where its loops step and its clamps bite, through searches against the CSR reference (spv_data.search_csr): ids, order,
distance bits, counts, entries_walked and candidates must be equal."""
import time

import numpy as np
import pytest

import spv_data as S

pytestmark = pytest.mark.gpu
U32, F32, U64 = np.uint32, np.float32, np.uint64


def random_rows(rng, n, top, lo=1, hi=30, plant=()):
    """n rows of lo..hi distinct indices over [0, top]; every index of `plant` and `top` itself is put into a handful of rows"""
    vecs = []
    for r in range(n):
        idx = np.unique(rng.integers(0, top + 1, size=rng.integers(lo, hi + 1)))
        vecs.append(rng.permutation(idx))
    for j, d in enumerate(list(plant) + [top]):
        for r in rng.choice(n, size=min(n, 3 + j % 3), replace=False):
            if d not in vecs[r]:
                vecs[r] = np.append(vecs[r], d)
    return [(v.astype(U32), rng.standard_normal(v.size).astype(F32)) for v in vecs]


def build(vdb, ids, vecs):
    offsets, indices, values = S.csr_of(vecs)
    ix = vdb.GpuSparseIndex()
    ix.add_csr(ids, offsets, indices, values)
    return ix, (np.asarray(ids, dtype=U64), offsets, indices, values, np.ones(len(vecs), dtype=bool))


def some_ids(rng, n):
    ids = rng.permutation(n).astype(U64) * U64(3) + U64(1)
    ids[n // 2] += U64(1 << 32)
    return ids


def chunk_edges(vocab):
    """first and last index of the scan's chunks 0, 1, a middle one, the last but one and the last non-empty one; 0 and vocab - 1"""
    chunk = -(-vocab // 1024)
    last = (vocab - 1) // chunk
    out = {0, vocab - 1}
    for t in {0, 1, last // 2, max(last - 1, 0), last}:
        out |= {t * chunk, min((t + 1) * chunk, vocab) - 1}
    return sorted(out)


@pytest.mark.parametrize("top", [1023, 1024, 1025, 2047, 2048, 3000, 30521])
def test_scan_chunking(vdb, top):
    """vocab = top + 1: thread t of the scan owns [t * chunk, (t + 1) * chunk) clamped at vocab, chunk = 1, 2, 2, 2, 3, 3, 30.  A wrong
    carry between chunks, or a chunk read past vocab, moves every list behind it."""
    rng = np.random.default_rng(top)
    vocab = top + 1
    edges = chunk_edges(vocab)
    ix, C = build(vdb, some_ids(rng, 2000), random_rows(rng, 2000, top, plant=edges))
    view = S.csc_view(C[1], C[2])
    e = np.array(edges, dtype=U32)
    queries = [(e[::-1], rng.standard_normal(e.size).astype(F32)), (e[:2], np.ones(2, F32)), (e[-2:], np.array([1.0, -1.0], F32)),
               (np.array([0, top], U32), np.array([0.5, 2.0], F32))]
    for _ in range(4):
        idx = rng.choice(vocab, size=200, replace=False).astype(U32)
        queries.append((idx, rng.standard_normal(idx.size).astype(F32)))
    S.check_csr(ix, C, queries, 50, view=view)
    assert ix.stats()["vocab"] == vocab
    for q in queries[:4]:
        assert ix.search_batch_arrays([q], 50)[2][0] > 0


def test_scan_chunk_of_16384(vdb):
    """largest stored index 2^24 - 1, the largest the index takes: chunk = 16384, and the last list is the last word of list_ptr"""
    rng = np.random.default_rng(24)
    top = (1 << 24) - 1
    ix, C = build(vdb, some_ids(rng, 300), random_rows(rng, 300, top, plant=[top - 1, 16384, 16383, 5 * 16384]))
    queries = [(np.array([top], U32), np.ones(1, F32)), (np.array([top, 16384, 0, top - 1, 16383, 5 * 16384], U32), np.arange(1, 7, dtype=F32))]
    S.check_csr(ix, C, queries, 20)
    assert ix.stats()["vocab"] == 1 << 24 and 3 <= ix.search_batch_arrays(queries[:1], 20)[2][0] <= 5


def test_vocabulary_bound_and_its_growth(vdb):
    rng = np.random.default_rng(1501)
    top = 1500                                           # vocab 1501: chunk 2, the last thread that owns anything owns one index
    vecs = random_rows(rng, 500, top)
    ids = some_ids(rng, 500)
    ix, C = build(vdb, ids, vecs)
    vocab = top + 1
    queries = [(np.array([vocab, 3], U32), np.array([1.0, 2.0], F32)), (np.array([vocab + 1, top], U32), np.array([1.0, 2.0], F32)),
               (np.array([(1 << 24) - 1, vocab + 1, vocab, 7, 8, 9], U32), np.arange(1, 7, dtype=F32)),
               (np.array([vocab, vocab + 1], U32), np.ones(2, F32))]
    before = S.check_csr(ix, C, queries, 30)
    assert before[2][3] == 0
    new_id = 999_999
    ix.add(new_id, [vocab + 1, 7], [5.0, -1.0])
    vecs2 = vecs + [(np.array([vocab + 1, 7], U32), np.array([5.0, -1.0], F32))]
    offsets, indices, values = S.csr_of(vecs2)
    C2 = (np.append(ids, U64(new_id)), offsets, indices, values, np.ones(501, dtype=bool))
    after = S.check_csr(ix, C2, queries, 30)
    st = ix.stats()
    assert st["vocab"] == vocab + 2 and st["rebuilds"] == 2
    assert after[2][3] == 1 and after[0][3, 0] == new_id
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(after, before))          # query 0 holds neither of the new row's indices
    for b in (1, 2):                                     # every earlier answer is there, in its order, around the new row
        got = [(int(i), d.tobytes()) for i, d in zip(after[0][b, :after[2][b]], after[1][b, :after[2][b]]) if i != new_id]
        want = [(int(i), d.tobytes()) for i, d in zip(before[0][b, :before[2][b]], before[1][b, :before[2][b]])]
        assert new_id in after[0][b, :after[2][b]] and got == want[:len(got)] and len(got) >= min(len(want), 29)


LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)


def rows_of_lengths(rng, lengths, top=2999):
    vecs = []
    for n in lengths:
        idx = rng.choice(top + 1, size=n, replace=False).astype(U32)
        vecs.append((idx, rng.standard_normal(n).astype(F32)))
    return vecs


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 44])
def test_long_and_empty_rows(vdb, n_rows):
    """a wave strides a row with e += 64: rows of 0, 1, 63, 64, 65, 128, 129 and 1000 entries, in partial and full blocks of four
    waves (every rotation of the lengths), and among 36 ordinary rows"""
    rng = np.random.default_rng(n_rows)
    wide = (rng.permutation(3000)[:1024].astype(U32), rng.standard_normal(1024).astype(F32))
    for start in range(len(LENGTHS) if n_rows < 44 else 1):
        lengths = [LENGTHS[(start + i) % len(LENGTHS)] for i in range(min(n_rows, len(LENGTHS)))]
        if n_rows == 44:
            lengths = list(rng.permutation(lengths + list(rng.integers(1, 31, size=36))))
        vecs = rows_of_lengths(rng, lengths)
        ix, C = build(vdb, some_ids(rng, len(vecs)), vecs)
        queries = [wide] + [(v[0][:7], np.ones(min(7, v[0].size), F32)) for v in vecs]      # an empty row's own (empty) query too
        out_ids, _, counts = S.check_csr(ix, C, queries, 50)
        st = ix.stats()
        assert len(ix) == len(vecs) == st["rows"] and st["nnz"] == sum(lengths)
        for r, n in enumerate(lengths):
            if n == 0:
                assert not (out_ids[np.arange(50)[None, :] < counts[:, None]] == C[0][r]).any()
            else:
                assert counts[1 + r] >= 1 and C[0][r] in out_ids[1 + r, :counts[1 + r]]


def test_empty_rows_live_and_die_like_others(vdb):
    ix = vdb.GpuSparseIndex()
    none = (np.zeros(0, U32), np.zeros(0, F32))
    ix.add_bulk([5, 6, 7], [none, none, none])
    q = [(np.array([0, 1], U32), np.ones(2, F32))]
    assert ix.search_batch_arrays(q, 5)[2][0] == 0       # every row is empty: vocab 0, nothing to walk, no error
    st = ix.stats()
    assert (len(ix), st["rows"], st["nnz"], st["vocab"], st["entries_walked"], st["candidates"]) == (3, 3, 0, 0, 0, 0)
    ix.remove(6)
    ix.add(5, [1], [2.0])                                # an empty row overwritten
    ix.add(8, [1, 0], [1.0, 1.0])
    ix.add(8, [], [])                                    # ... and a row overwritten by an empty one
    C = (np.array([5, 6, 7, 5, 8, 8], U64),) + S.csr_of([none, none, none, ([1], [2.0]), ([1, 0], [1.0, 1.0]), none]) + (
        np.array([0, 0, 1, 1, 0, 1], dtype=bool),)
    out_ids, _, counts = S.check_csr(ix, C, q, 5)
    st = ix.stats()
    assert counts[0] == 1 and out_ids[0, 0] == 5
    assert (len(ix), st["rows"], st["dead_rows"], st["nnz"], st["vocab"]) == (3, 6, 3, 3, 2)


def test_row_grid_stride(vdb):
    """4 * 2^20 + 5 rows: the build kernels' grids end at 2^20 blocks of four waves, so the last five rows are reached by row += waves
    alone, in the wave slots of rows 0 .. 4.  (The one test here that takes more than a few seconds; its duration is printed.)"""
    t0 = time.time()
    n = 4 * (1 << 20) + 5
    rows = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(4)
    indices = rng.integers(0, 64, size=n).astype(U32)
    values = (rows % 8191).astype(F32)
    offsets = np.arange(n + 1, dtype=np.int64)
    ids = rows.astype(U64)
    ix = vdb.GpuSparseIndex()
    ix.add_csr(ids, offsets, indices, values)
    C = (ids, offsets, indices, values, np.ones(n, dtype=bool))
    view = S.csc_view(offsets, indices)
    tail = indices[-5:]
    queries = [(np.array([int(tail[0])], U32), np.ones(1, F32)),
               (np.array([int(tail[1]), (int(tail[1]) + 1) % 64, (int(tail[1]) + 9) % 64], U32), np.array([1.0, -2.0, 0.5], F32))]
    S.check_csr(ix, C, queries, 1024, view=view)         # entries_walked and candidates count the last five rows
    eligible = rows >= n - 10                            # ... and under a mask that admits only the last ten they are the answer
    every = (np.arange(64, dtype=U32), np.ones(64, F32))
    out_ids, _, counts = S.check_csr(ix, C, [every], 1024, eligible, S.big_mask(ids, eligible, n), n, view=view)
    assert counts[0] == 10 and set(out_ids[0, :10].tolist()) == set(range(n - 10, n))
    assert ix.stats()["rows"] == n and ix.stats()["rebuilds"] == 1
    print("test_row_grid_stride: %.1f s" % (time.time() - t0))


def test_one_id_twice_in_one_call_and_a_refused_call(vdb):
    ix = vdb.GpuSparseIndex()
    a, b, c = ([1, 2], [1.0, 1.0]), ([2, 3], [4.0, 4.0]), ([3, 1], [9.0, 9.0])
    ix.add_bulk([10, 11, 10], [a, b, c])                 # the last vector of id 10 wins
    C = (np.array([10, 11, 10], U64),) + S.csr_of([a, b, c]) + (np.array([0, 1, 1], dtype=bool),)
    queries = [(np.array([1], U32), np.ones(1, F32)), (np.array([2], U32), np.ones(1, F32)), (np.array([3, 2, 1], U32), np.ones(3, F32))]
    first = S.check_csr(ix, C, queries, 5)
    st = ix.stats()
    assert (len(ix), st["rows"], st["dead_rows"], st["rebuilds"]) == (2, 3, 1, 1)
    with pytest.raises(vdb.IndexError_):                 # the middle row repeats an index: nothing of the call is stored
        ix.add_bulk([12, 11, 13], [a, ([5, 7, 5], [1.0, 2.0, 3.0]), c])
    assert len(ix) == 2 and ix.stats() == st
    again = S.check_csr(ix, C, queries, 5)
    assert ix.stats()["rebuilds"] == 1 and all(np.array_equal(x, y) for x, y in zip(first, again))
