"""The int8 flat index (GpuInt8Index, csrc/kernels_i8.hip) against the numpy reference (i8_data): ids, order, distance bits and
counts, equal or the test fails -- at the K tail and the zero padding, at the segment and query-tile edges read from the index's
own stats, under every k the select serves, on ties, at the accumulator's largest magnitudes, under masks and over a lifecycle."""
import numpy as np
import pytest

import i8_data as D

pytestmark = pytest.mark.gpu
I8, F32, U64 = np.int8, np.float32, np.uint64
METRICS = pytest.mark.parametrize("metric", [D.EUCLID, D.COSINE, D.DOT])


def make(vdb, metric):
    return vdb.GpuInt8Index(vdb.DistanceMetric(metric))


@METRICS
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 200])
def test_k_tail_segment_edges_and_query_tile_edges(vdb, metric, dim):
    """one index grown to 1, R - 1, R, R + 1 and 2 R + 5 rows; 1, QT - 1, QT, QT + 1 and 3 queries; k = 0, 1, 10, 100 and above the
    rows rotating through the batch.  dim = 1 makes most distances ties."""
    ix, rng = make(vdb, metric), np.random.default_rng(dim)
    st = ix.stats()
    R, QT = st["rows_per_segment"], st["query_tile"]
    assert ix.search_batch_arrays(np.ones((2, dim), I8), 3)[2].tolist() == [0, 0]       # an empty index
    ids, rows = np.zeros(0, U64), np.zeros((0, dim), I8)
    for n, nq in [(1, 1), (R - 1, QT - 1), (R, QT), (R + 1, QT + 1), (2 * R + 5, 3)]:
        new = D.random_rows(rng, n - ids.size, dim, metric)
        new_ids = rng.permutation(n - ids.size).astype(U64) * U64(3) + U64(ids.size * 3)
        ix.add_bulk(new_ids, new)
        ids, rows = np.concatenate([ids, new_ids]), np.concatenate([rows, new])
        queries = D.random_rows(rng, nq, dim, metric)
        ks = np.array([(0, 1, 10, 100, n + 7)[(b + n) % 5] for b in range(nq)], dtype=np.uintp)
        D.check(ix, metric, ids, rows, np.ones(n, bool), queries, np.minimum(ks, 128))
        st = ix.stats()
        assert (st["rows"], st["dim"], st["ld"], st["segments"]) == (n, dim, -(-dim // 64) * 64, -(-n // R))
        assert st["workgroups"] == st["segments"] * -(-nq // QT)


@METRICS
@pytest.mark.parametrize("extra", [0, 1], ids=["1500", "R+1500"])
def test_k_1024_on_1500_rows(vdb, metric, extra):
    """the small query tile of large k: 17 queries in two tiles, k = 1024 beside 0, 1 and 1023; every fifth row removed, so a
    segment offers 1200 live rows to buffers of 1088 keys: they are pruned at k = 1024 and the answer is full.  dim = 480 is above
    what the image of that tile holds of a query at once (448 bytes).  With R more rows the merge has two full lists to cut."""
    ix, rng = make(vdb, metric), np.random.default_rng(3)
    n = 1500 + extra * ix.stats()["rows_per_segment"]
    rows, ids = D.random_rows(rng, n, 480, metric), np.arange(n, dtype=U64)[::-1].copy()
    ix.add_bulk(ids, rows)
    live = np.arange(n) % 5 != 0
    for i in np.flatnonzero(~live):
        ix.remove(int(ids[i]))
    ks = np.array([(1024, 0, 1, 1023)[b % 4] for b in range(17)], dtype=np.uintp)
    _, _, counts = D.check(ix, metric, ids, rows, live, D.random_rows(rng, 17, 480, metric), ks)
    assert counts[0] == 1024 and ix.stats()["merge_keys"] == (1 + extra) * int(ks.sum())


@METRICS
def test_ties_across_two_to_the_63(vdb, metric):
    """400 identical rows, ids on both sides of 2^63, between rows that are nearer and farther: the select prunes full buffers of
    one distance and the id rank decides"""
    ix, rng = make(vdb, metric), np.random.default_rng(4)
    rows = np.concatenate([np.tile(np.array([[5, -7, 11, 0, 1]], I8), (400, 1)), D.random_rows(rng, 100, 5, metric)])
    ids = np.concatenate([U64((1 << 63) - 200) + rng.permutation(400).astype(U64), np.arange(100, dtype=U64)])
    perm = rng.permutation(500)
    ix.add_bulk(ids[perm], rows[perm])
    queries = np.array([[5, -7, 11, 0, 1], [1, 1, 1, 1, 1], [-128, 127, -128, 127, 0]], I8)
    for ks in (3, 128, np.array([129, 450, 1024], dtype=np.uintp)):
        D.check(ix, metric, ids[perm], rows[perm], np.ones(500, bool), queries, ks)


@METRICS
def test_largest_magnitudes_at_dim_16384(vdb, metric):
    """rows and queries of all -128 and all 127: s = 2^28, the one asymmetric int8 value, the query image staged in chunks"""
    ix = make(vdb, metric)
    rows = np.repeat(np.array([-128, 127, -128, 127, 1, -1], I8), 16384).reshape(6, 16384)
    rows[4, ::2], rows[5, 1::3] = 127, -128
    ids = np.array([9, 2, 4, 1 << 40, 0, 7], U64)
    ix.add_bulk(ids, rows)
    got = D.check(ix, metric, ids, rows, np.ones(6, bool), rows[[0, 1, 4]], 6)
    if metric == D.DOT:
        assert got[1][0, 0] == -F32(2.0 ** 28) and got[0][0, :2].tolist() == [4, 9]


@METRICS
def test_host_mask_and_compiled_mask_at_a_word_edge(vdb, metric):
    ix, rng = make(vdb, metric), np.random.default_rng(6)
    n, nbits = 200, 128                                  # ids 128 .. 199 lie beyond the mask: never eligible
    rows, ids = D.random_rows(rng, n, 70, metric), np.arange(n, dtype=U64)
    ix.add_bulk(ids, rows)
    queries = D.random_rows(rng, 5, 70, metric)
    table = vdb.MetaTable(0)
    table.set_present(0, nbits, True)
    for on in ([63, 64, 127], [0, 63, 64, 65, 126], []):
        eligible = np.isin(np.arange(n), on)
        words = np.zeros(nbits // 64, U64)
        for i in on:
            words[i >> 6] |= U64(1) << U64(i & 63)
        host = D.check(ix, metric, ids, rows, np.ones(n, bool), queries, 4, eligible, id_mask=words, mask_bits=nbits)
        table.set_codes(0, 0, eligible[:nbits].astype(np.int32))
        with table.compile([(vdb.MetaTable.EQ, 0, 1)], nbits) as cm:
            comp = D.check(ix, metric, ids, rows, np.ones(n, bool), queries, 4, eligible, compiled_mask=cm)
        assert all(np.array_equal(a, b) for a, b in zip(host, comp))


@METRICS
def test_remove_readd_flush_and_zero_norms(vdb, metric):
    ix, rng = make(vdb, metric), np.random.default_rng(7)
    rows, ids = D.random_rows(rng, 300, 33, metric), np.arange(300, dtype=U64) * U64(7)
    queries = D.random_rows(rng, 4, 33, metric)
    ix.add_bulk(ids, rows)
    live = np.ones(300, bool)
    D.check(ix, metric, ids, rows, live, queries, 10)                # searched before any explicit flush
    for i in (0, 17, 299):
        ix.remove(int(ids[i]))
        live[i] = False
    ix.remove(12345)                                                 # absent: no error
    ix.flush()
    D.check(ix, metric, ids, rows, live, queries, 10)
    again = D.random_rows(rng, 2, 33, metric)                        # id 17 * 7 comes back, id 5 * 7 is overwritten: the last vector counts
    ix.add_bulk(ids[[17, 5]], again)
    ids, rows, live = np.concatenate([ids, ids[[17, 5]]]), np.concatenate([rows, again]), np.concatenate([live, [True, True]])
    live[5] = False
    assert ix.len() == 298 and ix.stats()["dead_rows"] == 4
    D.check(ix, metric, ids, rows, live, queries, 300)
    with pytest.raises(vdb.DimensionMismatch):
        ix.add_bulk([1], np.zeros((1, 32), I8))
    with pytest.raises(vdb.DimensionMismatch):
        ix.search_batch_arrays(np.zeros((1, 34), I8), 1)
    with pytest.raises(TypeError):
        ix.search_batch_arrays(queries.astype(np.int16), 1)
    with pytest.raises(TypeError):
        ix.add_bulk([1], np.zeros((1, 33), F32))
    with pytest.raises(TypeError):
        ix.add(1, np.zeros(33, np.uint8))
    # zero norms: an error under Cosine alone, for a live row (masked or not) and for a query; gone with the row
    ix.add(999, np.zeros(33, I8))
    ids, rows, live = np.append(ids, U64(999)), np.concatenate([rows, np.zeros((1, 33), I8)]), np.append(live, True)
    zq = np.concatenate([queries, np.zeros((1, 33), I8)])
    if metric == D.COSINE:
        with pytest.raises(vdb.InvalidVector):
            ix.search_batch_arrays(queries, 3, id_mask=np.ones(1, U64), mask_bits=64)
        ix.remove(999)
        live[-1] = False
        with pytest.raises(vdb.InvalidVector):
            ix.search_batch_arrays(zq, 3)
        D.check(ix, metric, ids, rows, live, queries, 3)
    else:
        D.check(ix, metric, ids, rows, live, zq, 302)


def test_dot_equals_the_dense_index_over_the_widened_values(vdb):
    """dim <= 1024: every integer sum is below 2^24, so the f32 pipeline's sums are exact too"""
    rng = np.random.default_rng(8)
    rows, queries = D.random_rows(rng, 3000, 96, D.DOT), D.random_rows(rng, 9, 96, D.DOT)
    ids = rng.permutation(3000).astype(U64)
    ix, dense = make(vdb, D.DOT), vdb.GpuFlatIndex(vdb.DistanceMetric.DotProduct, device=0, keep_host_copy=False)
    ix.add_bulk(ids, rows)
    dense.add_bulk(rows.astype(F32), ids=ids)
    a, b = ix.search_batch_arrays(queries, 20), dense.search_batch_arrays(queries.astype(F32), 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2].tolist() == list(b[2])


def test_vector_store_life(vdb):
    rng = np.random.default_rng(9)
    store = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    with pytest.raises(ValueError):
        store.insert_with_metadata("a", vdb.Vector([0.0, 1.0]), vdb.Metadata(), int8=np.zeros(8, I8))
    store.enable_int8()
    vecs = rng.integers(-128, 128, size=(40, 8), dtype=I8)
    for i in range(40):
        store.insert_with_metadata(f"r{i}", vdb.Vector([float(i), 1.0]), vdb.Metadata({"color": "red" if i % 2 else "blue"}), int8=vecs[i])
    vecs[3] = vecs[10]
    store.insert_with_metadata("r3", vdb.Vector([3.0, 1.0]), vdb.Metadata({"color": "red"}), int8=vecs[3])   # upsert
    store.delete("r10")
    q = vecs[10]
    live = np.arange(40) != 10
    flt = vdb.MetadataFilter.Eq("color", "red")
    for f, eligible in ((None, live), (flt, live & (np.arange(40) % 2 == 1))):
        (wi, wd), = D.search(D.EUCLID, np.arange(40), vecs, np.ones(40, bool), q[None, :], 5, eligible)
        got = store.search_int8(q, 5, f)
        assert [r.id for r in got] == [f"r{i}" for i in wi] and [F32(r.distance) for r in got] == wd.tolist()
    assert got[0].id == "r3" and got[0].distance == 0.0
