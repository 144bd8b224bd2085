"""The binary flat index (GpuBinaryIndex, csrc/kernels_bin.hip) against the numpy reference (bin_data): ids, order, distance bits
and counts, equal or the test fails -- at the chunk and K edges, at the segment and query-tile edges read from the index's own
stats, on ties (the normal case under Hamming), under a threshold shared between workgroups, at the largest k and sums, under
masks and over a lifecycle."""
import numpy as np
import pytest

import bin_data as D

pytestmark = pytest.mark.gpu
U8, F32, U64 = np.uint8, np.float32, np.uint64
METRICS = pytest.mark.parametrize("metric", [D.HAMMING, D.JACCARD])


def make(vdb, metric):
    return vdb.GpuBinaryIndex(vdb.BinaryMetric(metric))


@METRICS
@pytest.mark.parametrize("density", [0.5, 0.02])
@pytest.mark.parametrize("dim", [8, 504, 512, 520, 1032])
def test_chunk_edges_segment_edges_and_query_tile_edges(vdb, metric, dim, density):
    """one index grown to 1, 100, R - 1, R, R + 1 and 2 R + 5 rows; 1, 5, QT - 1, QT, QT + 1 and 3 queries; k rotating through 0, 1,
    10, 100 and n + 7 -- above the rows at 1 row (k = 8, the one query) and at 100 rows (k = 107), cut to 128 at the larger steps
    so that the 64-query tile serves every step.  At R + 1 rows a mask leaves five rows on both sides of the segment edge to
    k = 10: a count below k out of two workgroups.  Sparse rows make u small and Jaccard ties common; 8 bits make nearly
    everything a tie."""
    ix, rng = make(vdb, metric), np.random.default_rng(dim)
    st = ix.stats()
    R, QT = st["rows_per_segment"], st["query_tile"]
    assert ix.search_batch_arrays(np.ones((2, dim // 8), U8), 3)[2].tolist() == [0, 0]   # an empty index
    ids, rows = np.zeros(0, U64), np.zeros((0, dim // 8), U8)
    for n, nq in [(1, 1), (100, 5), (R - 1, QT - 1), (R, QT), (R + 1, QT + 1), (2 * R + 5, 3)]:
        new = D.random_rows(rng, n - ids.size, dim, density)
        new_ids = rng.permutation(n - ids.size).astype(U64) * U64(3) + U64(ids.size * 3)
        ix.add_bulk(new_ids, new)
        ids, rows = np.concatenate([ids, new_ids]), np.concatenate([rows, new])
        queries = D.random_rows(rng, nq, dim, density)
        ks = np.array([(0, 1, 10, 100, min(n + 7, 128))[(b + n + 3) % 5] for b in range(nq)], dtype=np.uintp)
        assert (ks > n).any() == (n <= 100)
        D.check(ix, metric, ids, rows, np.ones(n, bool), queries, ks)
        st = ix.stats()
        assert (st["rows"], st["dim"], st["ld"], st["segments"]) == (n, dim, -(-dim // 512) * 64, -(-n // R))
        assert st["workgroups"] == st["segments"] * -(-nq // QT)
        if n == R + 1:
            eligible = np.zeros(n, bool)
            eligible[R - 4:] = True                                  # four rows of the first segment, the one row of the second
            words = np.zeros(int(ids.max()) // 64 + 1, U64)
            for i in ids[eligible]:
                words[int(i) >> 6] |= U64(1) << U64(int(i) & 63)
            got = D.check(ix, metric, ids, rows, np.ones(n, bool), queries[:3], 10, eligible, id_mask=words, mask_bits=words.size * 64)
            assert got[2].tolist() == [5, 5, 5]


@METRICS
def test_ties_across_two_to_the_63_over_two_segments(vdb, metric):
    """600 identical rows, ids on both sides of 2^63, among nearer and farther rows and spread over two segments: the select
    prunes full buffers of one distance and the id rank decides"""
    ix, rng = make(vdb, metric), np.random.default_rng(4)
    R = ix.stats()["rows_per_segment"]
    n = R + 400
    rows = D.random_rows(rng, n, 64, 0.5)
    same = np.arange(R - 300, R + 300)
    rows[same] = np.array([0xF0, 0x0F, 0xAA, 0x55, 0, 0xFF, 1, 0x80], U8)
    ids = np.arange(n, dtype=U64)
    ids[same] = U64((1 << 63) - 300) + rng.permutation(600).astype(U64)
    ix.add_bulk(ids, rows)
    queries = np.array([[0xF0, 0x0F, 0xAA, 0x55, 0, 0xFF, 1, 0x80], [0xF0, 0x0F, 0xAA, 0x55, 0, 0xFF, 0, 0], [0] * 8], U8)
    for ks in (3, 128, np.array([129, 700, 1024], dtype=np.uintp)):
        D.check(ix, metric, ids, rows, np.ones(n, bool), queries, ks)


@METRICS
@pytest.mark.parametrize("k", [100, 1024])
def test_nine_distinct_distances_at_dim_8(vdb, metric, k):
    ix, rng = make(vdb, metric), np.random.default_rng(5)
    rows, ids = D.random_rows(rng, 3000, 8, 0.5), rng.permutation(3000).astype(U64) << U64(40)
    ix.add_bulk(ids, rows)
    D.check(ix, metric, ids, rows, np.ones(3000, bool), D.random_rows(rng, 5, 8, 0.5), k)


@METRICS
@pytest.mark.parametrize("where", ["last", "first"])
def test_the_shared_threshold_cannot_lose_an_answer(vdb, metric, where):
    """3 R + 7 rows whose 1024 nearest all lie in one segment: the other segments' workgroups may have published thresholds of
    their own before or after it runs.  Two searches of the same index must give equal arrays."""
    ix, rng = make(vdb, metric), np.random.default_rng(6)
    n = 3 * ix.stats()["rows_per_segment"] + 7
    queries = D.random_rows(rng, 3, 256, 0.5)
    rows = D.random_rows(rng, n, 256, 0.5)
    near = queries[rng.integers(0, 3, 1100)] ^ D.random_rows(rng, 1100, 256, 0.03)
    if where == "last":
        rows[n - 1100:] = near
    else:
        rows[:1100] = near
    ids = rng.permutation(n).astype(U64)
    ix.add_bulk(ids, rows)
    for k in (10, 1024):
        first = D.check(ix, metric, ids, rows, np.ones(n, bool), queries, k)
        again = ix.search_batch_arrays(queries, k)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))


@METRICS
@pytest.mark.parametrize("extra", [0, 1], ids=["1500", "R+1500"])
def test_k_1024_on_1500_rows(vdb, metric, extra):
    """the small query tile of large k: 17 queries in two tiles, k = 1024 beside 0, 1 and 1023; every fifth row removed, so a
    segment offers 1200 live rows to buffers of 1088 keys: they are pruned at k = 1024 and the answer is full.  4096 bits are four
    times what that tile's image holds of a query at once.  With R more rows the merge has two full lists to cut."""
    ix, rng = make(vdb, metric), np.random.default_rng(3)
    n = 1500 + extra * ix.stats()["rows_per_segment"]
    rows, ids = D.random_rows(rng, n, 4096, 0.3), np.arange(n, dtype=U64)[::-1].copy()
    ix.add_bulk(ids, rows)
    live = np.arange(n) % 5 != 0
    for i in np.flatnonzero(~live):
        ix.remove(int(ids[i]))
    ks = np.array([(1024, 0, 1, 1023)[b % 4] for b in range(17)], dtype=np.uintp)
    _, _, counts = D.check(ix, metric, ids, rows, live, D.random_rows(rng, 17, 4096, 0.3), ks)
    assert counts[0] == 1024


@METRICS
def test_extremes_at_32768_bits(vdb, metric):
    """all ones, all zeros and alternating bytes: the largest sums (a = h = 32768), every image chunk, and an all-zero query
    against an all-zero row under Jaccard (u = 0: +0.0)"""
    ix = make(vdb, metric)
    rows = np.zeros((6, 4096), U8)
    rows[0], rows[2, ::2], rows[3, 1::2], rows[4], rows[5, 4095] = 255, 255, 255, 0xAA, 1
    ids = np.array([9, 2, 4, 1 << 40, 0, 7], U64)
    ix.add_bulk(ids, rows)
    got = D.check(ix, metric, ids, rows, np.ones(6, bool), rows[[0, 1, 2, 4]], 6)
    assert got[1][0, 5] == (32768.0 if metric == D.HAMMING else 1.0) and got[0][1, 0] == 2 and got[1][1, 0].view(np.uint32) == 0


@METRICS
def test_host_mask_and_compiled_mask_at_a_word_edge(vdb, metric):
    ix, rng = make(vdb, metric), np.random.default_rng(6)
    n, nbits = 200, 128                                  # ids 128 .. 199 lie beyond the mask: never eligible
    rows, ids = D.random_rows(rng, n, 72, 0.5), np.arange(n, dtype=U64)
    ix.add_bulk(ids, rows)
    queries = D.random_rows(rng, 5, 72, 0.5)
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
def test_remove_readd_flush_and_refused_dims(vdb, metric):
    ix, rng = make(vdb, metric), np.random.default_rng(7)
    L, invalid = ix._L, 5                                            # VDB_ERR_INVALID_ARGUMENT, straight from the C boundary
    u64p, u8p = L.vdb_bin_add_bulk.argtypes[1:3]
    one, wide = np.ones(1, U64), np.zeros((1, 4097), U8)
    assert L.vdb_bin_add_bulk(ix._h, one.ctypes.data_as(u64p), wide.ctypes.data_as(u8p), 1, 32776) == invalid
    assert len(ix) == 0                                              # nothing is stored, the dimension stays open
    rows, ids = D.random_rows(rng, 300, 40, 0.4), np.arange(300, dtype=U64) * U64(7)
    queries = D.random_rows(rng, 4, 40, 0.4)
    ix.add_bulk(ids, rows)
    live = np.ones(300, bool)
    D.check(ix, metric, ids, rows, live, queries, 10)                # searched before any explicit flush
    for i in (0, 17, 299):
        ix.remove(int(ids[i]))
        live[i] = False
    ix.remove(12345)                                                 # absent: no error
    ix.flush()
    D.check(ix, metric, ids, rows, live, queries, 10)
    again = D.random_rows(rng, 2, 40, 0.4)                           # id 17 * 7 comes back, id 5 * 7 is overwritten: the last vector counts
    ix.add_bulk(ids[[17, 5]], again)
    ids, rows, live = np.concatenate([ids, ids[[17, 5]]]), np.concatenate([rows, again]), np.concatenate([live, [True, True]])
    live[5] = False
    assert len(ix) == 298 and ix.stats()["dead_rows"] == 4
    D.check(ix, metric, ids, rows, live, queries, 300)
    with pytest.raises(vdb.DimensionMismatch):
        ix.add_bulk([1], np.zeros((1, 4), U8))
    with pytest.raises(vdb.DimensionMismatch):
        ix.search_batch_arrays(np.zeros((1, 6), U8), 1)
    assert L.vdb_bin_add_bulk(ix._h, one.ctypes.data_as(u64p), wide.ctypes.data_as(u8p), 1, 12) == invalid   # 12 bits: no whole bytes
    assert len(ix) == 298
    with pytest.raises(TypeError):
        ix.search_batch_arrays(queries.astype(np.int8), 1)


def test_hamming_equals_the_int8_index_over_the_widened_bits(vdb):
    rng = np.random.default_rng(8)
    rows, queries = D.random_rows(rng, 3000, 96, 0.5), D.random_rows(rng, 9, 96, 0.5)
    ids = rng.permutation(3000).astype(U64)
    ix, wide = make(vdb, D.HAMMING), vdb.GpuInt8Index(vdb.DistanceMetric.Euclidean)
    ix.add_bulk(ids, rows)
    wide.add_bulk(ids, np.unpackbits(rows, axis=1).astype(np.int8))
    a, b = ix.search_batch_arrays(queries, 20), wide.search_batch_arrays(np.unpackbits(queries, axis=1).astype(np.int8), 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(np.sqrt(a[1]).view(np.uint32), b[1].view(np.uint32)) and a[2].tolist() == list(b[2])


@pytest.mark.parametrize("device_filter", [False, True])
def test_vector_store_life(vdb, device_filter):
    rng = np.random.default_rng(9)
    store = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    store.set_device_filter(device_filter)
    with pytest.raises(ValueError):
        store.insert_with_metadata("a", vdb.Vector([0.0, 1.0]), vdb.Metadata(), binary=np.zeros(8, U8))
    store.enable_binary(vdb.BinaryMetric.Hamming)
    vecs = D.random_rows(rng, 40, 64, 0.5)
    for i in range(40):
        store.insert_with_metadata(f"r{i}", vdb.Vector([float(i), 1.0]), vdb.Metadata({"color": "red" if i % 2 else "blue"}), binary=vecs[i])
    vecs[3] = vecs[10]
    store.insert_with_metadata("r3", vdb.Vector([3.0, 1.0]), vdb.Metadata({"color": "red"}), binary=vecs[3])   # upsert
    store.delete("r10")
    q = vecs[10]
    live = np.arange(40) != 10
    flt = vdb.MetadataFilter.Eq("color", "red")
    for f, eligible in ((None, live), (flt, live & (np.arange(40) % 2 == 1))):
        # internal ids follow the inserts: the upserted r3 has the largest; the reference orders by them
        internal = np.arange(40)
        internal[3] = 40
        (wi, wd), = D.search(D.HAMMING, internal, vecs, np.ones(40, bool), q[None, :], 5, eligible)
        got = store.search_binary(q, 5, f)
        assert [r.id for r in got] == [f"r{i if i < 40 else 3}" for i in wi] and [F32(r.distance) for r in got] == wd.tolist()
    assert got[0].id == "r3" and got[0].distance == 0.0
