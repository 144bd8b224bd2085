"""What the sparse-vector index rests on that needs no GPU: the numpy restatement against an f64 evaluation of the same sums, the
rank fusion on hand-written lists, and the argument refusals in front of the device."""
import ctypes

import numpy as np
import pytest

import spv_data as S


def test_restatement_against_f64():
    """Per score: |f32 fold - f64 sum| <= nnz * 2^-24 * sum |q_d * x_d|, the standard bound of a length-nnz f32 fold."""
    ids, X, P = S.corpus()
    rng = np.random.default_rng(1)
    for _ in range(5):
        idx = np.sort(rng.choice(480, size=40, replace=False))
        val = rng.standard_normal(40).astype(np.float32)
        touched, s = S.scores(X, P, (idx, val))
        prod = X[:, idx].astype(np.float64) * val.astype(np.float64) * P[:, idx]
        nnz = P[:, idx].sum(axis=1)
        assert np.array_equal(touched, nnz > 0) and touched.sum() > 4096
        assert np.all(np.abs(s - prod.sum(axis=1)) <= nnz * 2.0 ** -24 * np.abs(prod).sum(axis=1))
        got, d = S.search(ids, X, P, (idx[::-1], val[::-1]), 7)          # the order the pairs come in does not matter
        best = np.lexsort((ids[touched], S.ordered(-s[touched])))[:7]
        assert np.array_equal(got, ids[touched][best]) and np.array_equal(d, -s[touched][best])


def test_rank_fusion(vdb):
    fuse = vdb.sparse_index.rrf_fuse
    got = fuse([[5, 9, 2], [2, 7, 5]], 10)
    want = {5: 1 / 61 + 1 / 63, 2: 1 / 63 + 1 / 61, 9: 1 / 62, 7: 1 / 62}
    assert [i for i, _ in got] == [2, 5, 7, 9]           # equal sums: the smaller id first
    assert all(s == want[i] for i, s in got)
    assert fuse([[5, 9, 2], [2, 7, 5]], 1) == [(2, want[2])] and fuse([[], []], 3) == []


def test_refusals_in_front_of_the_device(vdb):
    L = vdb._ffi.lib()
    INVALID = vdb._ffi.ERR_INVALID_ARGUMENT
    out = (ctypes.c_uint64 * 8)()
    assert L.vdb_spv_create(0, None) == INVALID
    assert L.vdb_spv_add_bulk(None, None, None, None, None, 1) == INVALID
    assert L.vdb_spv_remove(None, 1) == INVALID and L.vdb_spv_flush(None) == INVALID and L.vdb_spv_len(None) == 0
    assert L.vdb_spv_search_batch(None, None, None, None, 1, None, 1, None, 0, 1, None, None, None) == INVALID
    assert L.vdb_spv_search_batch_filtered(None, None, None, None, 1, None, 1, None, 1, None, None, None) == INVALID
    assert L.vdb_spv_stats(None, out) == INVALID and L.vdb_spv_debug_set_workspace_cap(None, 0) == INVALID
    with pytest.raises(ValueError):
        vdb.sparse_index._csr([([1, 2], [1.0])])


# ------------------------------------------------------------------ the CSR reference against the dense one, bit for bit
def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _random_batch(rng, hi, nq):
    qs = []
    for _ in range(nq):
        idx = rng.choice(hi, size=rng.integers(1, 41), replace=False).astype(np.uint32)
        qs.append((idx, rng.standard_normal(idx.size).astype(np.float32)))
    return qs


def test_csr_reference_equals_the_dense_one_on_the_corpus():
    import test_gpu_spv as G
    ids, X, P = S.corpus()
    offsets, indices, values = S.csr_from_dense(X, P)
    view = S.csc_view(offsets, indices)
    rng = np.random.default_rng(77)
    live = rng.random(ids.size) < 0.9
    elig = rng.random(ids.size) < 0.5
    batches = [(qs, k) for qs, k in G.CASES.values()] + [(_random_batch(rng, 500, 3), int(rng.integers(1, 60))) for _ in range(20)]
    for qs, k in batches:
        for q in qs:
            ctr = {}
            assert _same(S.search_csr(ids, offsets, indices, values, np.ones(ids.size, bool), q, k, view=view, counters=ctr),
                         S.search(ids, X, P, q, k))
            assert ctr["entries_walked"] == sum(int(P[:, d].sum()) for d in q[0] if d < S.VOCAB)
            assert _same(S.search_csr(ids, offsets, indices, values, live, q, k, elig, view),      # a dead row is an ineligible one
                         S.search(ids, X, P, q, k, elig & live))


def test_edge_corpus_holds_what_it_names_and_both_references_agree():
    E = S.edge_corpus()
    ids, offsets, indices, values, row = E["ids"], E["offsets"], E["indices"], E["values"], E["row"]
    X, P = S.dense_of(offsets, indices, values, E["vocab"])
    live = np.ones(ids.size, bool)
    assert any((np.diff(indices[a:b].astype(np.int64)) < 0).any() for a, b in zip(offsets[:-1], offsets[1:]))   # given unsorted
    for name, q, want in E["finite"]:
        touched, s, _ = S.fold_csr(offsets, indices, values, live, q)
        for r, bits in want.items():
            assert touched[row[r]] and int(s[row[r]].view(np.uint32)) == bits, (name, r, hex(int(s[row[r]].view(np.uint32))))
        assert not np.isnan(s[touched]).any()
        assert _same(S.search_csr(ids, offsets, indices, values, live, q, 1024), S.search(ids, X, P, q, 1024))
    fold = dict((n, w) for n, _, w in E["finite"])["fold"]
    assert fold["cancel_a"] != fold["cancel_b"]                        # only the ascending order gives these bits
    assert 0 < fold["den_product"] < 0x00800000 and 0 < fold["den_mid"] - 0x00800000 < 0x00800000
    for name, q, bad in E["nan"]:
        touched, s, _ = S.fold_csr(offsets, indices, values, live, q)
        assert set(np.flatnonzero(touched & np.isnan(s)).tolist()) >= {row[r] for r in bad}, name
        for ref in (lambda e: S.search_csr(ids, offsets, indices, values, live, q, 10, e), lambda e: S.search(ids, X, P, q, 10, e)):
            with pytest.raises(S.NanScore):
                ref(None)
        ok = ~(touched & np.isnan(s))
        assert _same(S.search_csr(ids, offsets, indices, values, live, q, 10, ok), S.search(ids, X, P, q, 10, ok))
        assert _same(S.search_csr(ids, offsets, indices, values, ok, q, 10), S.search(ids, X, P, q, 10, ok))
    assert {0x7fffbeef, 0xffffbeef} <= {int(v) for v in values.view(np.uint32)}
