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
