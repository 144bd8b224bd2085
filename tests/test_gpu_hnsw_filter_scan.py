"""vdb_hnsw_set_filter_scan: a masked HNSW search whose mask leaves few present nodes is answered by an exact scan of those nodes
in the inner flat index (the brute-force route DESIGN.md 11 names); with the default setting, and above the limit, the walk
answers exactly as before."""
import numpy as np
import pytest

import oracle
from conftest import load_package
from hnsw_filter_restatement import mask_of

pytestmark = pytest.mark.gpu

N, D, M = 5000, 16, 8


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


@pytest.fixture(scope="module")
def graph(vdb):
    """5000 x 16, m = 8; then ids removed, and ids added again with other vectors: (index, current vectors, present, queries)"""
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(M, 64, 50), seed=3)
    g.build_batch((np.arange(N, dtype=np.uint64), rows))
    present = np.ones(N, dtype=bool)
    for i in range(5, N, 50):                                         # removed for good
        g.remove(i)
        present[i] = False
    for i in range(7, N, 250):                                        # removed and added again with a new vector
        g.remove(i)
        rows[i] = rng.standard_normal(D).astype(np.float32)
        g.add(i, vdb.Vector(rows[i]))
    for i in range(9, N, 500):                                        # replaced in place
        rows[i] = rng.standard_normal(D).astype(np.float32)
        g.add(i, vdb.Vector(rows[i]))
    return g, rows, present, rng.standard_normal((12, D)).astype(np.float32)


def same(a, b):
    (ai, ad, ac), (bi, bd, bc) = a, b
    if not np.array_equal(ac, bc):
        return False
    return all(np.array_equal(ai[q, :ac[q]], bi[q, :bc[q]]) and
               np.array_equal(ad[q, :ac[q]].view(np.uint32), bd[q, :bc[q]].view(np.uint32)) for q in range(ac.size))


def pick(rng, present, count):
    """a mask with `count` present ids -- plus removed ids and ids beyond the graph, which must never be returned"""
    elig = np.zeros(N + 64, dtype=bool)
    elig[rng.choice(np.nonzero(present)[0], size=count, replace=False)] = True
    elig[np.nonzero(~present)[0][:30]] = True
    elig[N:] = True
    return elig


def test_default_setting_is_the_walk(vdb, graph):
    g, rows, present, qs = graph
    rng = np.random.default_rng(1)
    elig = pick(rng, present, 40)
    mask, bits = mask_of(elig)
    g.set_filter_scan(0)
    dev = g.search_batch_arrays(qs, 10, 64, id_mask=mask, mask_bits=bits)
    g.set_traversal(True)
    host = g.search_batch_arrays(qs, 10, 64, id_mask=mask, mask_bits=bits)
    g.set_traversal(False)
    assert same(dev, host)
    assert all(present[int(i)] and elig[int(i)] for b in range(len(qs)) for i in dev[0][b, :dev[2][b]])


def test_selective_mask_is_scanned_exactly(vdb, graph):
    g, rows, present, qs = graph
    rng = np.random.default_rng(2)
    elig = pick(rng, present, 40)
    mask, bits = mask_of(elig)
    live = (present & elig[:N]).astype(np.uint8)
    assert int(live.sum()) == 40
    flat = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False)
    flat.add_bulk(rows[present], ids=np.nonzero(present)[0].astype(np.uint64))
    g.set_filter_scan(1000)
    try:
        for k in (1, 10, 40, 60):
            got = g.search_batch_arrays(qs, k, 64, id_mask=mask, mask_bits=bits)
            want = flat.search_batch_arrays(qs, k, id_mask=mask, mask_bits=bits)
            assert (got[2] == min(k, 40)).all()
            assert same(got, (want[0], want[1], want[2]))
            for b in (0, 5, 11):
                oi, od = oracle.flat_search(0, rows, qs[b], k, live=live)
                assert np.array_equal(got[0][b, :got[2][b]], oi)
                assert np.array_equal(got[1][b, :got[2][b]].view(np.uint32), od.view(np.uint32))
        # no mask: the walk, whatever the setting
        plain = g.search_batch_arrays(qs, 10, 64)
        g.set_filter_scan(0)
        assert same(plain, g.search_batch_arrays(qs, 10, 64))
    finally:
        g.set_filter_scan(0)


def test_above_the_limit_the_walk_still_answers(vdb, graph):
    g, rows, present, qs = graph
    rng = np.random.default_rng(3)
    elig = pick(rng, present, 2000)
    mask, bits = mask_of(elig)
    g.set_filter_scan(0)
    walk = g.search_batch_arrays(qs, 10, 64, id_mask=mask, mask_bits=bits)
    g.set_filter_scan(1000)
    try:
        before = g.stats()
        got = g.search_batch_arrays(qs, 10, 64, id_mask=mask, mask_bits=bits)
        after = g.stats()
    finally:
        g.set_filter_scan(0)
    assert same(got, walk)
    assert after["device_queries"] - before["device_queries"] + after["host_redone"] - before["host_redone"] == len(qs)
