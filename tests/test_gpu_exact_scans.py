"""The exact scans that share one multi-query row fold (csrc/kernels_exact.h fold_multi) and one host driver: the kNN fallback
and the exact range scan (bounded_scan_kernel, eight queries per pass over the rows) and the row scan of the HNSW build
(scan_rows_kernel<4|8|16>).  The shapes sit where the fold and the driver can go wrong -- a dimension that is only a tail, only
a 16-float block, a block plus a tail; a last group of one query; fewer queries than an instantiation holds -- and every
comparison is bit for bit against the CPU oracle: ids, order, distance bits, counts and totals."""
import numpy as np
import pytest

import oracle
import range_data as rd
from conftest import load_package
from test_gpu_hnsw import assert_same_graph
from test_gpu_range import ROUTE0, ROUTE1, ROUTE2, check as check_range

pytestmark = pytest.mark.gpu

F32 = np.float32
METRICS = (rd.EUCLID, rd.COSINE, rd.DOT)
N, NQ, K = 20000, 17, 10                                           # above the 16384-row direct path; query groups of 8, 8 and 1
DIMS = (1, 15, 16, 17, 40)                                         # tail only; block only (15: tail only, one short of it); block + tail(s)
N_DEAD = 2000
MAX_RESULTS = 64

_CASES = {}


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def _bits(on):
    m = np.packbits(on.astype(np.uint8), bitorder="little")
    return np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64), len(on)


def case(vdb, metric, dim):
    """One index per (metric, dim), shared by the kNN and the range test: permuted ids (the idrank / rank2row path), N_DEAD rows
    removed, an id mask that leaves about two thirds of the ids eligible.  `live` is what the oracle sees: alive and eligible."""
    key = (metric, dim)
    if key not in _CASES:
        rng = np.random.default_rng(4100 + 10 * dim + metric)
        rows = rng.standard_normal((N, dim)).astype(F32)
        ids = rng.permutation(N).astype(np.uint64)
        q = (rows[rng.integers(0, N, NQ)] + F32(0.05) * rng.standard_normal((NQ, dim)).astype(F32)).astype(F32)
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
        ix.add_bulk(rows, ids=ids)
        dead = rng.choice(N, N_DEAD, replace=False)
        for r in dead:
            ix.remove(int(ids[r]))
        on = rng.random(N) < 0.67                                  # by id
        live = on[ids.astype(np.int64)]
        live[dead] = False
        for a in (rows, ids, q):
            a.setflags(write=False)
        _CASES[key] = dict(ix=ix, rows=rows, ids=ids, q=np.ascontiguousarray(q), live=live.astype(np.uint8), mask=_bits(on))
    return _CASES[key]


# ------------------------------------------------------------------ 1. the kNN fallback
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_fold_edges_knn_fallback(vdb, metric, dim):
    c = case(vdb, metric, dim)
    ix = c["ix"]
    ix.set_tiers(ix.TIERS_FORCE_EXACT)
    try:
        gi, gd, gc = ix.search_batch_arrays(c["q"], K, id_mask=c["mask"][0], mask_bits=c["mask"][1])
        st = ix.last_stats()
    finally:
        ix.set_tiers(0)
    assert st["exact_queries"] == NQ, st
    for b in range(NQ):                                            # (the comparison of test_gpu_parity.check_against_oracle)
        oi, od = oracle.flat_search(metric, c["rows"], c["q"][b], K, ids=c["ids"], live=c["live"])
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), (b, gi[b, :gc[b]], oi, gd[b, :gc[b]], od)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc[b]], od)


# ------------------------------------------------------------------ 2. the exact range scan
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_fold_edges_range_scan(vdb, metric, dim):
    c = case(vdb, metric, dim)
    ix = c["ix"]
    key = ("exact_scans", dim)
    # radii at the exact distance of a stored neighbour (a tie with the radius is in); from the 200th neighbour on the total
    # exceeds max_results; query 5 gets a negative radius
    at = (1, 7, MAX_RESULTS, 200, 1500)
    radii = np.array([rd.radius_at(rd.ranking((key, b), metric, c["rows"], c["q"][b], ids=c["ids"], live=c["live"]), at[b % len(at)])
                      for b in range(NQ)], dtype=F32)
    radii[5] = F32(-0.5)
    ix.set_screen(0)
    try:
        (gi, gd, gc, gt), st = check_range(ix, key, metric, c["rows"], c["q"], radii, MAX_RESULTS, ids=c["ids"], live=c["live"], mask=c["mask"])
    finally:
        ix.set_screen(1)
    assert (st[ROUTE0], st[ROUTE1], st[ROUTE2], st[3]) == (0, NQ, 0, 0), st          # every query on the scan, no filter pass
    assert (gt > gc).any() and (gt[[b for b in range(NQ) if at[b % len(at)] == 1 and b != 5]] >= 1).all(), (gc, gt)
    if metric != rd.DOT:
        assert int(gt[5]) == 0 and int(gc[5]) == 0


# ------------------------------------------------------------------ 3. the kNN bound's tie rule and the dense hand-over
@pytest.mark.parametrize("metric", (rd.EUCLID, rd.DOT))
def test_every_row_ties_with_the_bound(vdb, metric):
    """40000 identical rows: every row ties with the k-th distance the tiers found, so all of them survive the bounded pass
    (!(dist > bound)).  That is more than the 32768 keys a query's buffer holds, from which it follows that the per-query exact
    scan (exact_one) answers -- an inference from 40000 > 32768: no kNN statistic exposes the hand-over, the test checks the
    answer (the ten smallest ids at one distance, bit for bit) and exact_queries, not the route."""
    n, dim = 40000, 4
    rows = np.tile(np.array([0.5, -1.25, 2.0, 0.75], dtype=F32), (n, 1))
    ids = np.random.default_rng(7).permutation(n).astype(np.uint64)
    q = np.array([[0.25, 1.0, -0.5, 3.0], [0.5, -1.25, 2.0, 0.75]], dtype=F32)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
    ix.add_bulk(rows, ids=ids)
    ix.set_tiers(ix.TIERS_FORCE_EXACT)
    gi, gd, gc = ix.search_batch_arrays(q, K)
    assert ix.last_stats()["exact_queries"] == len(q)
    for b in range(len(q)):
        oi, od = oracle.flat_search(metric, rows, q[b], K, ids=ids)
        assert gc[b] == K and list(oi) == list(range(K)) and len(set(od.view(np.uint32))) == 1
        assert np.array_equal(gi[b, :K], oi), (b, gi[b, :K])
        assert np.array_equal(gd[b, :K].view(np.uint32), od.view(np.uint32)), (b, gd[b, :K], od)


# ------------------------------------------------------------------ 4. the row scan of the HNSW build
BATCHES = (1, 4, 5, 9, 16, 17)                                     # launches of 1, 4 | 5 | 9, 16, 16 + 1 query rows: scan_rows_kernel<4>, <8>, <16>


@pytest.mark.parametrize("dim", (5, 16, 24))
@pytest.mark.parametrize("metric", METRICS)
def test_hnsw_row_scan_build(vdb, metric, dim):
    n, m, efc = 300, 6, 40
    rng = np.random.default_rng(500 + 10 * dim + metric)
    rows = rng.standard_normal((n, dim)).astype(F32)
    zero_at = 150 if metric == rd.COSINE else None                 # a zero vector inside a batch of 17 (below)
    if zero_at is not None:
        rows[zero_at] = 0.0
    g = vdb.GpuHnswIndex(vdb.DistanceMetric(metric), vdb.HnswParams.new(m, efc, 30), seed=21 + metric)
    o = oracle.HnswOracle(metric, m=m, ef_construction=efc, ef_search=30, seed=21 + metric)
    g.set_build(False)
    ids = np.arange(n, dtype=np.uint64)
    i, t, present, sizes = 0, 0, [], set()
    while i < n:
        b = min(BATCHES[t % len(BATCHES)], n - i)
        t += 1
        if zero_at is not None and i <= zero_at < i + b:
            # mod.rs:37-42: the build stops at the failing insert; that node is stored without links, later vectors are not
            assert b == 17 and i < zero_at < i + b - 1
            with pytest.raises(vdb.InvalidVector):
                g.build_batch((ids[i:i + b], rows[i:i + b]))
            for j in range(i, zero_at):
                o.insert(j, rows[j])
            with pytest.raises(Exception):
                o.insert(zero_at, rows[zero_at])
            assert g.len() == len(o) == zero_at + 1
            present += list(range(i, zero_at))
            assert_same_graph(g, o, np.array(present, dtype=np.uint64))
            g.remove(zero_at); o.remove(zero_at)
            i = zero_at + 1
            continue
        g.build_batch((ids[i:i + b], rows[i:i + b]))
        for j in range(i, i + b):
            o.insert(j, rows[j])
        present += list(range(i, i + b))
        sizes.add(b)
        i += b
    assert sizes >= set(BATCHES)
    bs = g.build_stats()
    assert bs["frontier_inserts"] == 0 and bs["scan_inserts"] >= len(present), bs
    assert_same_graph(g, o, np.array(present, dtype=np.uint64))
    queries = rng.standard_normal((8, dim)).astype(F32)
    gi, gd, gc = g.search_batch_arrays(queries, 10, 40)
    for b in range(len(queries)):
        oi, od = o.search(queries[b], 10, 40)
        assert gc[b] == len(oi) and np.array_equal(gi[b, :gc[b]], oi), b
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), b
