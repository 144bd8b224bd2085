"""The device-resident HNSW walk (kernels_hnsw.hip hnsw_search_kernel) AT its limits, not in the middle of its range: the two
implementations of the result-heap pop on both sides of WAVE_POP_MAX (search and insert mode), the ef / k / m bounds of the
routing between the device walk and the host traversal, walks that overflow their LDS structures inside a batch of walks that
do not (fail[q], the host re-run, the scatter back into the batch), and every chunk / tail shape of the staged distance fold.

Every comparison is against oracle.HnswOracle with the same seed and insertion order: ids, order and distance bits, graphs by
levels and neighbour lists.  The pre-filtered walk is compared with hnsw_filter_restatement.Walker on Gaussian rows (no ties).
tests/test_hnsw_limits_cpu.py proves on the CPU that the data sets here cross the caps they are meant to cross."""
import time

import numpy as np
import pytest

import hnsw_limits as hl
from conftest import load_package
from hnsw_filter_restatement import mask_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def build_gpu(vdb, metric, rows, m, efc, seed, frontier_only=None):
    g = vdb.GpuHnswIndex(vdb.DistanceMetric(metric), vdb.HnswParams.new(m, efc, 50), seed=seed)
    if frontier_only is not None:
        g.set_build(frontier_only)
    g.build_batch((np.arange(rows.shape[0], dtype=np.uint64), rows))
    return g


def check_search(g, o, queries, k, ef, device, expected=None):
    """the routed search against the oracle, then once more through the forced host traversal: device == host"""
    expected = hl.oracle_results(o, queries, k, ef) if expected is None else expected
    got = hl.routed_search(g, queries, k, ef, device)
    hl.assert_rows_equal(got, expected, (k, ef))
    g.set_traversal(host_only=True)
    try:
        host = hl.routed_search(g, queries, k, ef, device=False)
    finally:
        g.set_traversal(host_only=False)
    assert hl.same_arrays(got, host), (k, ef)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. ef and k edges of the result heap
# ---------------------------------------------------------------------------------------------------------------------------
_ef_graphs = {}


@pytest.fixture
def ef_graph(vdb):
    def get(metric, kind):
        if (metric, kind) not in _ef_graphs:
            s = hl.EF_SHAPE
            rows, queries, seed = hl.ef_data(metric, kind)
            g = build_gpu(vdb, metric, rows, s["m"], s["efc"], seed)
            o = hl.build_oracle(metric, rows, s["m"], s["efc"], seed)
            hl.assert_same_graph(g, o, range(0, s["n"], 3))
            _ef_graphs[(metric, kind)] = (g, o, queries)
        return _ef_graphs[(metric, kind)]
    return get


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("ef", hl.EF_VALUES)
def test_ef_across_the_wave_pop_and_routing_boundaries(ef_graph, metric, ef):
    g, o, queries = ef_graph(metric, "gauss")
    expected = hl.oracle_results(o, queries, 10, ef)
    # more than ef nodes are reachable: the result heap really fills to ef + 1 before every pop (a full answer of k = ef proves it)
    full, _ = o.search(queries[0], ef, ef)
    assert len(full) == ef
    check_search(g, o, queries, 10, ef, device=ef <= hl.DEVICE_EF_MAX, expected=expected)


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("k,ef", hl.LARGE_K)
def test_k_larger_than_ef_sizes_the_result_heap(ef_graph, metric, k, ef):
    g, o, queries = ef_graph(metric, "gauss")
    expected = hl.oracle_results(o, queries, k, ef)
    assert all(len(i) == k for i, _ in expected)                       # ef_actual = max(ef, k): k results come back
    check_search(g, o, queries, k, ef, device=max(ef, k) <= hl.DEVICE_EF_MAX, expected=expected)


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("ef", hl.TIE_EF_VALUES)
def test_ef_boundaries_with_exact_ties(ef_graph, metric, ef):
    """Rows drawn from n / 8 base rows: the order of equal distances is the heap's backing array, which both pops must leave as
    Rust's BinaryHeap does.  Against the C oracle only (the Python restatement's heapq orders ties differently)."""
    g, o, queries = ef_graph(metric, "dups")
    expected = hl.oracle_results(o, queries, 10, ef)
    tied, td = o.search(queries[0], ef, ef)
    assert len(tied) == ef and np.unique(td).size < ef                 # ties inside the heap, not only in the data
    check_search(g, o, queries, 10, ef, device=True, expected=expected)
    check_search(g, o, queries, ef, ef, device=True)                   # the whole heap comes back: every tie's place is compared


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ef_construction across the same boundary: the walk in insert mode
# ---------------------------------------------------------------------------------------------------------------------------
_efc_oracles = {}


@pytest.mark.parametrize("frontier_only", [True, False])
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("efc", hl.EFC_VALUES)
def test_ef_construction_across_the_wave_pop_boundary(vdb, efc, metric, frontier_only):
    s = hl.EFC_SHAPE
    rows = hl.gauss(700 + metric, s["n"], s["d"])
    queries = hl.gauss(800 + metric, s["nq"], s["d"])
    seed = 41 + metric
    if (metric, efc) not in _efc_oracles:
        _efc_oracles[(metric, efc)] = hl.build_oracle(metric, rows, s["m"], efc, seed)
    o = _efc_oracles[(metric, efc)]
    g = build_gpu(vdb, metric, rows, s["m"], efc, seed, frontier_only=frontier_only)
    bs = g.build_stats()
    assert bs["record_overflows"] == 0, bs
    if frontier_only:                                                  # the device walks did the work
        assert bs["frontier_inserts"] == s["n"] and bs["scan_inserts"] == 0 and bs["walk_distances"] > 0, bs
    else:
        assert bs["scan_inserts"] == s["n"] and bs["frontier_inserts"] == 0, bs
    hl.assert_same_graph(g, o, range(s["n"]))
    check_search(g, o, queries, 10, 64, device=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. walks that overflow, in a mixed batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overflow(vdb):
    c = hl.OVERFLOW
    rows, plain_q, elig, filt_q = hl.overflow_data()
    t0 = time.time()
    o = hl.build_oracle(c["metric"], rows, c["m"], c["efc"], c["graph_seed"])
    t1 = time.time()
    g = build_gpu(vdb, c["metric"], rows, c["m"], c["efc"], c["graph_seed"])
    t2 = time.time()
    hl.assert_same_graph(g, o, range(0, c["n"], 16))
    print(f"overflow graph: oracle build {t1 - t0:.1f} s, GPU build {t2 - t1:.1f} s, {g.build_stats()}")
    small_q = hl.gauss(c["seed"] + 1, 8, c["d"])
    return dict(g=g, o=o, rows=rows, plain_q=plain_q, elig=elig, filt_q=filt_q, small_q=small_q)


def assert_clean_state(f):
    """a failed walk leaves nothing behind (fail flags, visited bitmaps): the next small search is device-resident and exact"""
    got = hl.routed_search(f["g"], f["small_q"], 10, 64, device=True)
    hl.assert_rows_equal(got, hl.oracle_results(f["o"], f["small_q"], 10, 64), "after an overflow batch")


def run_mixed(g, queries, k, ef, fails, expected, **kw):
    before = g.stats()
    got = g.search_batch_arrays(queries, k, ef, **kw)
    after = g.stats()
    redone, on_device = after["host_redone"] - before["host_redone"], after["device_queries"] - before["device_queries"]
    print(f"host_redone {redone} (predicted {int(np.sum(fails))}), device_queries {on_device}, of {len(queries)}")
    assert redone == int(np.sum(fails)), (redone, fails)
    assert redone + on_device == len(queries)
    hl.assert_rows_equal(got, expected, "mixed batch")
    return got


def test_plain_walks_that_overflow_the_visited_set_in_a_mixed_batch(overflow):
    f, c, p = overflow, hl.OVERFLOW, hl.OVERFLOW_PLAIN
    g, o, q = f["g"], f["o"], f["plain_q"]
    _, ctr = hl.walk_counters(o, c["metric"], f["rows"], q, p["k"], p["ef"])
    fails = np.array([hl.overflows(x, filtered=False) for x in ctr])
    print("layer-0 visited:", [x["layer_visited"][-1] for x in ctr], "pushed:", [x["pushed"] for x in ctr])
    assert 3 <= fails.sum() <= len(q) - 3
    expected = hl.oracle_results(o, q, p["k"], p["ef"])
    run_mixed(g, q, p["k"], p["ef"], fails, expected)
    assert_clean_state(f)
    # failing and passing walks interleaved: the host's results are scattered back by their place in the batch
    bad, good = np.flatnonzero(fails), np.flatnonzero(~fails)
    pairs = min(len(bad), len(good))
    order = np.array([i for pair in zip(bad[:pairs], good[:pairs]) for i in pair] + list(bad[pairs:]) + list(good[pairs:]))
    assert sorted(order) == list(range(len(q))) and not np.array_equal(order, np.arange(len(q)))
    run_mixed(g, q[order], p["k"], p["ef"], fails[order], [expected[i] for i in order])
    assert_clean_state(f)


def test_filtered_walks_that_overflow_the_candidate_heap_in_a_mixed_batch(overflow):
    f, c, p = overflow, hl.OVERFLOW, hl.OVERFLOW_FILTERED
    g, o, q, elig = f["g"], f["o"], f["filt_q"], f["elig"]
    res, ctr = hl.walk_counters(o, c["metric"], f["rows"], q, p["k"], p["ef"], elig)
    fails = np.array([hl.overflows(x, filtered=True) for x in ctr])
    print("pushed:", [x["pushed"] for x in ctr])
    assert 3 <= fails.sum() <= len(q) - 3
    mask, bits = mask_of(elig)
    dev = run_mixed(g, q, p["k"], p["ef"], fails, res, id_mask=mask, mask_bits=bits)         # device (+ host re-runs) == Walker
    assert all(elig[int(i)] for b in range(len(q)) for i in dev[0][b, :dev[2][b]])
    g.set_traversal(host_only=True)
    try:
        host = hl.routed_search(g, q, p["k"], p["ef"], device=False, id_mask=mask, mask_bits=bits)
    finally:
        g.set_traversal(host_only=False)
    assert hl.same_arrays(dev, host)
    assert_clean_state(f)
    # and a filtered batch right after it whose walks all fit: nothing of the failed walks' bitmaps is left
    near = q[~fails]
    run_mixed(g, near, p["k"], p["ef"], np.zeros(len(near), bool), [r for r, x in zip(res, fails) if not x], id_mask=mask, mask_bits=bits)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the m boundary (MAXP = 40 neighbours per expansion: m_max0 + 1 = 2 m + 1)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [18, 19, 20])
def test_m_boundary_of_the_device_walk(vdb, m):
    n, d = 600, 24
    rows, queries = hl.gauss(900 + m, n, d), hl.gauss(950 + m, 8, d)
    o = hl.build_oracle(0, rows, m, 64, seed=m)
    g = build_gpu(vdb, 0, rows, m, 64, seed=m)
    hl.assert_same_graph(g, o, range(n))
    bs = g.build_stats()
    assert (bs["frontier_inserts"], bs["scan_inserts"]) == ((n, 0) if m <= hl.DEVICE_M_MAX else (0, n)), bs
    assert max(len(o.neighbors(i, 0)) for i in range(n)) == 2 * m      # full lists: the expansion really has 2 m neighbours
    check_search(g, o, queries, 10, 100, device=m <= hl.DEVICE_M_MAX)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. dimension and chunk edges of the staged distance fold
# ---------------------------------------------------------------------------------------------------------------------------
DIMS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 385, 513, 769)
DIM_CASES = [(m, dim, metric) for m in (2, 19) for dim in DIMS for metric in ((0, 1, 2) if dim <= 257 else (0, 1))]


@pytest.mark.parametrize("m,dim,metric", DIM_CASES)
def test_dimension_and_chunk_edges_of_the_staged_fold(vdb, m, dim, metric):
    n = 300
    rows, queries = hl.gauss(1000 + dim, n, dim), hl.gauss(2000 + dim, 6, dim)
    o = hl.build_oracle(metric, rows, m, 32, seed=dim + m)
    g = build_gpu(vdb, metric, rows, m, 32, seed=dim + m)
    assert g.build_stats()["frontier_inserts"] == n                    # the fold ran in insert mode too
    hl.assert_same_graph(g, o, range(n))
    got = hl.routed_search(g, queries, 10, 48, device=True)
    hl.assert_rows_equal(got, hl.oracle_results(o, queries, 10, 48), (m, dim, metric))


@pytest.mark.parametrize("metric", [0, 1])
def test_a_dimension_too_large_for_the_lds_plan_is_host_routed(vdb, metric):
    """4 * dim bytes of query beside the walk's 106 KB of heaps and visited set leave no room for the staging buffers: searches
    take the host traversal, and a frontier-only build silently takes the row-scan path."""
    n, dim, m = 64, 14000, 8
    rows, queries = hl.gauss(3000 + metric, n, dim), hl.gauss(3100 + metric, 4, dim)
    o = hl.build_oracle(metric, rows, m, 32, seed=6)
    g = build_gpu(vdb, metric, rows, m, 32, seed=6, frontier_only=True)
    bs = g.build_stats()
    assert bs["scan_inserts"] == n and bs["frontier_inserts"] == 0 and bs["walk_distances"] == 0, bs
    hl.assert_same_graph(g, o, range(n))
    got = hl.routed_search(g, queries, 10, 48, device=False)
    hl.assert_rows_equal(got, hl.oracle_results(o, queries, 10, 48), dim)
