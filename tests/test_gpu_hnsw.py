"""The GPU-offloaded HNSW index (include/vdb_hnsw.h, BASELINE config 5) against the CPU restatement of the
reference's HNSW (oracle/hnsw_oracle.c).  With the same seed and insertion order the two must hold the SAME graph
(entry point, node levels, every neighbour list in order) and return the SAME results (ids, order, distance bits):
the product runs the reference's traversal and only moves the distance evaluations to the GPU.  Against the
reference itself parity is statistical (its levels are unseeded): the recall floors of tests/recall_test.rs."""
import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def build_pair(vdb, metric, rows, m, efc, efs, seed, bulk=True, ids=None):
    g = vdb.GpuHnswIndex(vdb.DistanceMetric(metric), vdb.HnswParams.new(m, efc, efs), seed=seed)
    o = oracle.HnswOracle(metric, m=m, ef_construction=efc, ef_search=efs, seed=seed)
    ids = np.arange(rows.shape[0], dtype=np.uint64) if ids is None else np.asarray(ids, dtype=np.uint64)
    if bulk:
        g.build_batch((ids, rows))
    else:
        for i, v in zip(ids, rows):
            g.add(int(i), vdb.Vector(v))
    for i, v in zip(ids, rows):
        o.insert(int(i), v)
    return g, o, ids


def assert_same_graph(g, o, ids):
    assert g.len() == len(o)
    assert g.entry_point() == o.entry_point()
    for i in ids:
        lv = o.level(int(i))
        assert g.level(int(i)) == lv, i
        if lv < 0:
            continue
        for l in range(lv + 1):
            assert g.neighbors(int(i), l) == o.neighbors(int(i), l), (int(i), l)
        assert g.neighbors(int(i), lv + 1) is None


def assert_same_results(g, o, queries, k, ef):
    gi, gd, gc = g.search_batch_arrays(queries, k, ef)
    for b in range(queries.shape[0]):
        oi, od = o.search(queries[b], k, ef)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), (b, gi[b, :gc[b]], oi)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc[b]], od)


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("n,d,m,efc", [(300, 8, 4, 32), (1500, 48, 16, 200), (800, 100, 8, 64)])
def test_graph_and_results_equal_the_cpu_restatement(vdb, metric, n, d, m, efc):
    rng = np.random.default_rng(n + d + metric)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((37, d)).astype(np.float32)
    g, o, ids = build_pair(vdb, metric, rows, m, efc, 50, seed=7 + metric)
    assert_same_graph(g, o, ids)
    assert_same_results(g, o, queries, 10, 100)
    assert_same_results(g, o, queries[:5], 1, 16)
    assert_same_results(g, o, queries[:5], 200, 50)                     # k > ef: ef_actual = k (graph.rs:406)
    # the result heap at the edge of what a wave pops with four ballots (514 entries) and beyond it (single-lane pop between wave pushes)
    assert_same_results(g, o, queries[:4], 10, 513)
    assert_same_results(g, o, queries[:4], 10, 700)
    st = g.stats()
    assert st["gpu_distances"] > 0 and st["device_queries"] == 37 + 5 + 5 + 4 + 4 and st["host_redone"] == 0, st


def test_device_resident_and_host_traversal_agree(vdb):
    """The same batch through the device-resident search (default) and the host traversal: both are the reference's walk."""
    import os
    import subprocess
    import sys
    rng = np.random.default_rng(12)
    rows = rng.random((3000, 40), dtype=np.float32)
    q = rng.random((64, 40), dtype=np.float32)
    g, o, ids = build_pair(vdb, 0, rows, 16, 100, 50, seed=2)
    gi, gd, gc = g.search_batch_arrays(q, 10, 200)
    assert g.stats()["device_queries"] == 64
    # m = 24 (lists of up to 49 neighbours) does not fit the device kernel: host traversal, same answers as the oracle
    g2, o2, _ = build_pair(vdb, 0, rows, 24, 100, 50, seed=2)
    assert_same_results(g2, o2, q[:9], 10, 64)
    assert g2.stats()["device_queries"] == 0 and g2.stats()["last_search_rounds"] > 0
    # the host traversal forced for the same batch (vdb_hnsw_set_traversal): identical results
    g.set_traversal(host_only=True, host_threads=3)
    hi, hd, hc = g.search_batch_arrays(q, 10, 200)
    assert g.stats()["device_queries"] == 64 and g.stats()["last_search_rounds"] > 0
    assert np.array_equal(hi, gi) and np.array_equal(hd.view(np.uint32), gd.view(np.uint32)) and np.array_equal(hc, gc)
    g.set_traversal(host_only=False)


def test_single_adds_equal_bulk_build(vdb):
    rng = np.random.default_rng(5)
    rows = rng.random((400, 12), dtype=np.float32)
    a, o, ids = build_pair(vdb, 0, rows, 8, 64, 50, seed=3, bulk=False)
    b, _, _ = build_pair(vdb, 0, rows, 8, 64, 50, seed=3, bulk=True)
    assert_same_graph(a, o, ids)
    assert_same_graph(b, o, ids)


def test_duplicate_rows_tie_order_follows_the_heap_layout(vdb):
    """Equal distances: into_sorted_vec keeps the BinaryHeap's array order among ties (neighbor_queue.rs:102-106);
    the product and the restatement must agree on it."""
    rng = np.random.default_rng(6)
    base = rng.random((60, 6), dtype=np.float32)
    rows = np.concatenate([base] * 5, 0)                                   # every vector 5 times
    g, o, ids = build_pair(vdb, 0, rows, 6, 40, 50, seed=9)
    assert_same_graph(g, o, ids)
    assert_same_results(g, o, base[:20], 12, 64)


def test_remove_semantics(vdb):
    rng = np.random.default_rng(8)
    rows = rng.random((500, 10), dtype=np.float32)
    g, o, ids = build_pair(vdb, 0, rows, 8, 64, 50, seed=4)
    ep, _ = o.entry_point()
    for victim in [3, 77, 78, ep, 499, 12345]:                             # incl. the entry point and an absent id
        g.remove(victim)
        o.remove(victim)
    assert_same_graph(g, o, ids)
    q = rng.random((9, 10), dtype=np.float32)
    assert_same_results(g, o, q, 10, 50)
    # inserts after deletions keep following the same random stream
    extra = rng.random((40, 10), dtype=np.float32)
    for j, v in enumerate(extra):
        g.add(1000 + j, vdb.Vector(v))
        o.insert(1000 + j, v)
    assert_same_graph(g, o, list(ids) + list(range(1000, 1040)))
    assert_same_results(g, o, q, 10, 50)


def test_reference_unit_tests_through_the_trait(vdb):
    V, M = vdb.Vector, vdb.DistanceMetric
    ix = vdb.GpuHnswIndex(M.Euclidean)                                     # mod.rs:88-98
    ix.add(0, V([1.0, 0.0, 0.0])); ix.add(1, V([0.0, 1.0, 0.0])); ix.add(2, V([1.0, 1.0, 0.0]))
    res = ix.search(V([1.0, 0.0, 0.0]), 2)
    assert len(res) == 2 and res[0][0] == 0 and res[0][1] < 1e-5
    assert ix.get_vector(0) == V([1.0, 0.0, 0.0]) and ix.get_vector(99) is None       # mod.rs:101-108
    g = vdb.GpuHnswIndex(M.Euclidean, vdb.HnswParams.new(4, 32, 16))       # graph.rs:488-504
    for i in range(5):
        g.add(i, V([float(i), 0.0]))
    r = g.search_with_ef(V([0.5, 0.0]), 2, 16)
    assert len(r) == 2 and {r[0][0], r[1][0]} == {0, 1}
    g = vdb.GpuHnswIndex(M.Euclidean, vdb.HnswParams.new(4, 32, 16))       # graph.rs:507-537
    g.add(0, V([1.0, 0.0])); g.add(1, V([0.0, 1.0])); g.add(2, V([1.0, 1.0]))
    ep, _ = g.entry_point()
    g.remove(ep)
    assert g.len() == 2 and len(g.search_with_ef(V([0.0, 1.0]), 1, 16)) == 1
    assert vdb.GpuHnswIndex(M.Cosine).search(V([1.0, 2.0]), 3) == []       # empty graph (graph.rs:392-395)


def test_hnsw_behind_the_vector_store(vdb):
    # mod.rs:111-133 / :136-153: VectorStore::with_index(HnswIndex)
    V = vdb.Vector
    store = vdb.VectorStore.with_index(vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(4, 32, 16)))
    store.insert("v1", V([1.0, 0.0, 0.0])); store.insert("v2", V([0.0, 1.0, 0.0])); store.insert("v3", V([0.0, 0.0, 1.0]))
    res = store.search(V([1.0, 0.1, 0.0]), 2)
    assert len(res) == 2 and res[0].id == "v1"
    store.delete("v1")
    assert len(store) == 2


def test_error_semantics(vdb):
    V = vdb.Vector
    ix = vdb.GpuHnswIndex(vdb.DistanceMetric.Cosine, vdb.HnswParams.new(4, 32, 16))
    ix.add(0, V([1.0, 0.0])); ix.add(1, V([0.0, 1.0]))
    with pytest.raises(vdb.InvalidVector):                                 # zero-norm query (distance.rs:51-55)
        ix.search(V([0.0, 0.0]), 1)
    with pytest.raises(vdb.DimensionMismatch):
        ix.search(V([1.0, 0.0, 0.0]), 1)
    with pytest.raises(vdb.DimensionMismatch):
        ix.add(2, V([1.0, 0.0, 0.0]))


@pytest.mark.parametrize("n,dim,nq,floor", [(100, 32, 50, 0.90), (1000, 64, 50, 0.90), (5000, 128, 20, 0.85)])
def test_recall_floors_of_the_reference(vdb, n, dim, nq, floor):
    # tests/recall_test.rs:28-80 with the GPU FlatIndex as ground truth
    rng = np.random.default_rng(n)
    rows = rng.random((n, dim), dtype=np.float32)
    queries = rng.random((nq, dim), dtype=np.float32)
    flat = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False)
    flat.add_bulk(rows)
    hnsw = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(16, 200, 50), seed=n)
    hnsw.build_batch((np.arange(n, dtype=np.uint64), rows))
    ti, _, _ = flat.search_batch_arrays(queries, 10)
    hi, hd, hc = hnsw.search_batch_arrays(queries, 10, 100)
    rec = np.mean([len(set(ti[b]) & set(hi[b, :hc[b]])) / 10.0 for b in range(nq)])
    assert rec >= floor, rec
    assert np.all(hd[:, 1:] >= hd[:, :-1])


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_frontier_only_build_equals_the_scan_build_and_the_cpu_restatement(vdb, metric):
    """bulk inserts used to fold every new vector against every stored row (N^2 / 2 distances).  The default
    build now runs a device walk per insert that evaluates only what search_layer asks for (graph.rs:155, :182) on the graph as
    of a block of 64 inserts earlier (the walks run one block ahead of the host), and the host replays the inserts in order -- the SAME graph, node for node, as the
    row-scan build and as the CPU restatement; the GPU evaluates a small multiple of the distances the reference's algorithm
    consumes, not N^2 / 2."""
    rng = np.random.default_rng(90 + metric)
    n, d, m, efc = 6000, 64, 12, 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[3000:3040] = rows[100:140]                                    # duplicates: exact ties inside the walks
    g, o, ids = build_pair(vdb, metric, rows, m, efc, 50, seed=11 + metric)          # default: frontier only
    assert_same_graph(g, o, ids)
    bs = g.build_stats()
    assert bs["frontier_inserts"] == n and bs["scan_inserts"] == 0, bs
    gpu = bs["walk_distances"] + bs["in_chunk_distances"] + bs["miss_distances"]
    assert bs["reference_distances"] > 0 and gpu <= 3 * bs["reference_distances"], bs     # within 3x of what the algorithm evaluates
    assert gpu < n * (n - 1) // 2, bs                                                   # (the row scans' count; at 6000 nodes a walk still sees a sixth of the graph)
    assert bs["record_overflows"] == 0, bs
    bt = g.build_times()                                               # vdb_hnsw_build_times: where the build's wall time went
    assert bt["replay_s"] > 0 and bt["replay_s"] >= bt["replay_miss_round_trips_s"] >= 0 and bt["walks_s"] >= 0 and bt["mirror_sync_s"] >= 0, bt
    g2 = vdb.GpuHnswIndex(vdb.DistanceMetric(metric), vdb.HnswParams.new(m, efc, 50), seed=11 + metric)
    g2.set_build(False)                                                # the row-scan build of round 2
    g2.build_batch((ids, rows))
    assert g2.build_stats()["scan_inserts"] == n
    assert g2.entry_point() == g.entry_point()
    for i in range(0, n, 7):
        lv = g.level(i)
        assert g2.level(i) == lv
        for l in range(lv + 1):
            assert g2.neighbors(i, l) == g.neighbors(i, l), (i, l)
    queries = rng.standard_normal((20, d)).astype(np.float32)
    assert_same_results(g, o, queries, 10, 100)
    # a second bulk on top of the first (the mirror grows incrementally), single adds in between, a removal (full rebuild)
    more = rng.standard_normal((700, d)).astype(np.float32)
    g.build_batch((np.arange(n, n + 700, dtype=np.uint64), more))
    for i, v in enumerate(more):
        o.insert(n + i, v)
    g.add(n + 700, vdb.Vector(rows[5])); o.insert(n + 700, rows[5])
    g.remove(17); o.remove(17)
    extra = rng.standard_normal((64, d)).astype(np.float32)
    g.build_batch((np.arange(n + 701, n + 765, dtype=np.uint64), extra))
    for i, v in enumerate(extra):
        o.insert(n + 701 + i, v)
    all_ids = np.arange(n + 765, dtype=np.uint64)
    assert_same_graph(g, o, all_ids)
    assert_same_results(g, o, queries, 10, 100)


def test_frontier_only_build_reports_a_zero_norm_row_like_the_reference(vdb):
    """mod.rs:37-42: build_batch returns at the first failing insert; that node is stored without links, later vectors are not."""
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((200, 16)).astype(np.float32)
    rows[120] = 0.0
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Cosine, vdb.HnswParams.new(8, 40, 20), seed=3)
    o = oracle.HnswOracle(1, m=8, ef_construction=40, ef_search=20, seed=3)
    with pytest.raises(vdb.InvalidVector):
        g.build_batch((np.arange(200, dtype=np.uint64), rows))
    failed = False
    for i, v in enumerate(rows):
        try:
            o.insert(i, v)
        except Exception:
            failed = True
            break
    assert failed and g.len() == len(o) == 121
    assert_same_graph(g, o, np.arange(120, dtype=np.uint64))
    # the level generator is where the reference's would be: the next inserts draw the same levels
    g.remove(120); o.remove(120)
    nxt = rng.standard_normal((40, 16)).astype(np.float32)
    g.build_batch((np.arange(300, 340, dtype=np.uint64), nxt))
    for i, v in enumerate(nxt):
        o.insert(300 + i, v)
    assert_same_graph(g, o, np.concatenate([np.arange(120), np.arange(300, 340)]).astype(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------
# An id the graph has held before is inserted again (graph.rs:260-261: the node is replaced, len counts it again; the lists of
# other nodes that name it keep naming it and lead to the new vector -- tests/test_hnsw_oracle.py pins the restatement's
# behaviour on graphs small enough to check by hand).  Every case starts from a BULK build and one search, so that the device
# mirror exists, is clean and is brought up to date incrementally from then on.
# ---------------------------------------------------------------------------------------------------------------------------
READD_SHAPE = dict(n=2000, d=16, m=6, efc=48)


def readd_base(vdb, metric, seed, n=None):
    n = n or READD_SHAPE["n"]
    d, m, efc = READD_SHAPE["d"], READD_SHAPE["m"], READD_SHAPE["efc"]
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    g, o, ids = build_pair(vdb, metric, rows, m, efc, 50, seed=seed)
    queries = rng.standard_normal((12, d)).astype(np.float32)
    assert_same_results(g, o, queries, 10, 64)                         # the mirror is uploaded and clean
    assert g.build_stats()["frontier_inserts"] == n
    return g, o, [int(i) for i in ids], rows, queries, rng


def in_links(o, ids, target):
    """(owner, layer) of every list of ANOTHER node that names `target`, from the restatement."""
    out = []
    for i in ids:
        if i == target:
            continue
        for l in range(o.level(i) + 1):
            if target in o.neighbors(i, l):
                out.append((i, l))
    return out


def check_both_walks(g, o, ids, queries, k=10, ef=64):
    """graph, then the device-resident walk (nothing redone on the host) and the forced host traversal against the restatement"""
    assert_same_graph(g, o, ids)
    assert_same_results(g, o, queries, k, ef)
    assert g.stats()["host_redone"] == 0, g.stats()
    g.set_traversal(host_only=True)
    assert_same_results(g, o, queries, k, ef)
    g.set_traversal(host_only=False)


def near(rng, vecs, count, scale=0.05):
    vecs = np.asarray(vecs, dtype=np.float32)
    return (vecs[rng.integers(0, len(vecs), count)] + scale * rng.standard_normal((count, vecs.shape[1]))).astype(np.float32)


def grow_and_check(vdb, g, o, ids, rng, around, queries):
    """One more fresh bulk (the speculative walks) and single adds close to `around` -- the old and new places of the re-added
    ids, where the lists that name them are: with m this small the new back-links make those lists outgrow m and be pruned,
    which is where a wrong cached edge distance would show (graph.rs:221-235 scores from the stored vectors)."""
    nxt = max(ids) + 1
    bulk = near(rng, around, 96)
    g.build_batch((np.arange(nxt, nxt + 96, dtype=np.uint64), bulk))
    for j, v in enumerate(bulk):
        o.insert(nxt + j, v)
    singles = near(rng, around, 24)
    for j, v in enumerate(singles):
        g.add(nxt + 96 + j, vdb.Vector(v))
        o.insert(nxt + 96 + j, v)
    ids = ids + list(range(nxt, nxt + 120))
    check_both_walks(g, o, ids, np.concatenate([queries, bulk[:4], singles[:4]]))
    return ids


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_readd_present_ids_at_the_same_a_lower_and_a_higher_level(vdb, metric):
    g, o, ids, rows, queries, rng = readd_base(vdb, metric, seed=40 + metric)
    n = len(ids)
    by_level = {lv: [i for i in ids if o.level(i) == lv] for lv in range(4)}
    high = [i for i in ids if o.level(i) >= 2][:3]                     # re-added at level 0
    low = by_level[0][:4]                                              # re-added at level 3
    same = by_level[1][:2] + by_level[0][4:6]                          # re-added at the level they have
    assert len(high) == 3 and len(low) == 4 and len(same) == 4
    old_vecs, new_vecs = [], []

    def readd(i, level):
        v = near(rng, rows[rng.integers(0, n, 1)], 1, 0.3)[0]          # somewhere else in the data
        old_vecs.append(rows[i]); new_vecs.append(v)
        g.add(i, vdb.Vector(v), level=level)
        o.insert(i, v, level)

    for i in same:
        readd(i, o.level(i))
    check_both_walks(g, o, ids, np.concatenate([queries, np.array(new_vecs)]))
    for i in high:
        above = [(j, l) for j, l in in_links(o, ids, i) if l >= 1]
        assert above, i                                                # lists above layer 0 name the id ...
        readd(i, 0)
        assert o.level(i) == 0 and [(j, l) for j, l in in_links(o, ids, i) if l >= 1] == above      # ... and still do, above its new level
    check_both_walks(g, o, ids, np.concatenate([queries, np.array(new_vecs)]))
    for i in low:                                                      # a search between the re-adds: the mirror is synced each time
        readd(i, 3)
        assert o.level(i) == 3 and o.neighbors(i, 1) and o.neighbors(i, 3) is not None      # three upper lists where it had none
        assert_same_results(g, o, np.array(new_vecs[-2:]), 10, 64)
    check_both_walks(g, o, ids, np.concatenate([queries, np.array(new_vecs)]))
    assert g.len() == len(o) == n + 11                                 # graph.rs:261: every re-add counts again
    assert g.build_stats()["frontier_inserts"] == n                    # (the re-adds took the path of their own)
    grow_and_check(vdb, g, o, ids, rng, np.array(old_vecs + new_vecs), queries)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_readd_the_entry_point_at_level_0(vdb, metric):
    """The entry point and max_level are only ever raised (graph.rs:336-339): the re-added node keeps the role with a level below
    max_level, lists only itself, and every search from then on answers with it alone.  A graph of its own."""
    g, o, ids, rows, queries, rng = readd_base(vdb, metric, seed=50 + metric, n=1500)
    ep, top = o.entry_point()
    assert top >= 1
    v = near(rng, rows[7:8], 1)[0]
    g.add(ep, vdb.Vector(v), level=0)
    o.insert(ep, v, 0)
    assert o.entry_point() == (ep, top) and o.level(ep) == 0 and o.neighbors(ep, 0) == [ep, ep]
    check_both_walks(g, o, ids, queries)
    gi, _, gc = g.search_batch_arrays(queries, 10, 64)
    assert np.all(gc == 1) and np.all(gi[:, 0] == ep)
    # a fresh bulk on top: its speculative walks start from that entry point, above its level
    more = rng.standard_normal((128, rows.shape[1])).astype(np.float32)
    nxt = len(ids)
    g.build_batch((np.arange(nxt, nxt + 128, dtype=np.uint64), more))
    for j, x in enumerate(more):
        o.insert(nxt + j, x)
    check_both_walks(g, o, ids + list(range(nxt, nxt + 128)), np.concatenate([queries, more[:6]]))


@pytest.mark.parametrize("frontier_only", [True, False])
def test_readded_ids_inside_a_bulk(vdb, frontier_only):
    """Present ids and a removed id in the middle of a bulk of fresh ones, levels from the seeded stream: the batch is inserted
    one vector after the other like the reference's build_batch (mod.rs:37-42)."""
    g, o, ids, rows, queries, rng = readd_base(vdb, 0, seed=60)
    n = len(ids)
    g.set_build(frontier_only)
    g.remove(55); o.remove(55)
    assert in_links(o, ids, 55)                                        # a list still names the removed id
    assert_same_results(g, o, queries, 10, 64)
    present = [int(i) for i in rng.choice([i for i in ids if i != 55], 12, replace=False)]
    batch_ids = list(range(n, n + 180))
    for t, i in enumerate(present):
        batch_ids.insert(5 + 14 * t, i)                                # runs of 5 .. 14 fresh ids between them, a long one at the end
    batch_ids.insert(100, 55)
    anchors = np.concatenate([rows[present], rows[[55]]])
    batch = near(rng, anchors, len(batch_ids), 0.2)
    before = g.build_stats()
    g.build_batch((np.array(batch_ids, dtype=np.uint64), batch))
    for i, v in zip(batch_ids, batch):
        o.insert(i, v)
    after = g.build_stats()
    fresh = after["frontier_inserts"] - before["frontier_inserts"] + after["scan_inserts"] - before["scan_inserts"]
    assert fresh == 180, (before, after)                               # the 13 others did not take a fresh id's path
    ids = ids + list(range(n, n + 180))
    assert g.len() == len(o) == n - 1 + len(batch_ids)
    check_both_walks(g, o, ids, np.concatenate([queries, batch[:8]]))
    g.set_build(True)
    grow_and_check(vdb, g, o, ids, rng, np.concatenate([anchors, batch[[5, 19, 33, 100]]]), queries)


@pytest.mark.parametrize("frontier_only", [True, False])
def test_the_same_id_twice_in_one_bulk(vdb, frontier_only):
    """The reference inserts the first vector, then replaces it with the second (graph.rs:260): both walks happen, with THEIR
    vectors, and the id counts twice."""
    g, o, ids, rows, queries, rng = readd_base(vdb, 0, seed=70, n=1200)
    n = len(ids)
    g.set_build(frontier_only)
    batch_ids = list(range(n, n + 100))
    batch_ids[60] = n + 10                                             # far apart
    batch_ids[31] = n + 30                                             # back to back
    batch_ids[99] = n + 98                                             # the last two
    batch = near(rng, rows[:50], 100, 0.5)
    g.build_batch((np.array(batch_ids, dtype=np.uint64), batch))
    for i, v in zip(batch_ids, batch):
        o.insert(i, v)
    assert g.len() == len(o) == n + 100
    ids = ids + sorted(set(batch_ids))
    check_both_walks(g, o, ids, np.concatenate([queries, batch[[10, 60, 30, 31, 98, 99]]]))
    gi, gd, _ = g.search_batch_arrays(batch[[60, 10]], 1, 64)
    assert gi[0, 0] == n + 10 and gd[0, 0] == 0.0 and not (gi[1, 0] == n + 10 and gd[1, 0] == 0.0)     # the second vector is the stored one
    g.set_build(True)
    grow_and_check(vdb, g, o, ids, rng, batch[[10, 60, 30, 31, 98, 99]], queries)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_remove_search_readd(vdb, metric):
    g, o, ids, rows, queries, rng = readd_base(vdb, metric, seed=80 + metric)
    n = len(ids)
    victims = list(range(100, 130))
    for i in victims:
        g.remove(i); o.remove(i)
    dangling = [i for i in victims if in_links(o, ids, i)]
    assert len(dangling) >= 5, dangling                                # remove cleans only the lists of the node's own neighbours
    check_both_walks(g, o, ids, queries)                               # the mirror is rebuilt without them
    new = near(rng, rows[rng.integers(0, n, len(victims))], len(victims), 0.3)
    for t, i in enumerate(victims):
        level = [-1, 0, 2][t % 3]                                      # from the seeded stream, or forced
        g.add(i, vdb.Vector(new[t]), level=level)
        o.insert(i, new[t], level)
        if t % 10 == 0:
            assert_same_results(g, o, new[t:t + 1], 10, 64)
    assert g.len() == len(o) == n
    for i in dangling:
        assert in_links(o, ids, i)
    check_both_walks(g, o, ids, np.concatenate([queries, new[:8]]))
    grow_and_check(vdb, g, o, ids, rng, np.concatenate([rows[victims], new]), queries)
