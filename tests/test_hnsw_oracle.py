"""The HNSW oracle (oracle/hnsw_oracle.c) against the reference's own unit tests for this module
(src/hnsw/graph.rs:436-538, src/hnsw/neighbor_queue.rs:150-195, src/hnsw/mod.rs:84-154) and the recall
floors of tests/recall_test.rs:67-80.  CPU only."""
import numpy as np
import pytest

import oracle

EUCLID = 0


def make_graph(seed=1):
    return oracle.HnswOracle(EUCLID, m=4, ef_construction=32, ef_search=16, seed=seed)      # graph.rs:432-434 make_params


def test_heaps_pop_in_neighbor_order():
    # neighbor_queue.rs:154-176: max-heap pops 3,2,1 ; min-heap pops 1,2,3
    d, _ = oracle.heap_replay(+1, [3.0, 1.0, 2.0], [0, 1, 2])
    assert list(d) == [3.0, 2.0, 1.0]
    d, _ = oracle.heap_replay(-1, [3.0, 1.0, 2.0], [0, 1, 2])
    assert list(d) == [1.0, 2.0, 3.0]
    # neighbor_queue.rs:178-189 push_bounded(limit 2) keeps the two closest
    d, _ = oracle.heap_replay(+1, [5.0, 1.0, 3.0], [0, 1, 2], bound=2)
    assert sorted(d) == [1.0, 3.0]
    # ties on distance order by id (neighbor_queue.rs:37-43)
    d, i = oracle.heap_replay(-1, [1.0, 1.0, 1.0, 0.5], [7, 3, 5, 9])
    assert list(i) == [9, 3, 5, 7]


def test_levels_follow_the_reference_formula():
    # graph.rs:118-123: floor(-ln(r) * 1/ln(m)), capped at max_layers - 1
    assert oracle.hnsw_level_from_unit(0.9) == 0
    assert oracle.hnsw_level_from_unit(1.0 / 16 - 1e-9) == 1
    assert oracle.hnsw_level_from_unit(1.0 / 256 - 1e-12) == 2
    assert oracle.hnsw_level_from_unit(0.0) == 15
    assert oracle.hnsw_level_from_unit(1e-300) == 15


def test_insert_single_and_multiple():
    g = make_graph()
    g.insert(0, [1.0, 0.0, 0.0])
    assert len(g) == 1 and g.entry_point()[0] == 0                     # graph.rs:436-443
    g = make_graph()
    for i in range(10):
        g.insert(i, [float(i), 0.0, 0.0])
    assert len(g) == 10                                                 # graph.rs:446-454


def test_self_search():
    # graph.rs:457-485: every inserted vector finds itself at distance ~0
    g = make_graph()
    vecs = [np.array([i * 0.1, (i * 7) * 0.1, (i * 13) * 0.1], dtype=np.float32) for i in range(100)]
    for i, v in enumerate(vecs):
        g.insert(i, v)
    for i, v in enumerate(vecs):
        ids, ds = g.search(v, 1, 16)
        assert len(ids) == 1 and ds[0] < 1e-5, (i, ids, ds)


def test_search_knn():
    # graph.rs:488-504
    g = make_graph()
    for i in range(5):
        g.insert(i, [float(i), 0.0])
    ids, ds = g.search([0.5, 0.0], 2, 16)
    assert len(ids) == 2 and set(ids) == {0, 1}


def test_remove_and_remove_entry_point():
    g = make_graph()
    g.insert(0, [1.0, 0.0])
    g.insert(1, [0.0, 1.0])
    g.remove(0)
    assert len(g) == 1                                                  # graph.rs:507-520
    ids, _ = g.search([0.0, 1.0], 1, 16)
    assert ids[0] == 1
    g.remove(99)                                                        # absent id: Ok(())  (graph.rs:346-348)
    g = make_graph()
    g.insert(0, [1.0, 0.0]); g.insert(1, [0.0, 1.0]); g.insert(2, [1.0, 1.0])
    ep, _ = g.entry_point()
    g.remove(ep)                                                        # graph.rs:523-537
    assert len(g) == 2
    ids, _ = g.search([0.0, 1.0], 1, 16)
    assert len(ids) == 1


def test_hnsw_index_via_trait():
    # mod.rs:88-98 (default params m=16, ef_construction=200; search ef = 50)
    g = oracle.HnswOracle(EUCLID)
    g.insert(0, [1.0, 0.0, 0.0]); g.insert(1, [0.0, 1.0, 0.0]); g.insert(2, [1.0, 1.0, 0.0])
    ids, ds = g.search([1.0, 0.0, 0.0], 2)
    assert len(ids) == 2 and ids[0] == 0 and ds[0] < 1e-5


def test_structure_invariants():
    rng = np.random.default_rng(3)
    g = oracle.HnswOracle(EUCLID, m=8, ef_construction=64, ef_search=32, seed=11)
    rows = rng.random((600, 16), dtype=np.float32)
    for i, v in enumerate(rows):
        g.insert(i, v)
    ep, max_level = g.entry_point()
    assert g.level(ep) == max_level == max(g.level(i) for i in range(600))
    for i in range(600):
        for l in range(g.level(i) + 1):
            nb = g.neighbors(i, l)
            assert len(nb) <= (16 if l == 0 else 8) and len(set(nb)) == len(nb) and i not in nb
            assert all(g.level(j) >= l for j in nb)                      # links only between nodes that exist on the layer
    assert g.neighbors(0, g.level(0) + 1) is None


@pytest.mark.parametrize("n,dim,nq,floor", [(100, 32, 50, 0.90), (1000, 64, 50, 0.90), (5000, 128, 20, 0.85)])
def test_recall_floors_of_the_reference(n, dim, nq, floor):
    # tests/recall_test.rs:28-80: HnswParams::new(16, 200, 50), search_with_ef(k = 10, ef = 100), uniform[0,1) data
    rng = np.random.default_rng(n)
    rows = rng.random((n, dim), dtype=np.float32)
    queries = rng.random((nq, dim), dtype=np.float32)
    g = oracle.HnswOracle(EUCLID, m=16, ef_construction=200, ef_search=50, seed=n)
    for i, v in enumerate(rows):
        g.insert(i, v)
    total = 0.0
    for q in queries:
        truth, _ = oracle.flat_search(EUCLID, rows, q, 10)
        ids, ds = g.search(q, 10, 100)
        assert np.all(ds[1:] >= ds[:-1])
        total += oracle.recall(truth, ids)
    assert total / nq >= floor, total / nq


# ---------------------------------------------------------------------------------------------------------------------------
# An id the graph has held before is inserted again.  HnswGraph::insert replaces whatever the slot holds and counts it again
# (graph.rs:260-261 `self.nodes[id] = Some(node); self.count += 1`); every list of ANOTHER node that names the id keeps naming
# it and from then on leads to the new vector (search_layer :169-182 and prune_neighbors :221-235 read the stored vector).
# The reference cannot be compiled where these tests run, so the expected graphs below are worked out by hand from the cited
# lines: points on a line (dim 1, Euclidean: d = |x - y|), m = 2 (m_max0 = 4), forced levels, and ef_construction = 8 >= the
# number of nodes, so that a search_layer over a connected layer returns EVERY node of it, nearest first.
# ---------------------------------------------------------------------------------------------------------------------------
def line_graph():
    return oracle.HnswOracle(EUCLID, m=2, ef_construction=8, ef_search=8, seed=1)


def lists(g, ids, layer=0):
    return {i: g.neighbors(i, layer) for i in ids}


def four_on_a_line():
    """ids 0..3 at x = 0, 1, 2, 3, all of level 0.  Insert k finds every earlier node, nearest first (k-1, .., 0), lists
    them all (<= m_max0 = 4) and is appended to each of their lists (:309-321); no list outgrows 4, nothing is pruned."""
    g = line_graph()
    for i in range(4):
        g.insert(i, [float(i)], 0)
    assert lists(g, range(4)) == {0: [1, 2, 3], 1: [0, 2, 3], 2: [1, 0, 3], 3: [2, 1, 0]}
    return g


def readd_1_at_10(g):
    """insert(1, x = 10, level 0) over four_on_a_line().  Node 1 is replaced by a node without links (:254-261), len = 5.
    The walk (:295-296) starts at the entry point 0 (d 10) and expands it: its list [1, 2, 3] still names id 1, which now
    holds x = 10: d(1) = 0, d(2) = 8, d(3) = 7.  Popped next: 1 (its list is empty), 3 and 2 (all visited).  nearest =
    [1 (0), 3 (7), 2 (8), 0 (10)], so the new node lists ITSELF first: neighbors[0] = [1, 3, 2, 0] (:299-306).  Back-links in
    that order (:309-327): to node 1 itself -> [1, 3, 2, 0, 1], 5 > m_max0 -> pruned at once from the stored vectors:
    (1, 0) (3, 7) (2, 8) (0, 10) (1, 0), stable sort -> 1 1 3 2 0, truncated to [1, 1, 3, 2]; then 3, 2 and 0 get id 1
    appended a SECOND time beside the in-link they already had (4 entries each: not pruned)."""
    g.insert(1, [10.0], 0)
    return g


def test_readd_present_id_keeps_in_links_and_counts_twice():
    g = four_on_a_line()
    in_links_before = [i for i in (0, 2, 3) if 1 in g.neighbors(i, 0)]
    assert in_links_before == [0, 2, 3]
    readd_1_at_10(g)
    assert len(g) == 5                                                    # graph.rs:261: count += 1, the id counts twice
    assert g.level(1) == 0 and g.entry_point() == (0, 0)
    for i in (0, 2, 3):                                                   # the old in-link is still there, in its old place
        assert g.neighbors(i, 0)[:3] == {0: [1, 2, 3], 2: [1, 0, 3], 3: [2, 1, 0]}[i]
    ids, ds = g.search([10.0], 1, 8)                                      # reached from 0 through the OLD in-link, at the NEW distance
    assert list(ids) == [1] and ds[0] == 0.0
    # q = 0.9: 0 (0.9), then 0's list: 1 (|10 - 0.9|), 2 (1.1), 3 (2.1); everything else is visited
    ids, ds = g.search([0.9], 4, 8)
    assert list(ids) == [0, 2, 3, 1]
    assert ds[3] == np.float32(oracle.distance(EUCLID, [0.9], [10.0])) and abs(ds[3] - 9.1) < 1e-5


def test_readded_node_lists_itself_twice():
    g = readd_1_at_10(four_on_a_line())
    assert lists(g, range(4)) == {0: [1, 2, 3, 1], 1: [1, 1, 3, 2], 2: [1, 0, 3, 1], 3: [2, 1, 0, 1]}


def two_layers():
    """0 (x = 0, level 1), 1 (x = 1, level 1), 2 (x = 2, level 0).  Insert 1: layers 1 and 0 from the entry point 0: lists [0]
    on both, 0 gets [1] on both; level 1 is not above max_level 1, the entry point stays 0 (:336-339).  Insert 2: greedy
    descent on layer 1 (:277-284) 0 (d 2) -> 1 (d 1); layer 0 from 1: nearest [1, 0]."""
    g = line_graph()
    g.insert(0, [0.0], 1); g.insert(1, [1.0], 1); g.insert(2, [2.0], 0)
    assert lists(g, range(3)) == {0: [1, 2], 1: [0, 2], 2: [1, 0]}
    assert g.neighbors(0, 1) == [1] and g.neighbors(1, 1) == [0] and g.entry_point() == (0, 1)
    return g


def test_readd_with_a_lower_level_keeps_the_in_link_above_it():
    """insert(1, x = 5, level 0): node 1 now has ONE list.  Phase 1 on layer 1 from 0 (d 5): 0's layer-1 list [1] leads to the
    new vector (d 0); 1 is popped but `layer < node.neighbors.len()` (:170) is 1 < 1: not expanded.  ep = 1 -- the node itself.
    Layer 0 from 1: its list is empty, nearest = [1]: neighbors[0] = [1], the back-link loop appends 1 again -> [1, 1]."""
    g = two_layers()
    g.insert(1, [5.0], 0)
    assert len(g) == 4 and g.level(1) == 0 and g.entry_point() == (0, 1)
    assert g.neighbors(0, 1) == [1]                                       # still names id 1 one layer above its level
    assert g.neighbors(1, 1) is None and g.neighbors(1, 0) == [1, 1]
    assert lists(g, (0, 2)) == {0: [1, 2], 2: [1, 0]}
    # q = 5: layer 1 reaches 1 through 0's list and does not expand it (no list there); layer 0 starts at 1, whose list names
    # only itself: the search ends with [1]
    ids, ds = g.search([5.0], 3, 8)
    assert list(ids) == [1] and ds[0] == 0.0
    # q = 0.2: layer 1 stays at 0 (d(1) = 4.8 is no improvement at ef = 1); layer 0: 0 (0.2), its list: 1 (4.8), 2 (1.8)
    ids, ds = g.search([0.2], 3, 8)
    assert list(ids) == [0, 2, 1]


def test_readd_the_entry_point_at_level_0():
    """insert(0, x = 0.5, level 0) over two_layers(): the entry point and max_level are only ever raised (:336-339), so they stay
    (0, 1) while node 0 has level 0.  Its walk starts at itself: not expanded on layer 1 (:170), no list yet on layer 0:
    neighbors[0] = [0], plus its own back-link -> [0, 0].  Every later search starts at 0, finds no list on layer 1 and only
    itself on layer 0: it answers [0]."""
    g = two_layers()
    g.insert(0, [0.5], 0)
    assert len(g) == 4 and g.entry_point() == (0, 1) and g.level(0) == 0
    assert g.neighbors(0, 0) == [0, 0] and g.neighbors(0, 1) is None
    assert g.neighbors(1, 1) == [0] and lists(g, (1, 2)) == {1: [0, 2], 2: [1, 0]}
    for x in (0.5, 2.0, -7.0):
        ids, ds = g.search([x], 3, 8)
        assert list(ids) == [0] and ds[0] == np.float32(abs(x - 0.5))


def test_readd_a_removed_id_revives_the_dangling_link():
    """ids 0..5 at x = 0..5, level 0.  Up to id 4 every node lists every other (<= 4 entries).  Insert 5: nearest [4, 3, 2, 1, 0],
    takes [4, 3, 2, 1]; each of them outgrows 4 entries and is pruned (stable sort by distance to the owner, :234):
      4: (3,1) (2,2) (1,3) (0,4) (5,1) -> [3, 5, 2, 1]   -- 4 drops 0, but 0 still lists 4
      3: (2,1) (1,2) (0,3) (4,1) (5,2) -> [2, 4, 1, 5]
      2: (1,1) (0,2) (3,1) (4,2) (5,3) -> [1, 3, 0, 4]
      1: (0,1) (2,1) (3,2) (4,3) (5,4) -> [0, 2, 3, 4]
    remove(4) cleans only the lists of 4's OWN neighbours 3, 5, 2, 1 (:350-360): 0 keeps [1, 2, 3, 4], a dangling link.
    insert(4, x = -1, level 0): the walk from 0 (d 1) expands 0's list: 1 (2), 2 (3), 3 (4), 4 (0: live again); 5 (6) is reached
    through 3.  nearest [4, 0, 1, 2, 3, 5] -> neighbors[0] = [4, 0, 1, 2].  Back-links: 4 itself -> [4, 0, 1, 2, 4] -> pruned
    (4,0) (0,1) (1,2) (2,3) (4,0) -> [4, 4, 0, 1]; 0 -> [1, 2, 3, 4, 4] -> pruned from the stored vectors, 4 at its NEW place:
    (1,1) (2,2) (3,3) (4,1) (4,1) -> [1, 4, 4, 2]; 1 and 2 have room."""
    g = line_graph()
    for i in range(6):
        g.insert(i, [float(i)], 0)
    assert lists(g, range(6)) == {0: [1, 2, 3, 4], 1: [0, 2, 3, 4], 2: [1, 3, 0, 4], 3: [2, 4, 1, 5], 4: [3, 5, 2, 1], 5: [4, 3, 2, 1]}
    g.remove(4)
    assert len(g) == 5 and g.level(4) == -1
    assert lists(g, (0, 1, 2, 3, 5)) == {0: [1, 2, 3, 4], 1: [0, 2, 3], 2: [1, 3, 0], 3: [2, 1, 5], 5: [3, 2, 1]}
    ids, _ = g.search([4.2], 2, 8)                                        # the dangling link is skipped (:177-180)
    assert list(ids) == [5, 3]
    g.insert(4, [-1.0], 0)
    assert len(g) == 6
    assert lists(g, range(6)) == {0: [1, 4, 4, 2], 1: [0, 2, 3, 4], 2: [1, 3, 0, 4], 3: [2, 1, 5], 4: [4, 4, 0, 1], 5: [3, 2, 1]}
    ids, ds = g.search([-1.0], 1, 8)
    assert list(ids) == [4] and ds[0] == 0.0
