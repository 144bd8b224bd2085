"""Shared by tests/test_hnsw_limits_cpu.py and tests/test_gpu_hnsw_limits.py: the capacities of the device-resident HNSW walk
(kernels_hnsw.hip hnsw_search_kernel) as the tests state them, the data sets that are built to cross them, and the CPU
prediction of which walks overflow.

The capacities are restated here ONCE; the CPU file checks them against the kernel source, the routing constants against
hnsw_search_supported, include/vdb_hnsw.h and DESIGN.md, so a change of the kernel that is not made here fails without a GPU.

  VISITED_MAX     a plain walk fails once a layer's visited set exceeds 3/4 of VIS_CAP
  CAND_CAP(_F)    a walk fails when it would push onto a full candidate heap (plain / pre-filtered)
  DEVICE_EF_MAX   max(ef, k) up to this is walked on the device (max(ef, k) + 1 <= RES_CAP), above it on the host
  DEVICE_M_MAX    m up to this is walked on the device (m_max0 + 1 = 2 m + 1 <= MAXP = 40)
  WAVE_POP_MAX    result heaps up to this length are popped by the wave (four ballots), longer ones by a single lane
"""
import numpy as np

import oracle
from hnsw_filter_restatement import Walker, eligible_fn

VIS_CAP, CAND_CAP, CAND_CAP_F, RES_CAP, MAXP, WAVE_POP_MAX = 16384, 4096, 11264, 1024, 40, 514
VISITED_MAX = VIS_CAP // 4 * 3
DEVICE_EF_MAX = RES_CAP - 1
DEVICE_M_MAX = (MAXP - 1) // 2

# ---- the ef / k edges of the result heap (one graph per metric and data kind)
EF_SHAPE = dict(n=3000, d=16, m=16, efc=64, nq=12)
EF_VALUES = (511, 512, 513, 514, 515, 1021, 1022, 1023, 1024, 1100)
LARGE_K = ((600, 50), (1022, 10), (1023, 10), (513, 513), (514, 1))          # (k, ef)
TIE_EF_VALUES = (513, 514, 1022)

# ---- ef_construction across the wave-pop boundary
EFC_SHAPE = dict(n=2500, d=16, m=8, nq=8)
EFC_VALUES = (513, 514, 600)

# ---- walks that overflow: n and the seed are chosen so that the conditions of test_hnsw_limits_cpu.py hold
OVERFLOW = dict(n=45000, d=48, m=19, efc=12, metric=0, seed=20, graph_seed=5)
OVERFLOW_PLAIN = dict(nq=16, ef=1022, k=10)
OVERFLOW_FILTERED = dict(near=6, far=6, ef=200, k=10, threshold=1.8, seed=1)


def build_oracle(metric, rows, m, efc, seed, ids=None):
    o = oracle.HnswOracle(metric, m=m, ef_construction=efc, ef_search=50, seed=seed)
    for i, v in zip(range(rows.shape[0]) if ids is None else ids, rows):
        o.insert(int(i), v)
    return o


def gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def dups(seed, n, d, shift=0.0):
    """every row drawn from n / 8 base rows (tools/fuzz_hnsw.py "dups"): exact distance ties everywhere"""
    rng = np.random.default_rng(seed)
    base = rng.random((max(n // 8, 1), d), dtype=np.float32) - np.float32(shift)
    return np.ascontiguousarray(base[rng.integers(0, base.shape[0], n)])


def ef_data(metric, kind):
    """-> rows, queries, graph seed of the ef / k edge graph"""
    s = EF_SHAPE
    seed = 500 + 10 * metric + (0 if kind == "gauss" else 1)
    # DotProduct over all-positive rows builds a graph in which fewer than 900 of the 3000 nodes are reachable (the large rows
    # are everyone's neighbours): the result heap would never fill at ef = 1022.  Its duplicated rows are centred instead.
    shift = 0.5 if metric == 2 else 0.0
    rows = gauss(seed, s["n"], s["d"]) if kind == "gauss" else dups(seed, s["n"], s["d"], shift)
    rng = np.random.default_rng(seed + 100)
    queries = rng.standard_normal((s["nq"], s["d"])).astype(np.float32) if kind == "gauss" else rng.random((s["nq"], s["d"]), dtype=np.float32) - np.float32(shift)
    return rows, queries, 31 + metric


def overflow_data():
    """-> rows, the 16 plain queries, the eligibility of the filtered case, its 12 queries (6 near eligible rows, then the same 6
    mirrored in the first coordinate: far from every eligible row)"""
    c, f = OVERFLOW, OVERFLOW_FILTERED
    rng = np.random.default_rng(c["seed"])
    rows = rng.standard_normal((c["n"], c["d"])).astype(np.float32)
    plain_q = rng.standard_normal((OVERFLOW_PLAIN["nq"], c["d"])).astype(np.float32)
    elig = rows[:, 0] > np.float32(f["threshold"])                      # ~3 % of the rows, clustered on one side of the data
    rng = np.random.default_rng(f["seed"])
    anchors = rows[rng.choice(np.flatnonzero(elig), f["near"], replace=False)]
    near = (anchors + 0.1 * rng.standard_normal(anchors.shape)).astype(np.float32)
    far = near.copy()
    far[:, 0] = -far[:, 0]
    return rows, plain_q, elig, np.concatenate([near, far[:f["far"]]])


def walk_counters(o, metric, rows, queries, k, ef, elig=None):
    """The restatement's walk of every query -> (results, counters): per query (ids, dists) and the exact counters of
    hnsw_filter_restatement.Walker ("pushed", "layer_visited")."""
    w = Walker(o, metric, {i: rows[i] for i in range(rows.shape[0])})
    res, ctr = [], []
    for q in queries:
        peaks = {}
        res.append(w.search(q, k, ef, None if elig is None else eligible_fn(elig), peaks))
        ctr.append(peaks)
    return res, ctr


def overflows(peaks, filtered):
    """Does the device walk with these counters fail (and is re-run on the host)?  The plain walk keeps every layer's visited set
    in LDS; the pre-filtered one keeps layer 0's in an HBM bitmap (no cap) and has the larger candidate heap.  Its descent
    above layer 0 (ef = 1) uses a small LDS hash, 3/4 of 2048 slots."""
    if filtered:
        return peaks["pushed"] > CAND_CAP_F or max(peaks["layer_visited"][:-1], default=0) > 2048 // 4 * 3
    return peaks["pushed"] > CAND_CAP or max(peaks["layer_visited"]) > VISITED_MAX


# ---- comparisons (ids, order, distance bits)
def same_arrays(a, b):
    (ai, ad, ac), (bi, bd, bc) = a, b
    if not np.array_equal(ac, bc):
        return False
    return all(np.array_equal(ai[q, :ac[q]], bi[q, :bc[q]]) and
               np.array_equal(ad[q, :ac[q]].view(np.uint32), bd[q, :bc[q]].view(np.uint32)) for q in range(ac.size))


def assert_rows_equal(got, expected, what=""):
    """got: (ids [nq, k], dists [nq, k], counts [nq]) of search_batch_arrays; expected: per query (ids, dists)"""
    gi, gd, gc = got
    assert len(expected) == gc.size
    for b, (ei, ed) in enumerate(expected):
        assert gc[b] == len(ei), (what, b, int(gc[b]), len(ei))
        assert np.array_equal(gi[b, :gc[b]], ei), (what, b, gi[b, :gc[b]], ei)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), np.asarray(ed, np.float32).view(np.uint32)), (what, b, gd[b, :gc[b]], ed)


def oracle_results(o, queries, k, ef):
    return [o.search(q, k, ef) for q in queries]


def assert_same_graph(g, o, ids):
    assert g.len() == len(o)
    assert g.entry_point() == o.entry_point()
    for i in ids:
        lv = o.level(int(i))
        assert g.level(int(i)) == lv, i
        for l in range(lv + 1):
            assert g.neighbors(int(i), l) == o.neighbors(int(i), l), (int(i), l)
        assert g.neighbors(int(i), lv + 1) is None


def routed_search(g, queries, k, ef, device, **kw):
    """search_batch_arrays with the routing asserted from the stats deltas: a device-resident search raises device_queries by nq
    and leaves host_redone alone; a host-routed one changes neither and counts traversal rounds."""
    before = g.stats()
    out = g.search_batch_arrays(queries, k, ef, **kw)
    after = g.stats()
    dq, hr = after["device_queries"] - before["device_queries"], after["host_redone"] - before["host_redone"]
    if device:
        assert dq == len(queries) and hr == 0, (k, ef, dq, hr, after)
    else:
        assert dq == 0 and hr == 0 and after["last_search_rounds"] > 0, (k, ef, dq, hr, after)
    return out
