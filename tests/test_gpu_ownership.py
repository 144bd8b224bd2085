"""The re-allocation edges of the host code (csrc/vdb_device.h owns every device buffer, pinned buffer, stream and event): a
buffer regrown, dropped and made again, or carried over into a larger one must change no result.  Every case compares ids and
distance bits with the CPU oracle.  (What happens when an allocation FAILS is checked on the CPU, tests/test_device_own_cpu.py.)"""
import gc

import numpy as np
import pytest

import filter_programs as fp
import oracle
from conftest import load_package
from hnsw_filter_restatement import Walker, eligible_fn, mask_of
from test_gpu_device_filter import read_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def check_flat(metric, rows, ids, ix, q, k, qsel=None):
    gi, gd, gc_ = ix.search_batch_arrays(q, k)
    for b in (range(q.shape[0]) if qsel is None else qsel):
        oi, od = oracle.flat_search(metric, rows, q[b], k, ids=ids)
        assert gc_[b] == len(oi), (b, gc_[b], len(oi))
        assert np.array_equal(gi[b, :gc_[b]], oi), (b, gi[b, :gc_[b]], oi)
        assert np.array_equal(gd[b, :gc_[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc_[b]], od)


# ------------------------------------------------------------------ flat store
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_rows_carry_over_a_capacity_boundary(vdb, metric, shadow):
    """1000 rows (capacity 1024), then 100 more: the store is re-allocated at 2048 and the uploaded rows, norms, scores, margins
    (none under Cosine) and ids are copied over; with the bf16 shadow switched on in between, the shadow is built in the new store."""
    rng = np.random.default_rng(40 + metric)
    rows = rng.standard_normal((1100, 24)).astype(np.float32)
    ids = np.arange(1100, dtype=np.uint64)
    q = rng.standard_normal((5, 24)).astype(np.float32)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
    ix.add_bulk(rows[:1000], ids=ids[:1000])
    check_flat(metric, rows[:1000], ids[:1000], ix, q, 10)
    assert ix.store_stats()[2] == 1024
    if shadow:
        ix.set_shadow(True)
    ix.add_bulk(rows[1000:], ids=ids[1000:])
    check_flat(metric, rows, ids, ix, q, 10)
    assert ix.store_stats()[2] == 2048


def test_empty_and_refill_at_another_dimension(vdb):
    rng = np.random.default_rng(50)
    a = rng.standard_normal((200, 24)).astype(np.float32)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    ix.add_bulk(a)
    check_flat(0, a, None, ix, a[:3], 5)
    for i in range(200):
        ix.remove(i)                                                                   # the last one frees the store
    assert ix.len() == 0 and ix.store_stats()[2] == 0
    b = rng.standard_normal((300, 40)).astype(np.float32)
    ix.add_bulk(b)
    assert ix.dim() == 40
    check_flat(0, b, None, ix, b[:3] + 0.5, 7)


def test_shadow_on_off_on(vdb):
    rng = np.random.default_rng(51)
    rows = rng.standard_normal((1500, 40)).astype(np.float32)
    q = rng.standard_normal((4, 40)).astype(np.float32)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(2), keep_host_copy=False)
    ix.add_bulk(rows)
    for on in (True, False, True):
        ix.set_shadow(on)
        check_flat(2, rows, None, ix, q, 10)


def test_sample_copy_rebuilt_dropped_and_made_again(vdb):
    """65536 rows x 64 is the smallest index with a bf16 copy of the sample rows."""
    rng = np.random.default_rng(52)
    rows = rng.random((65536 + 256, 64), dtype=np.float32)
    q = rng.random((4, 64), dtype=np.float32)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    ix.add_bulk(rows[:65536])
    check_flat(0, rows[:65536], None, ix, q, 10)
    assert ix.last_stats()["bf16_screen"] == 1
    ix.add_bulk(rows[65536:], first_id=65536)
    check_flat(0, rows, None, ix, q, 10)                                               # the copy is rebuilt for the new row count
    ix.set_sample_cache(False)
    check_flat(0, rows, None, ix, q, 10)
    ix.set_sample_cache(True)
    check_flat(0, rows, None, ix, q, 10)
    assert ix.last_stats()["bf16_screen"] == 1


# ------------------------------------------------------------------ HNSW
def check_hnsw(g, o, w, q, k, ef, elig=None):
    if elig is None:
        gi, gd, gc_ = g.search_batch_arrays(q, k, ef)
    else:
        mask, bits = mask_of(elig)
        gi, gd, gc_ = g.search_batch_arrays(q, k, ef, id_mask=mask, mask_bits=bits)
    for b in range(q.shape[0]):
        oi, od = o.search(q[b], k, ef) if elig is None else w.search(q[b], k, ef, eligible_fn(elig))
        assert gc_[b] == len(oi), (b, gc_[b], len(oi))
        assert np.array_equal(gi[b, :gc_[b]], oi), (b, gi[b, :gc_[b]], oi)
        assert np.array_equal(gd[b, :gc_[b]].view(np.uint32), np.asarray(od, dtype=np.float32).view(np.uint32)), b


@pytest.mark.parametrize("frontier_only", [True, False])
def test_hnsw_buffers_regrow_and_the_mirror_is_rebuilt(vdb, frontier_only):
    rng = np.random.default_rng(60)
    n0, n1, d = 300, 1800, 16
    rows = rng.standard_normal((n1, d)).astype(np.float32)                             # Gaussian: no distance ties
    q = rng.standard_normal((64, d)).astype(np.float32)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric(0), vdb.HnswParams.new(8, 64, 50), seed=9)
    g.set_build(frontier_only)
    o = oracle.HnswOracle(0, m=8, ef_construction=64, ef_search=50, seed=9)
    w = Walker(o, 0, {i: rows[i] for i in range(n1)})
    g.build_batch((np.arange(n0, dtype=np.uint64), rows[:n0]))
    for i in range(n0):
        o.insert(i, rows[i])
    check_hnsw(g, o, w, q[:4], 5, 50)
    check_hnsw(g, o, w, q, 20, 50)                                                      # the out buffers regrow
    check_hnsw(g, o, w, q[:4], 10, 50, elig=rng.random(n0) < 0.5)
    # beyond the mirror's 300 + 300 / 4 + 1024 ids: a full rebuild
    g.build_batch((np.arange(n0, n1, dtype=np.uint64), rows[n0:]))
    for i in range(n0, n1):
        o.insert(i, rows[i])
    w = Walker(o, 0, {i: rows[i] for i in range(n1)})                                  # (a Walker caches the lists it has read)
    check_hnsw(g, o, w, q[:4], 10, 50, elig=rng.random(n1) < 0.5)                       # the mask regrows
    check_hnsw(g, o, w, q[:4], 10, 50)
    # destroy; a second index in the same process
    del g
    gc.collect()
    g2 = vdb.GpuHnswIndex(vdb.DistanceMetric(0), vdb.HnswParams.new(8, 64, 50), seed=9)
    g2.set_build(frontier_only)
    g2.build_batch((np.arange(n0, dtype=np.uint64), rows[:n0]))
    o2 = oracle.HnswOracle(0, m=8, ef_construction=64, ef_search=50, seed=9)
    for i in range(n0):
        o2.insert(i, rows[i])
    check_hnsw(g2, o2, None, q[:4], 5, 50)


# ------------------------------------------------------------------ meta table
def test_released_mask_is_regrown(vdb):
    T = vdb.MetaTable
    rng = np.random.default_rng(70)
    n = 100_000
    codes = rng.integers(-1, 4, size=n).astype(np.int32)
    present = np.ones(n, dtype=bool)
    present[rng.choice(n, size=40, replace=False)] = False
    table = T(0)
    table.set_codes(0, 0, codes)
    edges = np.diff(np.concatenate([[0], present.view(np.int8), [0]]))
    for a, e in zip(np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)):         # runs of present ids
        table.set_present(int(a), int(e - a), True)
    prog = [(T.EQ, 0, 2)]
    small = table.compile(prog, 1000)
    got, count = read_mask(small)
    want, wcount = fp.interpret([(fp.EQ, 0, 2)], {0: codes}, present, 1000)
    assert np.array_equal(got, want) and count == wcount
    small.release()
    big = table.compile(prog, n)                                                       # the released mask, regrown
    got, count = read_mask(big)
    want, wcount = fp.interpret([(fp.EQ, 0, 2)], {0: codes}, present, n)
    assert np.array_equal(got, want) and count == wcount and wcount > 0
    big.release()
    table.close()


# ------------------------------------------------------------------ one-process sharded handle
def test_sharded_query_and_pack_buffers_regrow(vdb):
    rng = np.random.default_rng(80)
    rows = rng.standard_normal((4001, 24)).astype(np.float32)
    q = rng.standard_normal((300, 24)).astype(np.float32)
    sh = vdb.GpuFlatIndex(vdb.DistanceMetric(1), devices=[0, 0], keep_host_copy=False)
    sh.add_bulk(rows)
    check_flat(1, rows, None, sh, q[:4], 10)
    check_flat(1, rows, None, sh, q, 10, qsel=range(0, 300, 23))
    check_flat(1, rows, None, sh, q[:4], 10)
