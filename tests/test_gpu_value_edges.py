"""Distances at the edges of f32 -- +-inf inside the returned top-k, -0.0, subnormals, the Cosine denominator and its clamp,
hidden NaN / zero-norm rows -- through every path that computes or orders by one.  The families are tests/value_families.py;
tests/test_value_edges_cpu.py proves what the oracle's answer holds for each at the shapes used here.

Every comparison is on ids, counts and distance BITS: the first path of a test against oracle.flat_search on a fixed subset of
queries, every other path against the first path's arrays by same().  Where the oracle errors the engine must raise the same
class on every path, with the same message.  No tolerance anywhere.  Tier counters are asserted only as far as they say which
tier ran (flags, or counts that are the batch size by construction); where a family pushes queries down the tiers the
counters are carried in the assertion message instead."""
import ctypes

import numpy as np
import pytest

import oracle
import value_families as vf
from conftest import load_package

pytestmark = pytest.mark.gpu

_IX = {}
_ORACLE = {}
ERRORS = {"NanDistance": "NaN distance", "InvalidVector": "Cannot compute cosine distance with zero vector"}


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    yield v
    _IX.clear()
    _ORACLE.clear()


def same(a, b):
    return np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def index_for(vdb, family, metric, n, d, nq, hide=True, tombstones=True, cache=True, **kw):
    """(index, rows, queries) of one family: ids are the row numbers, dead_rows(n, hide) are tombstoned."""
    key = (family, metric, n, d, nq, hide, tombstones, repr(sorted(kw.items())))
    rows, q = vf.make(family, n, d, nq, metric)
    if key in _IX:
        return _IX[key], rows, q
    shadow = kw.pop("shadow", False)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    if shadow:
        ix.set_shadow(True)
    ix.add_bulk(rows)
    if tombstones:
        for r in vf.dead_rows(n, hide):
            ix.remove(int(r))
    if cache:
        if len(_IX) > 6:
            _IX.pop(next(iter(_IX)))
        _IX[key] = ix
    return ix, rows, q


def oracle_rows(family, metric, n, d, nq, k, b, live, tag):
    key = (family, metric, n, d, nq, k, b, tag)
    if key not in _ORACLE:
        rows, q = vf.make(family, n, d, nq, metric)
        _ORACLE[key] = oracle.flat_search(metric, rows, q[b], k, live=live)
    return _ORACLE[key]


def check_oracle(res, family, metric, n, d, nq, k, live, tag="plain", what=None):
    gi, gd, gc = res
    for b in vf.checked_queries(nq):
        oi, od = oracle_rows(family, metric, n, d, nq, k, b, live, tag)
        msg = (family, metric, (n, d, nq, k), tag, b, what)
        assert gc[b] == len(oi), msg + (int(gc[b]), len(oi))
        assert np.array_equal(gi[b, :len(oi)], oi), msg + (gi[b, :len(oi)], oi)
        assert np.array_equal(gd[b, :len(oi)].view(np.uint32), od.view(np.uint32)), msg + (gd[b, :len(oi)], od)


def expect_error(vdb, family, call, first=None):
    """The oracle errors (tests/test_value_edges_cpu.py::claim_hidden_error): the same class, and one message on every path."""
    cls = getattr(vdb, vf.FAMILIES[family][2])
    with pytest.raises(cls) as e:
        call()
    assert ERRORS[vf.FAMILIES[family][2]] in str(e.value) and str(e.value)
    assert first is None or str(e.value) == first, (str(e.value), first)
    return str(e.value)


def with_tiers(ix, flags, call):
    ix.set_tiers(flags)
    try:
        return call()
    finally:
        ix.set_tiers(0)


PLAIN = {"tame", "nan_hidden", "cos_den_zero"}              # families whose hidden-row index behaves like gaussian data on every tier
# Counters pinned below for these families were observed on an MI355X on top of commit 05ee9ef (every metric, every shape):
#   20,000 rows, default / set_screen(0) / FORCE_RETHRESHOLD / FORCE_F32 (the last two change nothing below the screening floor):
#       tame: mfma_queries = nq, exact_queries = 0; nan_hidden under Euclid and Dot: mfma_queries = 0, exact_queries = uncertified = nq
#       (the tombstoned NaN row is still in the index maxima); always f32_tier_queries = rethreshold_queries = 0
#   65,536 rows (24 and 300 queries) and large k: default mfma_queries = nq, exact_queries = pool_overflows = rethreshold_queries = 0;
#       FORCE_RETHRESHOLD rethreshold_queries = nq; FORCE_F32 f32_tier_queries = nq; FORCE_EXACT exact_queries = nq


# ------------------------------------------------------------------ the direct exact scan of small indexes
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_direct_path(vdb, family, metric):
    n, d, nq, ks = vf.SHAPES["direct"]
    ix, rows, q = index_for(vdb, family, metric, n, d, nq)
    live = vf.live_bytes(n)
    for k in ks:
        res = ix.search_batch_arrays(q, k)
        st = ix.last_stats()
        assert st["exact_queries"] == nq and st["bf16_screen"] == 0, st
        check_oracle(res, family, metric, n, d, nq, k, live, what=st)
        other = with_tiers(ix, ix.TIERS_NO_DIRECT, lambda: ix.search_batch_arrays(q, k))
        assert same(res, other), (family, metric, k, ix.last_stats())
    if vf.FAMILIES[family][2]:
        bad, _, _ = index_for(vdb, family, metric, n, d, nq, hide=False)
        msg = expect_error(vdb, family, lambda: bad.search_batch_arrays(q, ks[0]))
        expect_error(vdb, family, lambda: with_tiers(bad, bad.TIERS_NO_DIRECT, lambda: bad.search_batch_arrays(q, ks[0])), msg)


# ------------------------------------------------------------------ the f32 tier, the ragged K stage, the forced exact scan
@pytest.mark.parametrize("shape", ["tiered", "ragged"])
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_tiers_below_the_screening_floor(vdb, family, metric, shape):
    """20,000 rows: above the direct path's limit, below the screening tier's floor, so set_screen(1) and set_screen(0) are
    both answered by the f32 MFMA tier and its re-rank; every knob of the list must leave the arrays as they are."""
    n, d, nq, (k,) = vf.SHAPES[shape]
    ix, rows, q = index_for(vdb, family, metric, n, d, nq)
    live = vf.live_bytes(n)
    res = ix.search_batch_arrays(q, k)
    st = ix.last_stats()
    assert st["bf16_screen"] == 0, st

    def f32_tier_answered(st):
        if family in PLAIN:
            assert st["mfma_queries"] + st["exact_queries"] == nq and st["f32_tier_queries"] == 0 and st["rethreshold_queries"] == 0, st
        if family == "tame":
            assert st["mfma_queries"] == nq and st["uncertified"] == 0, st
    f32_tier_answered(st)
    check_oracle(res, family, metric, n, d, nq, k, live, what=st)
    ix.set_screen(0)
    try:
        assert same(res, ix.search_batch_arrays(q, k)), (family, metric, ix.last_stats())
    finally:
        ix.set_screen(1)
    for flags in (ix.TIERS_FORCE_RETHRESHOLD, ix.TIERS_FORCE_F32, ix.TIERS_FORCE_EXACT):
        other = with_tiers(ix, flags, lambda: ix.search_batch_arrays(q, k))
        st2 = ix.last_stats()
        assert same(res, other), (family, metric, flags, st2)
        if flags == ix.TIERS_FORCE_EXACT:
            assert st2["exact_queries"] == nq, st2
        else:                                                      # no screening pass to re-threshold or to hand over from
            f32_tier_answered(st2)
    if vf.FAMILIES[family][2]:
        bad, _, _ = index_for(vdb, family, metric, n, d, nq, hide=False)
        msg = expect_error(vdb, family, lambda: bad.search_batch_arrays(q, k))
        expect_error(vdb, family, lambda: with_tiers(bad, bad.TIERS_FORCE_EXACT, lambda: bad.search_batch_arrays(q, k)), msg)


# ------------------------------------------------------------------ the screening tier and everything behind it
def _screen_variants(ix):
    def knob(on, off):
        def run(call):
            on()
            try:
                return call()
            finally:
                off()
        return run
    return {
        "screen0": knob(lambda: ix.set_screen(0), lambda: ix.set_screen(1)),
        "no_sample_cache": knob(lambda: ix.set_sample_cache(False), lambda: ix.set_sample_cache(True)),
        "force_rethreshold": lambda call: with_tiers(ix, ix.TIERS_FORCE_RETHRESHOLD, call),
        "force_f32": lambda call: with_tiers(ix, ix.TIERS_FORCE_F32, call),
        "force_exact": lambda call: with_tiers(ix, ix.TIERS_FORCE_EXACT, call),
    }


@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_screening_tier_and_forced_hand_overs(vdb, family, metric):
    n, d, nq, (k,) = vf.SHAPES["screened"]
    ix, rows, q = index_for(vdb, family, metric, n, d, nq)
    live = vf.live_bytes(n)
    res = ix.search_batch_arrays(q, k)
    st = ix.last_stats()
    assert st["bf16_screen"] == 1 and st["shadow_rows"] == 0, st
    if family in PLAIN:                                            # gaussian rows: the certified fast path answers
        assert st["mfma_queries"] == nq and st["exact_queries"] == 0 and st["pool_overflows"] == 0 and st["rethreshold_queries"] == 0, st
    check_oracle(res, family, metric, n, d, nq, k, live, what=st)
    for name, run in _screen_variants(ix).items():
        other = run(lambda: ix.search_batch_arrays(q, k))
        st2 = ix.last_stats()
        assert same(res, other), (family, metric, name, st2, st)
        assert st2["bf16_screen"] == (0 if name == "screen0" else 1), (name, st2)          # (a forced hand-over follows the screening pass)
        if name == "force_exact":
            assert st2["exact_queries"] == nq, st2
        if name == "force_f32" and family in PLAIN:
            assert st2["f32_tier_queries"] == nq, st2
        if name == "force_rethreshold" and family in PLAIN:
            assert st2["rethreshold_queries"] == nq and st2["exact_queries"] == 0, st2
    sh, _, _ = index_for(vdb, family, metric, n, d, nq, cache=False, shadow=True)
    other = sh.search_batch_arrays(q, k)
    st2 = sh.last_stats()
    assert st2["bf16_screen"] == 1 and st2["shadow_rows"] == 1, st2
    assert same(res, other), (family, metric, "shadow", st2, st)
    del sh
    if vf.FAMILIES[family][2]:
        bad, _, _ = index_for(vdb, family, metric, n, d, nq, hide=False, cache=False)
        msg = expect_error(vdb, family, lambda: bad.search_batch_arrays(q, k))
        if vf.FAMILIES[family][2] == "NanDistance":                # (a zero-norm row fails the search before any tier runs)
            assert bad.last_stats()["bf16_screen"] == 1             # the NaN was met behind the screening pass
        for name, run in _screen_variants(bad).items():
            expect_error(vdb, family, lambda: run(lambda: bad.search_batch_arrays(q, k)), msg)


@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_wide_batches_on_the_screening_tier(vdb, family, metric):
    """300 queries: the 512-query kernel (set_wide(True), the default) and the 256-query passes."""
    n, d, nq, (k,) = vf.SHAPES["wide"]
    ix, rows, q = index_for(vdb, family, metric, n, d, nq, cache=False)
    live = vf.live_bytes(n)
    res = ix.search_batch_arrays(q, k)
    st = ix.last_stats()
    assert st["bf16_screen"] == 1, st
    check_oracle(res, family, metric, n, d, nq, k, live, what=st)
    ix.set_wide(False)
    other = ix.search_batch_arrays(q, k)
    st2 = ix.last_stats()
    assert st2["bf16_screen"] == 1 and same(res, other), (family, metric, st2, st)
    if family in PLAIN:
        assert st["mfma_queries"] == nq and st2["mfma_queries"] == nq and st["exact_queries"] == 0 and st2["exact_queries"] == 0, (st, st2)
    if vf.FAMILIES[family][2]:
        for r in vf.dead_rows(n):                                  # the hidden row comes back under its id: alive and eligible again
            if r == vf.HIDDEN(n):
                ix.add(int(r), vdb.Vector(rows[r]))
        msg = expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k))
        ix.set_wide(True)
        expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k), msg)


# ------------------------------------------------------------------ large k
LARGE_K_CASES = [c for c in vf.CASES if c[0] in ("inf_tail", "overflow", "bf16_edge", "subnormal", "nan_hidden", "cos_den_zero", "tame")]


@pytest.mark.parametrize("family,metric", LARGE_K_CASES, ids=["%s-m%d" % c for c in LARGE_K_CASES])
def test_large_k(vdb, family, metric):
    n, d, nq, (k,) = vf.large_k_shape(vdb._ffi.lib().vdb_flat_large_k_min_rows(vf.K_LARGE))
    ix, rows, q = index_for(vdb, family, metric, n, d, nq, cache=False)
    live = vf.live_bytes(n)
    res = ix.search_batch_arrays(q, k)
    st = ix.last_stats()
    assert st["bf16_screen"] == 1, st
    check_oracle(res, family, metric, n, d, nq, k, live, what=st)
    other = with_tiers(ix, ix.TIERS_FORCE_RETHRESHOLD, lambda: ix.search_batch_arrays(q, k))
    st2 = ix.last_stats()
    assert same(res, other), (family, metric, st2, st)
    if family in PLAIN:                                            # the large-k re-rank answered; forced, its re-threshold pass did
        assert st["mfma_queries"] == nq and st["exact_queries"] == 0 and st["rethreshold_queries"] == 0, st
        assert st2["rethreshold_queries"] == nq and st2["exact_queries"] == 0, st2
    if vf.FAMILIES[family][2]:
        ix.add(vf.HIDDEN(n), vdb.Vector(rows[vf.HIDDEN(n)]))
        msg = expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k))
        expect_error(vdb, family, lambda: with_tiers(ix, ix.TIERS_FORCE_RETHRESHOLD, lambda: ix.search_batch_arrays(q, k)), msg)


# ------------------------------------------------------------------ masked searches: the tiers over every row, the sparse-filter scan
@pytest.mark.parametrize("selectivity", [0.5, 0.01], ids=["half", "one_percent"])
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_masked_searches(vdb, family, metric, selectivity):
    """The error families' row is ALIVE here.  A NaN row that the mask excludes is never computed: the search succeeds, and
    fails under a mask that admits the row.  A zero-norm row under Cosine fails every search while it is alive, masked out or
    not -- the reference's filtered search computes every row before it filters (storage.rs search_with_filter; DESIGN.md
    sections 1 and 4.8) -- and the masked results equal the oracle's once the row is removed."""
    n, d, nq, (k,) = vf.SHAPES["tiered"]
    error = vf.FAMILIES[family][2]
    zero_norm = error == "InvalidVector"
    ix, rows, q = index_for(vdb, family, metric, n, d, nq, hide=not error, cache=not zero_norm)
    on, words = vf.id_mask(n, selectivity, 7)
    live = vf.live_bytes(n, hide=not error or zero_norm) & on
    tag = "mask%g" % selectivity
    if zero_norm:
        assert not on[vf.HIDDEN(n)]
        _, open_words = vf.id_mask(n, selectivity, 7, hide=False)
        msg = None
        for mode in (0, 1):
            ix.set_sparse_filter(mode)
            for w in (words, open_words):
                msg = expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k, id_mask=w, mask_bits=n), msg)
        ix.remove(vf.HIDDEN(n))
    ix.set_sparse_filter(0)
    res = ix.search_batch_arrays(q, k, id_mask=words, mask_bits=n)
    assert ix.sparse_stats()[0] == 0
    check_oracle(res, family, metric, n, d, nq, k, live, tag=tag, what=ix.last_stats())
    ix.set_sparse_filter(1)
    try:
        answered = ix.sparse_stats()[2]
        other = ix.search_batch_arrays(q, k, id_mask=words, mask_bits=n)
        sp = ix.sparse_stats()
        assert sp[0] == 1 and sp[2] == answered + 1, sp
        assert same(res, other), (family, metric, tag)
        if error and not zero_norm:
            _, open_words = vf.id_mask(n, selectivity, 7, hide=False)
            msg = expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k, id_mask=open_words, mask_bits=n))
            ix.set_sparse_filter(0)
            expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k, id_mask=open_words, mask_bits=n), msg)
    finally:
        ix.set_sparse_filter(0)


# ------------------------------------------------------------------ the device entry points
@pytest.mark.parametrize("metric", [vf.EUCLID, vf.DOT])
def test_device_entry_points_with_two_tickets_in_flight(vdb, metric):
    import torch
    n, d, nq, (k,) = vf.SHAPES["tiered"]
    ix, rows, q = index_for(vdb, "inf_tail", metric, n, d, nq)
    batches = [q, vf.make("tame", n, d, nq, metric)[1]]             # an inf_tail batch and a tame batch, one handle
    host = [ix.search_batch_arrays(b, k) for b in batches]
    check_oracle(host[0], "inf_tail", metric, n, d, nq, k, vf.live_bytes(n))
    dev = torch.device("cuda", 0)
    qs = [torch.from_numpy(b.copy()).to(dev) for b in batches]

    def outputs():
        return (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                torch.empty((nq,), dtype=torch.int32, device=dev))

    def arrays(o):
        return o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().astype(np.uintp)
    for i in range(2):
        o = outputs()
        ix.search_batch_device(qs[i].data_ptr(), nq, d, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        torch.cuda.synchronize()
        assert same(arrays(o), host[i]), (metric, i)
    outs = [outputs() for _ in range(2)]
    tickets = [ix.search_batch_device_submit(qs[i].data_ptr(), nq, d, k, outs[i][0].data_ptr(), outs[i][1].data_ptr(), outs[i][2].data_ptr())
               for i in range(2)]
    for t in tickets:
        ix.search_batch_device_wait(t)
    torch.cuda.synchronize()
    for i in range(2):
        assert same(arrays(outs[i]), host[i]), (metric, i)


# ------------------------------------------------------------------ the sharded handle
@pytest.mark.parametrize("metric", [vf.EUCLID, vf.DOT])
def test_sharded_handle_orders_the_infinite_tail_by_id_across_shards(vdb, metric):
    n, d, nq, (k,) = vf.SHAPES["tiered"]
    sh, rows, q = index_for(vdb, "inf_tail", metric, n, d, nq, cache=False, devices=[0, 0, 0])
    assert sh.shards() == 3
    live = vf.live_bytes(n)
    res = sh.search_batch_arrays(q, k)
    assert (res[2] == k).all()
    check_oracle(res, "inf_tail", metric, n, d, nq, k, live)
    for b in range(nq):                                             # the infinite tail: more than half the result, ascending ids from all over
        tail = res[0][b][np.isinf(res[1][b])].astype(np.int64)
        assert tail.size >= k - vf.F_FINITE and (np.diff(tail) > 0).all(), (b, res[0][b], res[1][b])
    plain, _, _ = index_for(vdb, "inf_tail", metric, n, d, nq)
    assert same(res, plain.search_batch_arrays(q, k))
    # fewer eligible rows than k, two in each shard: every part is short, the merged count is the number of eligible rows
    on, words = vf.short_mask(n)
    short = sh.search_batch_arrays(q, k, id_mask=words, mask_bits=n)
    elig = int((on & (live != 0)).sum())
    assert elig < k and (short[2] == elig).all()
    check_oracle(short, "inf_tail", metric, n, d, nq, k, live & on, tag="short")
    assert same(short, plain.search_batch_arrays(q, k, id_mask=words, mask_bits=n))


# ------------------------------------------------------------------ the merge kernels alone
@pytest.mark.parametrize("W,k", vf.MERGE_SHAPES)
def test_merge_kernels_order_special_values_as_the_oracle_compares_them(vdb, W, k):
    """-inf, -0.0, +0.0, subnormals and +inf in hand-built sorted parts, some short or empty.  The oracle's comparator (cmp_pair)
    finds -0.0 and +0.0 equal, so between them the id decides; the distance bits pass through unchanged."""
    import torch
    from vectordb_from_scratch_amd.sharded import merge_topk_hip
    B = 5
    ids, d, counts = vf.merge_parts(W, B, k, seed=W * k)
    dev = torch.device("cuda", 0)
    gi, gd, gc = merge_topk_hip(torch.from_numpy(ids.view(np.int64)).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(counts).to(dev), k)
    torch.cuda.synchronize()
    gi, gd, gc = gi.cpu().numpy().view(np.uint64), gd.cpu().numpy(), gc.cpu().numpy()
    nk = B * k                                                      # the packed layout: ids | dists | counts | status | pad
    words = B * (3 * k + 1) + 1
    words += words & 1
    packed = np.zeros((W, words), dtype=np.int32)
    for p in range(W):
        packed[p, :2 * nk] = ids[p].reshape(-1).view(np.int32)
        packed[p, 2 * nk:3 * nk] = d[p].reshape(-1).view(np.int32)
        packed[p, 3 * nk:3 * nk + B] = counts[p]
    pk = torch.from_numpy(packed).to(dev)
    oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    od = torch.empty((B, k), dtype=torch.float32, device=dev)
    oc = torch.empty((B,), dtype=torch.int32, device=dev)
    os_ = torch.zeros((1,), dtype=torch.int32, device=dev)
    rc = vdb._ffi.lib().vdb_merge_topk_packed_device(0, ctypes.c_void_p(pk.data_ptr()), W, words, B, k, ctypes.c_void_p(oi.data_ptr()),
                                                     ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(oc.data_ptr()),
                                                     ctypes.c_void_p(os_.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
    pi, pd, pc = oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy()
    for b in range(B):
        ii = np.concatenate([ids[p, b, :counts[p, b]] for p in range(W)])
        dd = np.concatenate([d[p, b, :counts[p, b]] for p in range(W)])
        o = vf.merge_order(ii, dd)[:k]
        for name, got_i, got_d, got_c in (("arrays", gi, gd, gc), ("packed", pi, pd, pc)):
            assert got_c[b] == len(o), (name, b, got_c[b], len(o))
            assert np.array_equal(got_i[b, :len(o)], ii[o]), (name, b, got_i[b, :len(o)], ii[o], dd[o])
            assert np.array_equal(got_d[b, :len(o)].view(np.uint32), dd[o].view(np.uint32)), (name, b)


# ------------------------------------------------------------------ vdb_flat_distances_batch
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_distances_batch_bits(vdb, family, metric):
    n, d, nq, _ = vf.SHAPES["direct"]
    error = vf.FAMILIES[family][2]
    ix, rows, q = index_for(vdb, family, metric, n, d, nq, tombstones=False)
    rng = np.random.default_rng(n + metric)
    with np.errstate(over="ignore", invalid="ignore"):
        extreme = np.argsort(np.abs(rows).max(1))[[0, 1, 2, -3, -2, -1]]          # the smallest and the largest rows
    hidden = vf.HIDDEN(n)
    lists = [np.unique(np.concatenate([np.arange(8), extreme, rng.integers(0, n, 40)])).astype(np.uint64) for _ in range(nq)]
    lists = [l[l != hidden] for l in lists]
    got = ix.distances_batch(q, lists)
    for b in range(nq):
        want = np.array([oracle.distance(metric, q[b], rows[int(r)]) for r in lists[b]], dtype=np.float32)
        assert not np.isnan(want).any()
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (family, metric, b, got[b], want)
    if error == "InvalidVector":                                   # the oracle's outcome for the pair whose row norm underflows to 0
        with pytest.raises(oracle.OracleError):
            oracle.distance(metric, q[0], rows[hidden])
        expect_error(vdb, family, lambda: ix.distances_batch(q[:1], [np.array([1, hidden], dtype=np.uint64)]))
    elif error:                                                    # vdbo_distance returns the NaN; so does the pair kernel
        assert np.isnan(oracle.distance(metric, q[0], rows[hidden]))
        out = ix.distances_batch(q[:1], [np.array([1, hidden], dtype=np.uint64)])[0]
        assert np.isnan(out[1]) and out[0].view(np.uint32) == oracle.distance(metric, q[0], rows[1]).view(np.uint32)


# ------------------------------------------------------------------ HNSW (stands alone)
@pytest.mark.parametrize("n,d,m,efc", [(300, 8, 4, 32), (1500, 48, 16, 100)])
@pytest.mark.parametrize("family,metric", vf.HNSW_CASES, ids=["%s-m%d" % c for c in vf.HNSW_CASES])
def test_hnsw_graph_and_walks_equal_the_cpu_restatement(vdb, family, metric, n, d, m, efc):
    """The graph built through the GPU-offloaded inserts, the device walk and the host traversal against oracle/hnsw_oracle.c.
    No family here yields a NaN, between a query and a row or between two rows: tests/test_value_edges_cpu.py folds every pair."""
    from test_gpu_hnsw import assert_same_graph, assert_same_results, build_pair
    rows, q = vf.make_hnsw(family, n, d, metric)
    g, o, ids = build_pair(vdb, metric, rows, m, efc, 32, seed=11 + metric)
    assert_same_graph(g, o, ids)
    assert_same_results(g, o, q, 10, 32)
    st = g.stats()
    assert st["device_queries"] == q.shape[0], st
    dev = g.search_batch_arrays(q, 10, 32)
    g.set_traversal(host_only=True, host_threads=2)
    try:
        host = g.search_batch_arrays(q, 10, 32)
        assert g.stats()["last_search_rounds"] > 0
    finally:
        g.set_traversal(host_only=False)
    assert same(dev, host), (family, metric, n)
