"""The re-threshold pass at large k (112 < k <= 1024: rerank_all_large_kernel behind a second filter pass) and
the switch that routes every query through it (VDB_TIERS_FORCE_RETHRESHOLD).  Every answer is compared bit for bit -- ids,
order, distance bits -- with the same search under VDB_TIERS_FORCE_EXACT, and for a few queries with the CPU oracle."""
import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu

TIMING = ("fused_kernel_ns", "host_enqueued_ns", "host_flags_ns", "host_total_ns")


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def counters(st):
    return {key: v for key, v in st.items() if key not in TIMING}


def check_oracle(metric, rows, q, k, res, qsel, ids=None, live=None):
    gi, gd, gc = res
    for b in qsel:
        kb = k[b] if not np.isscalar(k) else k
        oi, od = oracle.flat_search(metric, rows, q[b], kb, ids=ids, live=live)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), b
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), b


def make(vdb, metric, rows, ids=None, devices=None):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, devices=devices)
    ix.add_bulk(rows, ids=ids)
    return ix


def under(ix, flags, q, k, **kw):
    """(results, counters) of one search with the tier flags set."""
    ix.set_tiers(flags)
    try:
        res = ix.search_batch_arrays(q, k, **kw)
        return res, ix.last_stats()
    finally:
        ix.set_tiers(0)


def forced(ix, q, k, **kw):
    return under(ix, ix.TIERS_FORCE_RETHRESHOLD, q, k, **kw)


def exact(ix, q, k, **kw):
    return under(ix, ix.TIERS_FORCE_EXACT, q, k, **kw)[0]


def near_rows(rng, rows, B, noise=0.05):
    q = rows[rng.integers(0, rows.shape[0], B)] + rng.standard_normal((B, rows.shape[1])).astype(np.float32) * noise
    return np.ascontiguousarray(q, dtype=np.float32)


# ------------------------------------------------------------------ 1. the forced route, every metric
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_forced_route_answers_every_query(vdb, metric):
    """k = 113 and k = 10 on 74 000 rows.  k = 150 needs vdb_flat_large_k_min_rows(150) = 82 080 rows to be in the range at all,
    so it runs on 83 000 rows (the same first 74 000)."""
    rng = np.random.default_rng(400 + metric)
    d, B = 32, 12
    rows = rng.standard_normal((83_000, d)).astype(np.float32)
    q = near_rows(rng, rows[:74_000], B)
    for n, ks in ((74_000, (113, 10)), (83_000, (150,))):
        ix = make(vdb, metric, rows[:n])
        for k in ks:
            a, st = forced(ix, q, k)
            assert st["bf16_screen"] == 1 and st["rethreshold_queries"] == B, (k, st)
            assert st["exact_queries"] == 0 and st["f32_tier_queries"] == 0, (k, st)
            assert same(a, exact(ix, q, k)), k
            check_oracle(metric, rows[:n], q, k, a, [0, B - 1])


# ------------------------------------------------------------------ 2. sweep (512) and sort-area (1024) boundaries
@pytest.mark.parametrize("metric", [0, 2])
def test_sweep_and_sort_area_boundaries(vdb, metric):
    rng = np.random.default_rng(410 + metric)
    n, d, B = 292_000, 32, 6
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = near_rows(rng, rows, B)
    ix = make(vdb, metric, rows)
    for k in (511, 512, 513, 1023, 1024):
        a, st = forced(ix, q, k)
        assert st["bf16_screen"] == 1 and st["rethreshold_queries"] == B and st["exact_queries"] == 0, (k, st)
        assert same(a, exact(ix, q, k)), k
    check_oracle(metric, rows, q, 1024, a, [0, B - 1])
    # outside the range the flag changes nothing
    a, st = forced(ix, q, 1025)
    b = ix.search_batch_arrays(q, 1025)
    assert st["bf16_screen"] == 0 and st["rethreshold_queries"] == 0 and counters(st) == counters(ix.last_stats()), st
    assert same(a, b)


# ------------------------------------------------------------------ 3. K slices and the tail
@pytest.mark.parametrize("d", [1, 33, 1030])
def test_dimensions_across_the_k_slices(vdb, d):
    """d = 1030: a 512-candidate sweep needs several slices, and 1030 is no multiple of 4 * 64."""
    rng = np.random.default_rng(420 + d)
    n, B, k = 74_000, 4, 113
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = near_rows(rng, rows, B)
    for metric in (0, 1, 2):
        ix = make(vdb, metric, rows)
        a, st = forced(ix, q, k)
        print(d, metric, counters(st))
        assert st["bf16_screen"] == 1, st
        assert same(a, exact(ix, q, k)), metric
        if d > 1:                                                   # (d = 1: bf16 scores of scalars tie by the thousand, lists above 2048 keys)
            assert st["rethreshold_queries"] == B and st["exact_queries"] == 0, st
        check_oracle(metric, rows, q, k, a, [0, B - 1])


# ------------------------------------------------------------------ 4. the natural hand-over
def test_rethreshold_pass_answers_what_the_large_k_depth_limit_could_not(vdb):
    """1500 rows inside the bf16 error bound of each other, at random positions: the first pass (depth 1024 at k = 113) cannot
    certify, its k-th exact distance implies a score cut, the re-threshold pass re-ranks every key under it."""
    rng = np.random.default_rng(28)
    n, d, k = 120_000, 96, 113
    rows = rng.standard_normal((n, d)).astype(np.float32)
    centre = rng.standard_normal(d).astype(np.float32) * 2.0
    where = rng.choice(n, 1500, replace=False)
    rows[where] = centre + 1e-3 * rng.standard_normal((1500, d)).astype(np.float32)
    q = (centre + 1e-4 * rng.standard_normal((5, d))).astype(np.float32)
    for metric in (0, 1, 2):
        ix = make(vdb, metric, rows)
        a = ix.search_batch_arrays(q, k)
        st = ix.last_stats()
        print(metric, counters(st))
        assert same(a, exact(ix, q, k))
        assert st["bf16_screen"] == 1 and st["uncertified"] > 0, st
        assert st["rethreshold_queries"] == st["uncertified"] and st["exact_queries"] == 0, st
        check_oracle(metric, rows, q, k, a, [0, 4])


# ------------------------------------------------------------------ 5. a list that does not fit
def test_more_than_2048_keys_under_the_cut_go_to_the_exact_scan(vdb):
    rng = np.random.default_rng(430)
    d, B, k = 32, 6, 113
    base = rng.standard_normal((24, d)).astype(np.float32)
    rows = np.ascontiguousarray(np.tile(base, (5000, 1)))          # every row 5000 times: 5000 keys under any cut
    q = near_rows(rng, base, B)
    for metric in (0, 1, 2):
        ix = make(vdb, metric, rows)
        a, st = forced(ix, q, k)
        assert st["bf16_screen"] == 1 and st["rethreshold_queries"] == 0 and st["exact_queries"] == B, st
        assert same(a, exact(ix, q, k))
        check_oracle(metric, rows, q, k, a, [0, B - 1])             # ties come out ordered by id


# ------------------------------------------------------------------ 6. tombstones, id mask, the id space
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_tombstones_mask_ragged_ks_and_the_id_space(vdb, metric):
    rng = np.random.default_rng(440 + metric)
    n, d, B = 100_000, 64, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(np.arange(n, dtype=np.uint64) * 7 + 3)   # sparse, not monotone
    top, zero = 4321, 8765
    ids[top] = np.uint64(2**64 - 1)
    ids[zero] = np.uint64(0)
    ix = make(vdb, metric, rows, ids=ids)
    dead = rng.choice(np.setdiff1d(np.arange(n), [top, zero]), 8000, replace=False)
    for r in dead:
        ix.remove(int(ids[r]))
    live = np.ones(n, dtype=np.uint8)
    live[dead] = 0
    q = rng.standard_normal((B, d)).astype(np.float32)
    q[1] = rows[top] + 0.01 * rng.standard_normal(d).astype(np.float32)     # the row with id 2^64 - 1 is its nearest
    q[2] = rows[zero] + 0.01 * rng.standard_normal(d).astype(np.float32)
    ks = np.array([10, 150] * (B // 2), dtype=np.uintp)
    a, st = forced(ix, q, ks)
    assert st["bf16_screen"] == 1 and st["rethreshold_queries"] == B and st["exact_queries"] == 0, st
    assert same(a, exact(ix, q, ks))
    assert np.uint64(2**64 - 1) in a[0][1, :150] and np.uint64(0) in a[0][2, :10]
    check_oracle(metric, rows, q, ks, a, [0, 1, 2], ids=ids, live=live)
    mask_bits = 1 << 21
    mask = rng.integers(0, 2**64, mask_bits // 64, dtype=np.uint64)            # about half of the ids below 2^21
    a, st = forced(ix, q, ks, id_mask=mask, mask_bits=mask_bits)
    assert st["bf16_screen"] == 1 and st["rethreshold_queries"] == B and st["exact_queries"] == 0, st
    assert same(a, exact(ix, q, ks, id_mask=mask, mask_bits=mask_bits))
    bit = np.array([(i < mask_bits) and bool((int(mask[i // 64]) >> (i % 64)) & 1) for i in ids.tolist()], dtype=np.uint8)
    check_oracle(metric, rows, q, ks, a, [1, 3], ids=ids, live=live & bit)


# ------------------------------------------------------------------ 7. errors
def _outcome(fn):
    try:
        fn()
        return None
    except Exception as e:                                          # noqa: BLE001 -- the error class is what is compared
        return type(e).__name__


def test_forced_errors_match_the_unforced_and_small_k(vdb):
    rng = np.random.default_rng(450)
    rows = rng.random((100_000, 32), dtype=np.float32)
    q = rng.random((4, 32), dtype=np.float32)
    z = rows.copy()
    z[1234] = 0.0
    nanr = rows.copy()
    nanr[777] = np.nan
    for metric, data, want in ((1, z, "InvalidVector"), (0, nanr, None), (2, nanr, None), (1, nanr, None)):
        ix = make(vdb, metric, data)
        small = _outcome(lambda: ix.search_batch_arrays(q, 10))
        large = _outcome(lambda: ix.search_batch_arrays(q, 150))
        small_f = _outcome(lambda: forced(ix, q, 10))
        large_f = _outcome(lambda: forced(ix, q, 150))
        assert small == large == small_f == large_f, (metric, small, large, small_f, large_f)
        if want:
            assert large_f == want


# ------------------------------------------------------------------ 8. switches
def test_switches_around_the_forced_route(vdb):
    rng = np.random.default_rng(460)
    n, d, B, k = 83_000, 128, 16, 150
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = near_rows(rng, rows, B)
    ix = make(vdb, 0, rows)
    with pytest.raises(Exception):
        ix.set_tiers(32)                                            # VDB_ERR_INVALID_ARGUMENT: no such flag
    a, sa = forced(ix, q, k)
    sa = counters(sa)
    assert sa["bf16_screen"] == 1 and sa["rethreshold_queries"] == B and sa["exact_queries"] == 0, sa
    # the pass switched off wins over the forced route: the routing of NO_RETHRESHOLD alone
    b, sb = under(ix, ix.TIERS_NO_RETHRESHOLD | ix.TIERS_FORCE_RETHRESHOLD, q, k)
    c, sc = under(ix, ix.TIERS_NO_RETHRESHOLD, q, k)
    assert counters(sb) == counters(sc) and sb["rethreshold_queries"] == 0, (sb, sc)
    assert same(a, b) and same(a, c)
    # ignored together with FORCE_EXACT and FORCE_F32
    e, se = under(ix, ix.TIERS_FORCE_EXACT | ix.TIERS_FORCE_RETHRESHOLD, q, k)
    assert se["rethreshold_queries"] == 0 and se["exact_queries"] == B and same(a, e), se
    f, sf = under(ix, ix.TIERS_FORCE_F32 | ix.TIERS_FORCE_RETHRESHOLD, q, 10)
    assert sf["rethreshold_queries"] == 0 and sf["f32_tier_queries"] == B, sf
    assert same(f, exact(ix, q, 10))
    # shadow rows on, then the sample cache off: the same results and counters
    ix.set_shadow(True)
    g, sg = forced(ix, q, k)
    sg = counters(sg)
    assert sg.pop("shadow_rows") == 1 and sa.pop("shadow_rows") == 0
    ix.set_sample_cache(False)
    h, sh = forced(ix, q, k)
    sh = counters(sh)
    sh.pop("shadow_rows")
    assert sa == sg == sh, (sa, sg, sh)
    assert same(a, g) and same(a, h)


# ------------------------------------------------------------------ 9. a sharded handle
def test_sharded_handle_takes_the_forced_route_on_every_shard(vdb):
    rng = np.random.default_rng(470)
    n, d, B, k = 160_000, 32, 8, 113
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = near_rows(rng, rows, B)
    plain = make(vdb, 0, rows)
    sh = make(vdb, 0, rows, devices=[0, 0])                        # two shards of 80 000 rows, the peer-copy exchange
    a, st = forced(sh, q, k)
    assert st["bf16_screen"] >= 1 and st["rethreshold_queries"] == 2 * B and st["exact_queries"] == 0, st
    b, sp = forced(plain, q, k)
    assert sp["rethreshold_queries"] == B, sp
    assert same(a, b) and same(a, exact(plain, q, k))
    check_oracle(0, rows, q, k, a, [0, B - 1])
