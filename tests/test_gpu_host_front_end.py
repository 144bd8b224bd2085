"""The output shapes every host-pointer batch search shares (csrc/vdb_hostio.h copy_out), through the C entry points themselves
with poisoned output arrays: a caller's stride above the largest k, a per-query k that contains 0, and a k above the number of
stored rows -- for the plain search, by stored id, recommend, one row per group, grouped and range, on a plain handle and
(where the entry point serves one) on a two-shard handle.  The expectation is the SAME search through the package's wrapper,
whose arrays are exactly max(k) wide and which the other suites pin to the oracle bit for bit; nothing beyond a count may be
written.  64 rows x 8 dimensions, 3 queries."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, NQ, K = 64, 8, 3, 5
POISON_ID, POISON_D, POISON_C, POISON_N = 0xDEADBEEFDEADBEEF, 0x7FC0BEEF, -77, 12345
u64p, szp, fp, i32p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float, ctypes.c_int32, ctypes.c_uint32))

_rng = np.random.default_rng(16)
ROWS = _rng.random((N, D), dtype=np.float32)
Q = np.ascontiguousarray(_rng.random((NQ, D), dtype=np.float32))
QID = np.array([3, 17, 40], dtype=np.uint64)
POS, NEG = [[1, 2], [10], [20]], [[3], [11], []]
EX = np.array([1, 2, 3, 10, 11, 20], dtype=np.uint64)
OFFS = np.array([0, 3, 5, 6], dtype=np.uintp)
NPOS = np.array([2, 1, 1], dtype=np.uint32)
CODES = (np.arange(N) % 7).astype(np.int32)                       # 7 groups
GROUP_OF = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32)          # even ids | ids below 10 | no mask
MASKS = np.array([[0x5555555555555555], [0x3FF]], dtype=np.uint64)
_cache = {}


def handle(vdb, sharded):
    if sharded not in _cache:
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False, **({"devices": [0, 0]} if sharded else {}))
        ix.add_bulk(ROWS)
        _cache[sharded] = ix
    return _cache[sharded]


def table(vdb):
    if "table" not in _cache:
        t = vdb.MetaTable(0)
        t.set_codes(0, 0, CODES)
        t.set_present(0, N, True)
        _cache["table"] = t
    return _cache["table"]


def raw(vdb, ix, kind, ks, k, kstride):
    """the C entry point with poisoned outputs: ks an array (k unused) or None (k for every query) -> ids, dists, codes, counts"""
    L = vdb._ffi.lib()
    oi = np.full((NQ, kstride), POISON_ID, dtype=np.uint64)
    od = np.full((NQ, kstride), POISON_D, dtype=np.uint32).view(np.float32)
    ocode = np.full((NQ, kstride), POISON_C, dtype=np.int32)
    oc = np.full(NQ, POISON_N, dtype=np.uintp)
    ksp = None
    if ks is not None:
        ks = np.ascontiguousarray(ks, dtype=np.uintp)
        ksp = ks.ctypes.data_as(szp)
    out = (kstride, oi.ctypes.data_as(u64p), od.ctypes.data_as(fp))
    ocp, h, qp = oc.ctypes.data_as(szp), ix._h, Q.ctypes.data_as(fp)
    if kind == "plain":
        rc = L.vdb_flat_search_batch(h, qp, NQ, D, ksp, k, None, 0, *out, ocp)
    elif kind == "by_id":
        rc = L.vdb_flat_search_batch_by_id(h, QID.ctypes.data_as(u64p), NQ, ksp, k, None, 0, *out, ocp)
    elif kind == "recommend":
        rc = L.vdb_flat_recommend_batch(h, EX.ctypes.data_as(u64p), OFFS.ctypes.data_as(szp), NPOS.ctypes.data_as(u32p), NQ, ksp, k, None, 0, *out, ocp)
    elif kind == "distinct":
        rc = L.vdb_flat_search_batch_distinct(h, qp, NQ, D, ksp, k, table(vdb)._t, 0, None, 0, *out, ocode.ctypes.data_as(i32p), ocp)
    else:
        rc = L.vdb_flat_search_batch_grouped(h, qp, NQ, D, ksp, k, MASKS.ctypes.data_as(u64p), 2, 64, GROUP_OF.ctypes.data_as(u32p), *out, ocp)
    assert rc == 0, vdb._ffi.last_error()
    return oi, od, ocode, oc


def wrapped(vdb, ix, kind, k):
    """the same search with one k through the package: arrays exactly k wide -> ids, dists, codes or None, counts"""
    if kind == "plain":
        i, d, c = ix.search_batch_arrays(Q, k)
    elif kind == "by_id":
        i, d, c = ix.search_batch_by_id(QID, k)
    elif kind == "recommend":
        i, d, c = ix.recommend_batch(POS, NEG, k)
    elif kind == "distinct":
        i, d, code, c = ix.search_batch_distinct(Q, k, table(vdb), 0)
        return i, d, code, c
    else:
        i, d, c = ix.search_batch_grouped(Q, k, GROUP_OF, id_masks=MASKS, mask_bits=64)
    return i, d, None, c


def check(got, want, ks, what):
    """got: the first min(ks[b], want's count) entries of want's list b, and nothing written beyond them"""
    oi, od, ocode, oc = got
    wi, wd, wcode, wc = want
    for b in range(NQ):
        c = min(int(wc[b]), int(ks[b]))
        assert int(oc[b]) == c, (what, b, oc.tolist(), wc.tolist())
        assert np.array_equal(oi[b, :c], wi[b, :c]) and np.array_equal(od[b, :c].view(np.uint32), wd[b, :c].view(np.uint32)), (what, b)
        assert (oi[b, c:] == POISON_ID).all() and (od[b, c:].view(np.uint32) == POISON_D).all(), (what, b)
        if wcode is not None:
            assert np.array_equal(ocode[b, :c], wcode[b, :c]) and (ocode[b, c:] == POISON_C).all(), (what, b)
        else:
            assert (ocode == POISON_C).all()


# the rows a k above the store returns, per query: everything eligible
ALL = {"plain": [N] * 3, "by_id": [N - 1] * 3, "recommend": [N - 3, N - 2, N - 1], "distinct": [7] * 3, "grouped": [32, 10, N]}
CASES = [(kind, sharded) for kind in ("plain", "by_id", "recommend", "distinct", "grouped") for sharded in (False, True)
         if not (kind == "grouped" and sharded)]                  # (a sharded handle refuses the grouped call)


@pytest.mark.parametrize("kind,sharded", CASES)
def test_stride_above_k_zero_k_and_k_above_the_store(vdb, kind, sharded):
    ix = handle(vdb, sharded)
    want = wrapped(vdb, ix, kind, K)
    assert all(int(c) == K for c in want[3])
    # a stride above the largest k
    check(raw(vdb, ix, kind, None, K, K + 3), want, [K] * NQ, "kstride > k")
    # a per-query k with a 0 in it, and a stride above its largest
    ks = [0, K, 2]
    check(raw(vdb, ix, kind, ks, 999, K + 3), want, ks, "ks with 0")
    # k above the number of stored rows: every eligible row, once
    big = N + 36
    deep = wrapped(vdb, ix, kind, big)
    assert [int(c) for c in deep[3]] == ALL[kind]
    check(raw(vdb, ix, kind, None, big, big + 3), deep, [big] * NQ, "k > len")
    check(raw(vdb, ix, kind, [big, 1, 0], 0, big), deep, [big, 1, 0], "ks up to k > len")
    for b in range(NQ):                                           # the deep lists begin with the shallow ones
        assert np.array_equal(deep[0][b, :K], want[0][b, :K]) and np.array_equal(deep[1][b, :K].view(np.uint32), want[1][b, :K].view(np.uint32))


def test_range_max_results_above_the_store(vdb):
    """the range search's stride IS max_results: above the store every row comes back once, in the order of the plain search, and
    the slots beyond the count stay as the caller left them"""
    ix = handle(vdb, False)
    L = vdb._ffi.lib()
    mr = N + 36
    oi = np.full((NQ, mr), POISON_ID, dtype=np.uint64)
    od = np.full((NQ, mr), POISON_D, dtype=np.uint32).view(np.float32)
    oc = np.full(NQ, POISON_N, dtype=np.uintp)
    tot = np.full(NQ, POISON_N, dtype=np.uint64)
    rad = np.array([np.inf, np.inf, -1.0], dtype=np.float32)      # the last query: nothing within the radius
    rc = L.vdb_flat_range_search_batch(ix._h, Q.ctypes.data_as(fp), NQ, D, rad.ctypes.data_as(fp), ctypes.c_float(0.0), None, 0, mr,
                                       oi.ctypes.data_as(u64p), od.ctypes.data_as(fp), oc.ctypes.data_as(szp), tot.ctypes.data_as(u64p))
    assert rc == 0, vdb._ffi.last_error()
    wi, wd, wc = ix.search_batch_arrays(Q, N)
    assert oc.tolist() == [N, N, 0] and tot.tolist() == [N, N, 0]
    for b in range(NQ):
        c = int(oc[b])
        assert np.array_equal(oi[b, :c], wi[b, :c]) and np.array_equal(od[b, :c].view(np.uint32), wd[b, :c].view(np.uint32)), b
        assert (oi[b, c:] == POISON_ID).all() and (od[b, c:].view(np.uint32) == POISON_D).all(), b
