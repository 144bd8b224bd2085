"""The SPLIT row layout (csrc/row_split.h, vdb_flat_set_split): rows split in place into their bf16 piece and their low halves, the
screening tier's filter pass and re-ranks reading them as they lie, every other reader converting back first.

Nothing a caller can see may depend on the layout: every comparison here is bit for bit (ids, counts, the bit patterns of the
distances) against an index that never converts (mode 0) and, on two queries per case, against the CPU oracle."""
import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu

N = 65536 + 37                                     # the screening tier's minimum and a ragged last tile
F32, SPLIT = 0, 1


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


def make_pair(vdb, metric, rows, ids=None):
    """(an index that never converts, one that converts before the next eligible search) over the same rows"""
    out = []
    for mode in (0, 2):
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
        ix.set_split(mode)
        ix.add_bulk(rows, ids=ids)
        out.append(ix)
    return out


def check_oracle(metric, rows, q, k, res, qsel):
    gi, gd, gc = res
    for b in qsel:
        oi, od = oracle.flat_search(metric, rows, q[b], k)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), (b, gi[b, :gc[b]], oi)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc[b]], od)


_DATA = {}


def data(d):
    """rows and 300 queries of dimension d, made once"""
    if d not in _DATA:
        rng = np.random.default_rng(1000 + d)
        _DATA[d] = (rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((300, d)).astype(np.float32))
    return _DATA[d]


_PAIRS = {}


def pair(vdb, metric, d):
    if (metric, d) not in _PAIRS:
        _PAIRS[(metric, d)] = make_pair(vdb, metric, data(d)[0])
    return _PAIRS[(metric, d)]


# ------------------------------------------------------------------ round trip
@pytest.mark.parametrize("n,d", [(N, 64), (65536, 192)])
def test_forward_and_back_leaves_every_byte(vdb, n, d):
    rng = np.random.default_rng(n + d)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    bits = rows.view(np.uint32)
    bits[::7, 0] = (bits[::7, 0] & 0xffff0000) | 0x8000           # ties, ...
    bits[::11, 1] |= 0xffff                                       # ... full low halves, ...
    rows[3] = 0.0
    rows[5, :] = np.float32(1e-42)                                # ... zeros and denormals
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    ix.set_split(2)
    ix.add_bulk(rows)
    q = rng.standard_normal((4, d)).astype(np.float32)
    ix.search_batch_arrays(q, 5)                                  # converts forward first
    assert ix.layout() == (SPLIT, 1)
    got = np.empty_like(rows)
    for r in range(n):
        got[r] = ix.get_vector(r).as_slice()
        if r == 0:
            assert ix.layout() == (F32, 2)                        # the first read converted back, the others find f32 rows
    assert ix.layout() == (F32, 2)
    assert np.array_equal(got.view(np.uint32), rows.view(np.uint32))


# ------------------------------------------------------------------ search parity
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("B", [1, 37, 256, 300])
@pytest.mark.parametrize("d", [64, 192, 768])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_search_parity_with_f32_rows_and_the_oracle(vdb, metric, d, B, k):
    rows, queries = data(d)
    q = queries[:B]
    a, b = pair(vdb, metric, d)
    ra = a.search_batch_arrays(q, k)
    sa = a.last_stats()
    rb = b.search_batch_arrays(q, k)
    sb = b.last_stats()
    assert a.layout()[0] == F32
    if b.layout()[0] != SPLIT:                                    # a batch above 256 queries does not convert; the next small one does
        assert B > 256
        b.search_batch_arrays(q[:1], k)
        assert b.layout()[0] == SPLIT
        rb = b.search_batch_arrays(q, k)
        sb = b.last_stats()
        assert b.layout()[0] == SPLIT
    assert sa["bf16_screen"] == 1 and sb["bf16_screen"] == 1
    assert same(ra, rb), (metric, d, B, k)
    check_oracle(metric, rows, q, k, rb, sorted({0, B - 1}))


# ------------------------------------------------------------------ ties: every element exactly between two bf16 values
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ties_round_the_other_way_and_change_nothing(vdb, metric):
    d = 64
    rng = np.random.default_rng(55 + metric)
    rows = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((37, d)).astype(np.float32)
    for m in (rows, q):
        b = m.view(np.uint32)
        b[...] = (b & np.uint32(0xffff0000)) | np.uint32(0x8000)
    a, b = make_pair(vdb, metric, rows)
    for k in (1, 10):
        ra, rb = a.search_batch_arrays(q, k), b.search_batch_arrays(q, k)
        st = b.last_stats()
        assert b.layout()[0] == SPLIT
        assert same(ra, rb)
        assert st["bf16_screen"] == 1 and st["mfma_queries"] + st["exact_queries"] == len(q), st   # certified or handed on, never dropped
        check_oracle(metric, rows, q, k, rb, range(0, len(q), 6))


# ------------------------------------------------------------------ non-finite elements keep the f32-row behaviour
@pytest.mark.parametrize("bad", [0x7fc00000, 0xffffffff, 0x7f800000, 0xff800000])
def test_non_finite_rows_stay_f32(vdb, bad):
    d = 64
    rng = np.random.default_rng(bad & 0xffff)
    rows = rng.standard_normal((N, d)).astype(np.float32)
    rows.view(np.uint32)[N // 2, 3] = bad
    q = rng.standard_normal((5, d)).astype(np.float32)
    a, b = make_pair(vdb, 0, rows)

    def run(ix):
        try:
            return ("ok",) + tuple(ix.search_batch_arrays(q, 10))
        except Exception as e:                                    # a NaN distance fails the search, as the reference panics
            return ("error", type(e).__name__, str(e))

    ra, rb = run(a), run(b)
    assert b.layout() == (F32, 2)                                 # forward, found out, straight back
    assert ra[0] == rb[0]
    if ra[0] == "ok":
        assert same(ra[1:], rb[1:])
    else:
        assert ra[1:] == rb[1:]
    rb2 = run(b)                                                  # and it is not tried again until the rows change
    assert b.layout() == (F32, 2) and rb2[0] == rb[0]
    b.remove(N // 2)
    b.compact()
    a.remove(N // 2)
    ra3, rb3 = run(a), run(b)
    assert b.layout()[1] > 2                                      # the rows changed: the layout is tried again
    assert ra3[0] == "ok" and rb3[0] == "ok" and same(ra3[1:], rb3[1:])


# ------------------------------------------------------------------ every other reader converts back
def test_other_readers_convert_back(vdb):
    d = 64
    rows, queries = data(d)
    q = queries[:9]
    a, b = make_pair(vdb, 0, rows)
    # adaptive, with a run of 3: a reader that converts back and then searches (by id, forced exact) must leave F32 rows behind,
    # which mode 2 -- convert before the next eligible search -- would hide
    b.set_split(1)
    b.debug_set_split_after(3)

    def to_split():
        b.set_tiers(0)
        a.set_tiers(0)
        for _ in range(4):
            b.search_batch_arrays(q, 10)
        assert b.layout()[0] == SPLIT

    to_split()
    assert np.array_equal(np.asarray(b.get_vector(123).as_slice(), dtype=np.float32).view(np.uint32), rows[123].view(np.uint32))
    assert b.layout()[0] == F32

    to_split()
    ids = np.array([5, 70, 65000, N - 1], dtype=np.uint64)
    assert same(a.search_batch_by_id(ids, 10), b.search_batch_by_id(ids, 10))
    assert b.layout()[0] == F32

    to_split()
    ra = a.search_batch_arrays(q, 10)
    radius = float(ra[1][0, 5])
    assert same(a.range_search_batch(q, radius, 64), b.range_search_batch(q, radius, 64))
    assert b.layout()[0] == F32

    to_split()
    for ix in (a, b):
        ix.set_tiers(vdb.GpuFlatIndex.TIERS_FORCE_EXACT)
    assert same(a.search_batch_arrays(q, 10), b.search_batch_arrays(q, 10))
    assert b.layout()[0] == F32

    to_split()
    extra = np.random.default_rng(3).standard_normal((5, d)).astype(np.float32)
    for ix in (a, b):
        ix.add_bulk(extra, first_id=10 ** 6)
        ix.flush()
    assert b.layout()[0] == F32
    qa = np.concatenate([q, extra[:2]])
    ra, rb = a.search_batch_arrays(qa, 10), b.search_batch_arrays(qa, 10)
    assert same(ra, rb)
    assert rb[0][len(q), 0] == 10 ** 6                            # the appended row is found, at distance 0

    to_split()
    for ix in (a, b):
        for i in range(100, 130):                              # (still at least 65536 rows: the screening tier)
            ix.remove(i)
        ix.compact()
    assert b.layout()[0] == F32
    for _ in range(4):
        rb = b.search_batch_arrays(qa, 10)
    ra = a.search_batch_arrays(qa, 10)
    assert b.layout()[0] == SPLIT and same(ra, rb)
    live = np.ones(N + 5, dtype=bool)
    live[100:130] = False
    allrows = np.concatenate([rows, extra])
    allids = np.concatenate([np.arange(N, dtype=np.uint64), np.arange(5, dtype=np.uint64) + np.uint64(10 ** 6)])
    for bq in (0, len(qa) - 1):
        oi, od = oracle.flat_search(0, allrows[live], qa[bq], 10, ids=allids[live])
        assert np.array_equal(rb[0][bq], oi) and np.array_equal(rb[1][bq].view(np.uint32), od.view(np.uint32))


# ------------------------------------------------------------------ the adaptive rule
def test_adaptive_rule_counts_resets_and_waits(vdb):
    import torch
    d = 64
    rows, queries = data(d)
    q = queries[:8]
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    ix.add_bulk(rows)                                             # mode 1 is the default
    ix.debug_set_split_after(3)
    ref = ix.search_batch_arrays(q, 10)
    for _ in range(2):
        assert same(ix.search_batch_arrays(q, 10), ref)
    assert ix.layout() == (F32, 0)                                # three searches counted
    assert same(ix.search_batch_arrays(q, 10), ref)
    assert ix.layout() == (SPLIT, 1)                              # ... the next one converted first
    ix.get_vector(0)                                              # one f32 reader: back, and the count starts again
    assert ix.layout() == (F32, 2)
    for _ in range(3):
        assert same(ix.search_batch_arrays(q, 10), ref)
    assert ix.layout() == (F32, 2)
    ix.get_vector(1)                                              # an f32 reader in the middle of a run resets it too
    for _ in range(2):
        ix.search_batch_arrays(q, 10)
    assert ix.layout() == (F32, 2)
    # with a search in flight nothing converts: the submitted search reads the rows as they are
    dq = torch.from_numpy(q).cuda()
    outs = [(torch.zeros((8, 10), dtype=torch.int64, device="cuda"), torch.zeros((8, 10), dtype=torch.float32, device="cuda"),
             torch.zeros(8, dtype=torch.int32, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = ix.search_batch_device_submit(dq.data_ptr(), 8, d, 10, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr())   # the third of the run
    t1 = ix.search_batch_device_submit(dq.data_ptr(), 8, d, 10, outs[1][0].data_ptr(), outs[1][1].data_ptr(), outs[1][2].data_ptr())
    assert ix.layout() == (F32, 2)                                # the run is long enough, but the first search is in flight
    ix.search_batch_device_wait(t0)
    ix.search_batch_device_wait(t1)
    assert ix.layout() == (F32, 2)
    for o in outs:
        assert np.array_equal(o[0].cpu().numpy().view(np.uint64), ref[0]) and np.array_equal(o[1].cpu().numpy().view(np.uint32), ref[1].view(np.uint32))
    assert same(ix.search_batch_arrays(q, 10), ref)               # nothing in flight any more
    assert ix.layout() == (SPLIT, 3)
    ix.set_split(0)                                               # mode 0: never again once it is back
    ix.get_vector(2)
    for _ in range(5):
        ix.search_batch_arrays(q, 10)
    assert ix.layout() == (F32, 4)
