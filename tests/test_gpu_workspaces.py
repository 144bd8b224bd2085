"""The two search workspaces of a handle (csrc/vdb_index.h: Workspace, idle_workspace, other_workspace): which one an entry
point takes, what it may borrow from the other, and what is refused while tickets are out.  The entry points pass the workspace
down explicitly; these sequences are the ones the in-flight tests of test_gpu_parity.py / test_gpu_split_paths.py do not pin.
One index of 66,000 x 64 rows under Cosine (above the screening tier's minimum, row stride a multiple of 64), k = 10; every
result is compared with the oracle bit for bit: ids, order, distance bits, counts."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

COSINE = 1
N, D, K, NQ_BIG, NQ_TICKET = 66_000, 64, 10, 520, 64


class Data:
    def __init__(self):
        rng = np.random.default_rng(20)
        self.rows = rng.standard_normal((N, D)).astype(np.float32)
        self.q = rng.standard_normal((NQ_BIG, D)).astype(np.float32)
        self.ids = np.zeros((NQ_BIG, K), dtype=np.uint64)
        self.dists = np.zeros((NQ_BIG, K), dtype=np.float32)
        for b in range(NQ_BIG):                                    # the reference, once
            self.ids[b], self.dists[b] = oracle.flat_search(COSINE, self.rows, self.q[b], K)


@pytest.fixture(scope="module")
def data():
    return Data()


def make_index(vdb, data):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(COSINE), keep_host_copy=False)
    ix.add_bulk(data.rows)
    return ix


@pytest.fixture(scope="module")
def ix(vdb, data):
    return make_index(vdb, data)


class DeviceBatch:
    """queries [lo, hi) of the data on the device with output buffers; check() compares them with the oracle"""
    def __init__(self, data, lo, hi):
        import torch
        dev = torch.device("cuda", 0)
        self.data, self.lo, self.hi, self.nq = data, lo, hi, hi - lo
        self.q = torch.from_numpy(data.q[lo:hi]).to(dev)
        self.ids = torch.zeros((self.nq, K), dtype=torch.int64, device=dev)
        self.dists = torch.zeros((self.nq, K), dtype=torch.float32, device=dev)
        self.counts = torch.zeros((self.nq,), dtype=torch.int32, device=dev)

    def args(self, dim=D):
        return (self.q.data_ptr(), self.nq, dim, K, self.ids.data_ptr(), self.dists.data_ptr(), self.counts.data_ptr())

    def arrays(self):
        import torch
        torch.cuda.synchronize()
        return self.ids.cpu().numpy().view(np.uint64), self.dists.cpu().numpy(), self.counts.cpu().numpy()

    def check(self, what):
        check(self.arrays(), self.data, self.lo, self.hi, what)


def check(got, data, lo, hi, what):
    ids, dists, counts = got
    assert np.all(np.asarray(counts) == K), what
    assert np.array_equal(ids, data.ids[lo:hi]), what
    assert np.array_equal(dists.view(np.uint32), data.dists[lo:hi].view(np.uint32)), what


def test_a_large_synchronous_search_beside_a_ticket(vdb, data, ix):
    """A ticket of 64 queries is out; a synchronous search of 520 takes the other workspace and may not alternate its passes
    into the ticket's.  Both results are the oracle's."""
    small, big = DeviceBatch(data, 0, NQ_TICKET), DeviceBatch(data, 0, NQ_BIG)
    t = ix.search_batch_device_submit(*small.args())
    try:
        ix.search_batch_device(*big.args())
        big.check("synchronous, beside the ticket")
    finally:
        ix.search_batch_device_wait(t)
    small.check("the ticket")
    big.check("synchronous, after the wait")


def test_two_tickets_waited_for_in_reverse_order(vdb, data, ix):
    a, b, c = DeviceBatch(data, 0, NQ_TICKET), DeviceBatch(data, 100, 100 + NQ_TICKET), DeviceBatch(data, 200, 264)
    t0 = ix.search_batch_device_submit(*a.args())
    t1 = ix.search_batch_device_submit(*b.args())
    try:
        assert (t0, t1) == (0, 1)
        with pytest.raises(vdb.IndexError_, match="two searches are already in flight on this handle"):
            ix.search_batch_device_submit(*c.args())
        with pytest.raises(vdb.IndexError_, match="two submitted searches are in flight on this handle: wait for one first"):
            ix.search_batch_device(*c.args())
    finally:
        ix.search_batch_device_wait(t1)
        ix.search_batch_device_wait(t0)
    a.check("ticket 0")
    b.check("ticket 1")
    ix.search_batch_device(*c.args())
    c.check("synchronous, afterwards")


def test_a_failing_submit_beside_a_ticket(vdb, data):
    """The second submit passes its argument checks and fails in the search (a query dimension the store does not have): the
    outstanding ticket is untouched, the next searches are right, the handle takes writes again after the wait."""
    ix = make_index(vdb, data)                                     # (its own handle: it adds a row)
    a, bad = DeviceBatch(data, 0, NQ_TICKET), DeviceBatch(data, 64, 128)
    t = ix.search_batch_device_submit(*a.args())
    try:
        with pytest.raises(vdb.DimensionMismatch):
            ix.search_batch_device_submit(*bad.args(dim=D // 2))
    finally:
        ix.search_batch_device_wait(t)
    a.check("the ticket")
    check(ix.search_batch_arrays(data.q[:NQ_TICKET], K), data, 0, NQ_TICKET, "host-pointer search after the wait")
    t = ix.search_batch_device_submit(*bad.args())                 # the slot the failed submit had is free
    ix.search_batch_device_wait(t)
    bad.check("a ticket after the failed submit")
    ix.add(10**9, vdb.Vector(data.rows[0]))                        # writes are accepted again
    assert ix.len() == N + 1


def test_wide_and_narrow_passes_of_a_large_batch(vdb, data, ix):
    """520 queries: two passes of the wide filter kernel, or three 256-query passes alternating between the workspaces with all
    thresholds computed first.  The same bits either way."""
    got = {}
    try:
        for wide in (True, False):
            ix.set_wide(wide)
            b = DeviceBatch(data, 0, NQ_BIG)
            ix.search_batch_device(*b.args())
            b.check("wide" if wide else "narrow")
            got[wide] = b.arrays()
            st = ix.last_stats()
            assert st["bf16_screen"] == 1 and st["mfma_queries"] + st["exact_queries"] == NQ_BIG, st
    finally:
        ix.set_wide(True)
    for x, y in zip(got[True], got[False]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_host_pointer_calls_are_refused_beside_a_ticket(vdb, data, ix):
    a = DeviceBatch(data, 0, NQ_TICKET)
    q = data.q[:8]
    radii = data.dists[:8, K - 1].copy()                           # the k-th distance: the K nearest rows lie within it
    none = np.full(8, ix.GROUP_NONE, dtype=np.uint32)
    calls = {
        "search_batch_arrays": lambda: ix.search_batch_arrays(q, K),
        "range_search_batch": lambda: ix.range_search_batch(q, radii, K)[:3],
        "search_batch_grouped": lambda: ix.search_batch_grouped(q, K, none),
    }
    t = ix.search_batch_device_submit(*a.args())
    try:
        for name, call in calls.items():
            with pytest.raises(vdb.IndexError_, match="a submitted search is still in flight on this handle: wait for it first"):
                call()
    finally:
        ix.search_batch_device_wait(t)
    a.check("the ticket")
    for name, call in calls.items():
        check(call(), data, 0, 8, name + " after the wait")


def test_begin_finish_with_a_forced_tier(vdb, data, ix):
    b = DeviceBatch(data, 0, NQ_TICKET)
    ix.set_tiers(ix.TIERS_FORCE_F32)
    try:
        ix.search_batch_device_begin(*b.args())
        changed = ix.search_batch_device_finish()
    finally:
        ix.set_tiers(0)
    assert changed is True
    st = ix.last_stats()
    assert st["bf16_screen"] == 1 and st["f32_tier_queries"] == NQ_TICKET, st
    b.check("begin / finish, every query handed to the f32 tier")
