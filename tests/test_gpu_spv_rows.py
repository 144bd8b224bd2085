"""The row-major route of the sparse-vector index (vdb_spv_set_route, csrc/kernels_spv_rows.hip) against the CSR reference
(spv_data.search_csr): ids, order, distance bits, counts and the statistics, bit for bit, at the lane, tile, block and pass edges
of its kernels; the value, select-mask and lifecycle tests of the inverted route replayed on it; the automatic mode."""
import numpy as np
import pytest

import spv_data as S
import spv_lifecycle as L
import test_gpu_spv_select as SEL
import test_gpu_spv_values as V
from test_gpu_spv_lifecycle import GpuAdapter

pytestmark = pytest.mark.gpu
U32, F32, U64 = np.uint32, np.float32, np.uint64
BITS = 18000


class Routed:
    """the package, but every GpuSparseIndex it makes searches on the given route"""

    def __init__(self, vdb, mode):
        self._vdb, self._mode = vdb, mode

    def __getattr__(self, name):
        return getattr(self._vdb, name)

    def GpuSparseIndex(self, *a):
        ix = self._vdb.GpuSparseIndex(*a)
        ix.set_route(self._mode)
        return ix


@pytest.fixture(scope="module")
def corpus():
    ids, X, P = S.corpus()
    offsets, indices, values = S.csr_from_dense(X, P)
    C = (ids, offsets, indices, values, np.ones(ids.size, dtype=bool))
    return C, S.csc_view(offsets, indices)


def index_of(vdb, C, route):
    ix = vdb.GpuSparseIndex()
    ix.set_route(route)
    ix.add_csr(*C[:4])
    return ix


def q_of(dims, rng):
    dims = np.asarray(dims, dtype=U32)
    return dims, rng.standard_normal(dims.size).astype(F32)


def batch(seed, nq):
    """the long lists 7, 8, 9; the absent index 100; indices at and above vocab; row 20's explicit zero; an empty query; random ones"""
    rng = np.random.default_rng(seed)
    special = [[9, 7, 8], [100], [7, 600, 1 << 20], [7], [], [470, 100], list(range(40))]
    qs = [q_of(special[b % 11] if b % 11 < len(special) else rng.choice(500, size=rng.integers(1, 41), replace=False), rng) for b in range(nq)]
    ks = (np.arange(nq) * 41 % 1025).astype(np.uintp)
    ks[0] = 1024
    return qs, ks


@pytest.mark.parametrize("nq,slots", [(1, 0), (63, 0), (64, 0), (65, 0), (256, 0), (257, 0), (65, 27)])
def test_query_side_edges(vdb, corpus, nq, slots):
    """a lane, a tile and a workgroup more or less; with 27 accumulator slots, chunks of 27, 27 and 11 queries"""
    C, view = corpus
    ix = index_of(vdb, C, 1)
    ix.debug_set_workspace_cap(slots * 4 * C[0].size)
    qs, ks = batch(nq, nq)
    S.check_csr(ix, C, qs, ks, view=view)
    st, rs = ix.stats(), ix.route_stats()
    assert st["candidates"] > 4096 and st["chunks"] == (3 if slots else 1)
    assert rs["route"] == 1 and rs["passes"] == st["chunks"]


@pytest.mark.parametrize("n,lens", [(63, (0, 1, 63, 64, 65, 1000)), (64, (0, 1, 63, 64, 65, 1000)), (65, (1000, 65, 64, 63, 1, 0)),
                                    (129, (0, 1, 63, 64, 65, 1000)), (129, (0,))])
def test_row_side_edges(vdb, n, lens):
    """row lengths around the block of 64 entries and far above it, mixed inside one row tile; every seventh row holds no queried
    index; then dead rows: a whole tile of them (n = 129), one between live rows, the last; a store of empty rows only"""
    rng = np.random.default_rng(n)
    vecs = []
    for r in range(n):
        pool = np.arange(600, 1700) if r % 7 == 3 else np.arange(1700)
        vecs.append(q_of(rng.choice(pool, size=lens[r % len(lens)], replace=False), rng))
    ids = np.arange(n, dtype=U64) * U64(3) + U64(1)
    offsets, indices, values = S.csr_of(vecs)
    ix = vdb.GpuSparseIndex()
    ix.set_route(1)
    ix.add_csr(ids, offsets, indices, values)
    queries = [q_of(rng.choice(600, size=300, replace=False), rng), q_of([5], rng), q_of(np.arange(400, 600), rng)]
    live = np.ones(n, dtype=bool)
    S.check_csr(ix, (ids, offsets, indices, values, live), queries, 1024)
    live[[1, n - 1]] = False
    if n > 64:
        live[:64] = False
        live[70:71] = False
    for i in ids[~live]:
        ix.remove(int(i))
    S.check_csr(ix, (ids, offsets, indices, values, live), queries, 1024)


@pytest.mark.parametrize("test", [V.test_finite_edges_bit_for_bit, V.test_every_nan_raises_when_eligible_and_is_silent_when_hidden,
                                  V.test_nan_rows_removed_are_silent_and_nothing_stays_dirty], ids=lambda t: t.__name__)
def test_values_at_the_edges_of_f32(vdb, test):
    """edge_corpus() on route 1: NaN query values of every payload (0x7fffbeef, the accumulators' pattern, among them) raise, are
    silent under a mask and after removal, and leave nothing dirty"""
    test(Routed(vdb, 1), S.edge_corpus())


@pytest.mark.parametrize("bits", [1, 64, 65])
def test_mask_edges(vdb, bits):
    SEL.test_mask_edges(Routed(vdb, 1), bits)


def test_routes_alternate_on_one_handle(vdb, corpus):
    """route 0, 1, 0, 1 with different batches, a row that widens the vocabulary (dim_slot regrows), route 1 again; under no mask,
    a host mask and a compiled one: every read equals the reference and the same read on a fresh index"""
    C, view = corpus
    ids = C[0]
    ix, fresh = index_of(vdb, C, 0), index_of(vdb, C, 0)
    eligible = (np.arange(ids.size) % 3 == 0) & (ids < BITS)
    mask = S.id_mask(ids, eligible, BITS)
    table = vdb.MetaTable(0)
    table.set_present(0, BITS, True)
    on = np.zeros(BITS, dtype=np.int32)
    on[ids[eligible].astype(np.int64)] = 1
    table.set_codes(0, 0, on)

    def read(route, seed, nq, C, view):
        qs, ks = batch(seed, nq)
        qs[1] = q_of([3000, 7, 8], np.random.default_rng(seed))
        ix.set_route(route)
        with table.compile([(vdb.MetaTable.EQ, 0, 1)], BITS) as cm:
            for kw, elig in (({}, None), (dict(mask=mask, bits=BITS), eligible), (dict(compiled=cm), eligible)):
                got = S.check_csr(ix, C, qs, ks, elig, view=view, **kw)
                assert ix.route_stats()["route"] == route
                want = S.check_csr(fresh, C, qs, ks, elig, view=view, **kw)
                assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))

    for route, seed, nq in ((0, 1, 70), (1, 2, 65), (0, 2, 65), (1, 3, 130)):
        read(route, seed, nq, C, view)
    wide = (np.array([3000, 7], U32), np.array([2.0, -1.0], F32))
    for x in (ix, fresh):
        x.add_csr(np.array([5], U64), np.array([0, 2], np.uintp), *wide)
    offsets, indices, values = S.csr_of([wide])
    C2 = (np.append(ids, U64(5)), np.append(C[1], C[1][-1] + 2), np.append(C[2], indices), np.append(C[3], values), np.ones(ids.size + 1, dtype=bool))
    eligible = np.append(eligible, False)
    read(1, 4, 66, C2, S.csc_view(C2[1], C2[2]))
    assert ix.stats()["vocab"] == 3001


@pytest.mark.parametrize("j", range(len(L.PROFILES)))
def test_pinned_schedule_on_the_row_route(vdb, j):
    L.run(L.pinned()[j], GpuAdapter(Routed(vdb, 1)))


def test_automatic_mode(vdb, corpus):
    """counted work a factor of 100 on either side of rho: 64 queries that hold every index of a store whose rows all hold the same
    five (the ratio of the two counts is 64, its maximum), then one query on index 470 of the seeded corpus (10 rows of 6000)"""
    C, view = corpus
    rng = np.random.default_rng(6)
    n, dims = 300, np.arange(5, dtype=U32)
    ids = np.arange(n, dtype=U64) + U64(1)
    offsets, indices, values = S.csr_of([q_of(dims, rng) for _ in range(n)])
    small = (ids, offsets, indices, values, np.ones(n, dtype=bool))
    for C, queries, route in ((small, [q_of(dims, rng) for _ in range(64)], 1), (C, [q_of([470], rng)], 0)):
        ix = index_of(vdb, C, 2)
        rho = ix.route_rho()
        got = S.check_csr(ix, C, queries, 10)
        df = np.bincount(C[2], minlength=1 << 12)
        inv, rows = sum(int(df[q[0]].sum()) for q in queries), C[2].size * -(-len(queries) // 64)
        assert inv >= 100 * rho * rows if route else inv <= rho / 100 * rows, (inv, rows, rho)
        rs = ix.route_stats()
        assert (rs["route"], rs["work_inverted"], rs["work_rows"]) == (route, inv, rows)
        want = S.check_csr(index_of(vdb, C, 1 - route), C, queries, 10)
        assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
    with pytest.raises(vdb.VectorDbError):
        ix.set_route(3)
