"""The segmented inverted walk of the sparse-vector index (vdb_spv_set_segmented, csrc/kernels_spv_seg.hip) against the CSR
reference (spv_data.search_csr): ids, order, distance bits, counts and the statistics, bit for bit, at the segment edges, in the
merge of the partial lists, at the edges of f32, under masks and tombstones, alternating with the other walks on one handle, over
the pinned lifecycle schedules, and where the sub-list table does not fit."""
import numpy as np
import pytest

import spv_data as S
import spv_lifecycle as L
import test_gpu_spv_select as SEL
import test_gpu_spv_values as V
from test_gpu_spv_lifecycle import GpuAdapter

pytestmark = pytest.mark.gpu
U32, F32, U64 = np.uint32, np.float32, np.uint64
MAX = 16384
BOTH = pytest.mark.parametrize("R", [64, MAX])


class Segmented:
    """the package, but every GpuSparseIndex it makes walks in segments of R rows"""

    def __init__(self, vdb, R):
        self._vdb, self._R = vdb, R

    def __getattr__(self, name):
        return getattr(self._vdb, name)

    def GpuSparseIndex(self, *a):
        ix = self._vdb.GpuSparseIndex(*a)
        ix.set_segmented(self._R)
        return ix


def same(got, want):
    return all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))


def ran(ix, R, n):
    """segment_stats of the last search on a store of n rows: the segmented walk from two segments on"""
    st, segs = ix.segment_stats(), -(-n // R)
    assert (st["segmented"], st["segments"], st["rows_per_segment"]) == ((1, segs, R) if segs > 1 else (0, 0, 0)), st
    return st


@BOTH
@pytest.mark.parametrize("n", ["R-1", "R", "R+1", "2R+1"])
def test_segment_edges(vdb, R, n):
    """index 0 in every row, 1 only in the last row of segment 0 and the first of segment 1, 2 only in the last segment, 4 nowhere,
    600 above vocab; 1 and 3 queries with k = 0, 1, 10 and 1024 rotating through the batch; the counters equal the option off"""
    n = {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[n]
    last = np.arange(max((n - 1) // R * R, n - 2), n)
    lists = {0: np.arange(n), 1: np.arange(R - 1, min(R + 1, n)), 2: last, 5: [0]}
    lists[6] = np.setdiff1d(np.arange(1, n), np.concatenate([lists[1], last]))
    ix, C, view = SEL.from_lists(Segmented(vdb, R), lists, n, seed=n)
    off = SEL.from_lists(vdb, lists, n, seed=n)[0]
    rng = np.random.default_rng(n)
    queries = [SEL.q_of([0, 1, 2, 4, 600], rng), SEL.q_of([1], rng), SEL.q_of([2, 4], rng)]
    met = [np.unique(np.concatenate([lists[d] for d in q[0].tolist() if d in lists]) // R).size for q in queries]   # segments with a posting
    for nq in (1, 3):
        for turn in range(4):
            ks = np.array([(0, 1, 10, 1024)[(turn + b) % 4] for b in range(nq)], dtype=np.uintp)
            S.check_csr(ix, C, queries[:nq], ks, view=view)
            if ks.max():                                 # (k = 0 for every query: nothing is launched)
                assert ran(ix, R, n)["workgroups"] == (sum(met[:nq]) if n > R else 0) and ix.route_stats()["route"] == 0
            off.search_batch_arrays(queries[:nq], ks)
            assert ix.stats() == off.stats() and off.segment_stats()["segmented"] == 0


@BOTH
def test_merge_of_equal_scores(vdb, R):
    """6000 rows of one score over 94 segments (R = 64), or 2000 in each of three (R = 16384: every partial list of k = 1024 is
    full); the j-th of them in segment s has id j * segments + s, so the k smallest ids lie in different segments.  Index 1:
    stored +-0.0, which both score +0.0, beside -2^-149."""
    segs, per = (94, 64) if R == 64 else (3, 2000)
    n = 6000 if R == 64 else 2 * R + per
    rows = np.concatenate([np.arange(s * R, min(s * R + per, n)) for s in range(segs)])
    ids = np.arange(n, dtype=U64) + U64(1 << 33)
    ids[rows] = ((rows % R) * segs + rows // R).astype(U64)
    weight = (lambda r, d: np.ones(r.size, F32) if d == 0 else np.where(r % 3 == 0, -S.DEN, np.where(r % 2 == 0, F32(-0.0), F32(0.0))))
    ix, C, view = SEL.from_lists(Segmented(vdb, R), {0: rows, 1: rows, 3: np.arange(n)}, n, weight=weight, ids=ids)
    out_ids, _, counts = S.check_csr(ix, C, [SEL.q_of([0]), SEL.q_of([1]), SEL.q_of([0])], np.array([1024, 1024, 10], dtype=np.uintp), view=view)
    assert ran(ix, R, n)["workgroups"] == 3 * segs
    assert np.array_equal(out_ids[0], np.arange(1024, dtype=U64)) and counts.tolist() == [1024, 1024, 10]


def shifted_edge_corpus(R):
    """edge_corpus() behind R - 3 rows that hold index 95 alone, which no query of the corpus names: its rows lie across the first
    segment boundary"""
    E, m = S.edge_corpus(), R - 3
    out = dict(E, row={name: r + m for name, r in E["row"].items()})
    out["ids"] = np.concatenate([np.arange(m, dtype=U64) + U64(1 << 20), E["ids"]])
    out["offsets"] = np.concatenate([np.arange(m, dtype=np.int64), E["offsets"] + m])
    out["indices"] = np.concatenate([np.full(m, 95, U32), E["indices"]])
    out["values"] = np.concatenate([np.ones(m, F32), E["values"]])
    return out


@BOTH
@pytest.mark.parametrize("test", [V.test_finite_edges_bit_for_bit, V.test_every_nan_raises_when_eligible_and_is_silent_when_hidden,
                                  V.test_nan_rows_removed_are_silent_and_nothing_stays_dirty], ids=lambda t: t.__name__)
def test_values_at_the_edges_of_f32(vdb, R, test):
    """the value tests of the one-workgroup walk: every NaN raises while eligible, is silent under a mask and after removal, and the
    call after an error equals the reference and a fresh index"""
    test(Segmented(vdb, R), shifted_edge_corpus(R))


@BOTH
def test_masks_and_tombstones(vdb, R):
    """a host mask and a compiled one that admit only rows of the last segment; nothing admitted; segment 1 dead as a whole; dead
    rows between live ones; an id added again, into another segment"""
    n = 3 * R + 5
    ids = np.arange(n, dtype=U64) * U64(2) + U64(1)
    bits = 2 * n + 4
    ix, C, view = SEL.from_lists(Segmented(vdb, R), {0: np.arange(n), 1: np.arange(0, n, 3)}, n, seed=R, ids=ids)
    rng = np.random.default_rng(R)
    queries = [SEL.q_of([0, 1], rng), SEL.q_of([1], rng)]
    table = vdb.MetaTable(0)
    table.set_present(0, bits, True)
    for eligible in (np.arange(n) >= 3 * R, np.zeros(n, dtype=bool)):
        on = np.zeros(bits, dtype=np.int32)
        on[ids[eligible].astype(np.int64)] = 1
        table.set_codes(0, 0, on)
        with table.compile([(vdb.MetaTable.EQ, 0, 1)], bits) as cm:
            got = S.check_csr(ix, C, queries, 10, eligible, view=view, compiled=cm)
        want = S.check_csr(ix, C, queries, 10, eligible, S.big_mask(ids, eligible, bits), bits, view=view)
        assert same(got, want) and ran(ix, R, n)["workgroups"] == 2 * 4
    live = np.ones(n, dtype=bool)
    live[R:2 * R] = False
    live[[1, 3, R - 1, 2 * R, n - 1]] = False
    for i in ids[~live]:
        ix.remove(int(i))
    S.check_csr(ix, C[:4] + (live,), queries, 1024, view=view)
    assert ran(ix, R, n)["workgroups"] == 2 * 3              # no posting is left in segment 1
    ix.add_csr(ids[:1], np.array([0, 2], np.uintp), np.array([0, 1], U32), np.array([3.0, -2.0], F32))   # row 0 again, as row n
    live = np.append(live, True)
    live[0] = False
    C2 = (np.append(ids, ids[0]), np.append(C[1], C[1][-1] + 2), np.append(C[2], [1, 0]).astype(U32), np.append(C[3], [-2.0, 3.0]).astype(F32), live)
    S.check_csr(ix, C2, queries, 1024)
    ran(ix, R, n + 1)


@BOTH
def test_walks_alternate_on_one_handle(vdb, R):
    """segmented, route 1, the option off, segmented again, each equal to the reference and to an index that never had the option;
    then a row that widens vocab and opens a third segment.  Every change of the setting rebuilds the file once."""
    n = 2 * R
    lists = {0: np.arange(n), 1: np.arange(R - 5, R + 5), 2: np.arange(0, n, 7)}
    ix, C, view = SEL.from_lists(Segmented(vdb, R), lists, n, seed=5)
    fresh = SEL.from_lists(vdb, lists, n, seed=5)[0]
    rng = np.random.default_rng(5)
    queries = [SEL.q_of([0, 1, 2], rng), SEL.q_of([3000, 1], rng)]

    def read(segmented, rebuilds, C, view):
        got = S.check_csr(ix, C, queries, 10, view=view)
        assert ix.segment_stats()["segmented"] == segmented and ix.stats()["rebuilds"] == rebuilds
        assert same(got, S.check_csr(fresh, C, queries, 10, view=view))

    read(1, 1, C, view)
    ix.set_route(1)
    read(0, 1, C, view)
    ix.set_route(0)
    ix.set_segmented(0)
    read(0, 2, C, view)
    ix.set_segmented(R)
    read(1, 3, C, view)
    ix.set_segmented(R)                                      # no change: no rebuild
    read(1, 3, C, view)
    wide = (np.array([3000, 1], U32), np.array([2.0, -1.0], F32))
    for x in (ix, fresh):
        x.add_csr(np.array([7], U64), np.array([0, 2], np.uintp), *wide)
    C2 = (np.append(C[0], U64(7)), np.append(C[1], C[1][-1] + 2), np.append(C[2], wide[0]), np.append(C[3], wide[1]), np.ones(n + 1, dtype=bool))
    read(1, 4, C2, S.csc_view(C2[1], C2[2]))
    assert ix.segment_stats()["segments"] == 3 and ix.stats()["vocab"] == 3001


@pytest.mark.parametrize("j", range(len(L.PROFILES)))
def test_pinned_schedule_in_segments_of_64(vdb, j):
    L.run(L.pinned()[j], GpuAdapter(Segmented(vdb, 64)))


@BOTH
def test_table_cap_and_refused_values(vdb, R):
    """4 * 16384 + 1 one-entry rows, one of them at index 2^24 - 1: vocab * segments + 1 words are above 2^26, the file is built
    as without the option and the one-workgroup walk answers"""
    n = 4 * MAX + 1
    dims = np.arange(n, dtype=U32) % U32(50)
    dims[n - 2] = (1 << 24) - 1
    ids = np.arange(n, dtype=U64) + U64(3)
    C = (ids, np.arange(n + 1, dtype=np.int64), dims, np.random.default_rng(7).standard_normal(n).astype(F32), np.ones(n, dtype=bool))
    ix = Segmented(vdb, R).GpuSparseIndex()
    ix.add_csr(*C[:4])
    S.check_csr(ix, C, [SEL.q_of([3, (1 << 24) - 1, 49]), SEL.q_of([(1 << 24) - 1])], 10)
    assert ix.segment_stats() == dict(segmented=0, segments=0, rows_per_segment=0, workgroups=0)
    for bad in (1, 63, 96, 2 * MAX, 1 << 40):
        with pytest.raises(vdb.VectorDbError):
            ix.set_segmented(bad)
