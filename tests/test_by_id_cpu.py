"""CPU proofs behind tests/test_gpu_by_id.py: the data of tests/by_id_data.py does under the ORACLE what the GPU tests assume --
under Dot a stored row is often not among its own k + 1 nearest, exact duplicates sort by id on either side of the query's own
row, and dropping the last of k + 1 when the own id is absent equals the search over the rows without it."""
import numpy as np
import pytest

import oracle
import by_id_data as bd

U64 = np.uint64


def test_scaled_family_has_both_branches_under_dot():
    rows = bd.scaled()
    sel = bd.spaced(bd.N, bd.NSEL)
    assert len(set(sel.tolist())) == bd.NSEL and sorted(np.bincount(sel % 3).tolist()) == [32, 32, 32]
    want = bd.expected_cached("scaled96", bd.DOT, rows, sel, bd.K)
    struck = sum(1 for w in want if w[2])
    cut = sum(1 for w in want if w[3])
    print(f"Dot, k = {bd.K}: {struck} of {bd.NSEL} queries have themselves within the top {bd.K + 1}, {cut} do not")
    assert struck + cut == bd.NSEL
    assert struck >= bd.NSEL // 4 and cut >= bd.NSEL // 4
    # "drop the first hit" is wrong for most of the batch: the own row leads its list for fewer queries than have it at all
    res = oracle.search_batch(bd.DOT, rows, rows[sel], bd.K + 1)
    first = sum(1 for (oi, _), r in zip(res, sel) if oi[0] == U64(r))
    print(f"the own row is the first hit for {first} of {bd.NSEL} queries")
    assert first <= struck and first < bd.NSEL // 2
    for w in want:
        assert len(w[0]) == bd.K


@pytest.mark.parametrize("metric", [bd.EUCLID, bd.COSINE])
def test_scaled_family_finds_itself_under_euclid_and_cosine(metric):
    rows = bd.scaled()
    sel = bd.spaced(bd.N, 40)
    want = bd.expected_cached("scaled40", metric, rows, sel, bd.K)
    assert all(w[2] and not w[3] and len(w[0]) == bd.K for w in want)


@pytest.mark.parametrize("metric", bd.METRICS)
def test_dropping_the_last_of_k_plus_1_equals_the_search_without_the_row(metric):
    """The identity the feature rests on: top k of (eligible rows without x) = top k + 1 of (eligible rows), minus x, cut to k."""
    rows = bd.scaled()
    sel = bd.spaced(bd.N, 12)
    want = bd.expected(metric, rows, sel, bd.K)
    for r, (oi, od, _, _) in zip(sel, want):
        live = np.ones(bd.N, dtype=np.uint8)
        live[r] = 0
        wi, wd = oracle.flat_search(metric, rows, rows[r], bd.K, live=live)
        assert np.array_equal(oi, wi) and np.array_equal(od.view(np.uint32), wd.view(np.uint32)), r


@pytest.mark.parametrize("metric", [bd.EUCLID, bd.COSINE])
def test_triplicates_sort_around_the_own_row_by_id(metric):
    rows, ids = bd.triplicates()
    before = after = 0
    for copy in (0, 1, 2):
        for v in (0, 5, bd.TRI_V - 1):
            r = 3 * v + copy
            own = ids[r]
            twins = {int(ids[3 * v + c]) for c in range(3) if c != copy}
            oi, od = oracle.flat_search(metric, rows, rows[r], bd.K + 1, ids=ids)
            pos = int(np.nonzero(oi == own)[0][0])
            tpos = sorted(int(np.nonzero(oi == U64(t))[0][0]) for t in twins)
            assert sorted(tpos + [pos]) == [0, 1, 2], (copy, v, oi[:4])                # the three copies lead the list ...
            assert len({od[p].view(np.uint32) for p in (0, 1, 2)}) == 1                # ... at one distance, bit for bit
            assert list(oi[:3]) == sorted(oi[:3])                                      # ... in id order
            assert pos == copy                                                         # so the own row is 1st, 2nd or 3rd
            before += sum(1 for p in tpos if p < pos)
            after += sum(1 for p in tpos if p > pos)
            si, sd, struck, cut = bd.strike(oi, od, own, bd.K)
            assert struck and not cut and own not in si and twins <= set(si[:2].tolist()) and len(si) == bd.K
    assert before > 0 and after > 0


def test_strike_counts_at_the_edges():
    """count = min(k, eligible - [x eligible]) from the k + 1 list"""
    rows = bd.scaled(64, 8)
    sel = np.array([3, 7])
    for k, n_want in ((0, 0), (1, 1), (63, 63), (64, 63), (500, 63)):
        for oi, od, struck, cut in bd.expected(bd.EUCLID, rows, sel, k):
            assert len(oi) == n_want and (struck or k == 0) and not (struck and cut)
    live = np.ones(64, dtype=np.uint8)
    live[3] = 0                                                                        # the query's own row is not eligible
    (oi, od, struck, cut), = bd.expected(bd.EUCLID, rows, sel[:1], 10, live=live)
    assert not struck and cut and len(oi) == 10 and 3 not in oi
    (oi, od, struck, cut), = bd.expected(bd.EUCLID, rows, sel[:1], 63, live=live)
    assert not struck and not cut and len(oi) == 63
