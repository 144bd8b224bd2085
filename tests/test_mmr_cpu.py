"""CPU proofs behind tests/test_gpu_mmr.py: the library exports the diverse top-k entry points, and the data of
tests/mmr_data.py makes a wrong kernel VISIBLE -- the pair distances are bit-symmetric, the picks of the cluster family leave the
plain top 10, a contracted score differs in its bits, the triplicates tie and resolve by position, and a NaN score ranks last."""
import os
import re

import numpy as np
import pytest

import oracle
import by_id_data as bd
import mmr_data as md
from conftest import load_package

F32, U64 = np.float32, np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vdb_flat_search_batch_mmr", "vdb_flat_search_batch_mmr_filtered", "vdb_flat_mmr_stats")


def test_library_exports_and_ffi_declares_the_three_symbols():
    vdb = load_package()
    vdb.build()
    L = vdb._ffi.lib()
    header = open(os.path.join(ROOT, "include", "vdb_flat.h")).read()
    for name in NAMES:
        assert name in vdb._ffi.SYMBOLS
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert len(L.vdb_flat_search_batch_mmr.argtypes) == 16 and len(L.vdb_flat_search_batch_mmr_filtered.argtypes) == 15
    assert len(L.vdb_flat_mmr_stats.argtypes) == 2
    assert re.search(r"#define VDB_MMR_MAX_CANDIDATES %d\b" % md.MAX_CANDIDATES, header)
    assert L.vdb_abi_version() == 1
    for cls, names in ((vdb.GpuFlatIndex, ("search_batch_mmr", "mmr_stats")), (vdb.VectorStore, ("search_mmr", "search_mmr_batch"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def bits(x):
    return np.asarray(x, dtype=F32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("metric", md.METRICS)
def test_pair_distances_are_symmetric_bit_for_bit(metric):
    families = [md.cluster(17)[0][:60], md.cluster(33)[0][:60], bd.triplicates()[0][:45], bd.scaled()[:60]]
    if metric == md.EUCLID:
        families.append(md.inf_case()[0])
    for rows in families:
        for i in range(len(rows)):
            for j in range(i + 1, len(rows), 7):
                a, b = md.pair_distance(metric, rows[i], rows[j]), md.pair_distance(metric, rows[j], rows[i])
                assert np.array_equal(bits(a), bits(b)) or (np.isnan(a) and np.isnan(b)), (metric, i, j, a, b)


@pytest.mark.parametrize("metric", md.METRICS)
@pytest.mark.parametrize("dim", [17, 33])
def test_cluster_family_leaves_the_plain_top_10(dim, metric):
    rows, qs = md.cluster(dim, 8)
    plain = oracle.search_batch(metric, rows, qs, md.K)
    differ = leave = 0
    for lam in (0.5, 0.7):
        for w, (pi, _) in zip(md.expected(metric, rows, qs, md.K, md.M, lam), plain):
            assert len(w["ids"]) == md.K and w["c"] == md.M and not w["nan"] and w["pairs"] == sum(md.M - t for t in range(1, md.K))
            assert w["picks"][0] == 0 and len(set(w["picks"])) == md.K
            differ += int(w["ids"].tolist() != pi.tolist())
            leave += int(set(w["ids"].tolist()) != set(pi.tolist()))
    print(f"dim {dim} metric {metric}: the picks differ from the plain top {md.K} in {differ} of 16 cases, as a set in {leave}")
    assert differ >= 8 and leave >= 4
    # lambda = 1: the plain top 10, ids and distance bits, and the score is the distance
    for w, (pi, pd) in zip(md.expected(metric, rows, qs, md.K, md.M, 1.0), plain):
        assert np.array_equal(w["ids"], pi) and np.array_equal(bits(w["dists"]), bits(pd)) and np.array_equal(bits(w["scores"]), bits(pd))


@pytest.mark.parametrize("metric", md.METRICS)
def test_a_contracted_score_is_visible(metric):
    """lam = 0.7: lam * d is inexact, so fma(lam, d, -(mu * near)) rounds differently from the two-step form in some pick.
    lam = 0.5: the product is exact (a power of two), the fused and the separate forms CANNOT differ -- asserted, too."""
    rows, qs = md.cluster(33, 8)
    res = oracle.search_batch(metric, rows, qs, md.M)
    seen = 0
    for oi, od in res:
        vecs = rows[oi.astype(np.int64)]
        a = md.select(metric, vecs, od, md.K, 0.7)
        b = md.select(metric, vecs, od, md.K, 0.7, fused=True)
        seen += int(a[0] != b[0] or not np.array_equal(bits(a[1]), bits(b[1])))
        a = md.select(metric, vecs, od, md.K, 0.5)
        b = md.select(metric, vecs, od, md.K, 0.5, fused=True)
        assert a[0] == b[0] and np.array_equal(bits(a[1]), bits(b[1]))
    print(f"metric {metric}: the fused score differs in {seen} of {len(res)} cases at lambda 0.7")
    assert seen >= 1


@pytest.mark.parametrize("metric", [md.EUCLID, md.DOT])
def test_triplicates_tie_and_resolve_by_position(metric):
    rows, ids = bd.triplicates()
    qs = rows[[3 * 5, 3 * 333 + 1, 3 * 699 + 2]] + F32(0.01)
    for w in md.expected(metric, rows, qs, 30, 30, 0.5, ids=ids):
        p = w["picks"]
        assert sorted(p) == list(range(30)) and not w["nan"]
        # The candidates come in runs of three copies (positions 3 g .. 3 g + 2: equal d, ascending id).  Copies are the same
        # vector, so their near and score are equal bit for bit at every step: only the position decides among them.
        when = {pos: t for t, pos in enumerate(p)}
        for g in range(10):
            assert bits(w["dists"][when[3 * g]]) == bits(w["dists"][when[3 * g + 1]]) == bits(w["dists"][when[3 * g + 2]])
            assert when[3 * g] < when[3 * g + 1] < when[3 * g + 2], (g, p)
            if metric == md.EUCLID:
                # D = 0 to the picked copy and nothing is nearer: both siblings are chosen with lam * d - mu * 0
                assert bits(w["scores"][when[3 * g + 1]]) == bits(w["scores"][when[3 * g + 2]])
        assert p[1] != 1                                                       # the siblings of pick 1 are the LAST thing MMR wants


def test_a_nan_score_ranks_last_and_a_nan_pair_is_an_error():
    rows, q = md.inf_case()
    (w2,) = md.expected(md.EUCLID, rows, q, 2, 3, 0.5)
    assert w2["ids"].tolist() == [0, 1] and np.isnan(w2["scores"][1]) and not w2["nan"] and w2["pairs"] == 2
    assert np.isinf(w2["dists"][1])
    (w3,) = md.expected(md.EUCLID, rows, q, 3, 3, 0.5)
    assert w3["nan"] and w3["pairs"] == 3
    # among a NaN and a number the number wins, also from the later position (select() does not need d ascending)
    vecs = np.array([[0, 0], [np.inf, 0], [3, 4]], dtype=F32)
    picks, scores, _, nan = md.select(md.EUCLID, vecs, np.array([1, np.inf, 3], dtype=F32), 2, 0.5)
    assert picks == [0, 2] and not nan and scores[1] == F32(0.5) * F32(3) - F32(0.5) * F32(5)


def test_counts_and_stats_of_the_model():
    rows, qs = md.cluster(17, 8)
    live = np.zeros(len(rows), dtype=np.uint8)
    live[[3, 50, 51, 300, 599]] = 1
    want = md.expected(md.EUCLID, rows, qs, 10, 40, 0.5, live=live, stored=np.ones(len(rows), dtype=np.uint8))
    assert all(len(w["ids"]) == 5 and w["c"] == 5 and w["pairs"] == 4 + 3 + 2 + 1 for w in want)
    assert md.stats(want, 40) == [8, 40, 40, 80, 40]
    lams, ks = md.mixed(8)
    want = md.expected(md.EUCLID, rows, qs, ks, 40, lams)
    assert [len(w["ids"]) for w in want] == ks.tolist()
    full = md.expected(md.EUCLID, rows, qs, 10, 40, lams)
    for w, f, kb in zip(want, full, ks):                                       # prefix stability
        assert np.array_equal(w["ids"], f["ids"][:kb]) and np.array_equal(bits(w["scores"]), bits(f["scores"][:kb]))
