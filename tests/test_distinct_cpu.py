"""CPU proofs behind tests/test_gpu_distinct.py: the data of tests/distinct_data.py does under the ORACLE what the GPU tests
assume -- which stage of the driver every case must end in (the depths come from vdb_flat_distinct_depth through the ABI, which
needs no device), the prefix property of the expected answers, and the identity the exclusion rounds rest on."""
import numpy as np
import pytest

import distinct_data as dd
import range_data as rd
from conftest import load_package

U64 = np.uint64


@pytest.fixture(scope="module")
def abi_depth():
    vdb = load_package()
    vdb.build()
    return vdb.GpuFlatIndex.distinct_depth


def test_depth_at_its_edges(abi_depth):
    big = 10 ** 6
    for k, a in ((1, 32), (8, 32), (9, 36), (256, 1024), (257, 1024), (1024, 1024)):
        assert abi_depth(k, big, 0) == a == dd.depth(k, big, 0), k
        assert abi_depth(k, big, 1) == 1024 == dd.depth(k, big, 1), k
    for length in (0, 1, 31, 35, 1023):                                        # len < depth: never deeper than the index
        for k in (1, 9, 1024):
            assert abi_depth(k, length, 0) == min(length, dd.depth(k, big, 0)) == dd.depth(k, length, 0)
            assert abi_depth(k, length, 1) == length
    assert abi_depth(10, 65536, 0) == 40 and abi_depth(5, 65536, 0) == 32
    assert abi_depth(10, 65536, 2) == 0 and abi_depth(10, 65536, -1) == 0
    size_max = 2 ** 64 - 1
    assert abi_depth(size_max, size_max, 0) == 1024 and abi_depth(size_max, 5, 0) == 5


@pytest.mark.parametrize("metric", dd.METRICS)
def test_chunks_need_stage_b_and_no_more(metric, abi_depth):
    rows, q, codes = dd.chunks()
    dA, dB = abi_depth(dd.CH_K, len(rows), 0), abi_depth(dd.CH_K, len(rows), 1)
    assert (dA, dB) == (40, 1024)
    stages = []
    for b in range(dd.CH_NQ):
        rank = rd.ranking(("distinct chunks", b), metric, rows, q[b])
        ga, gb = dd.groups_within(rank, codes, dA), dd.groups_within(rank, codes, dB)
        print(f"metric {metric} query {b}: {ga} documents within {dA} ranks, {gb} within {dB}")
        assert gb >= dd.CH_K
        stages.append(dd.stage_of(rank, codes, dd.CH_K, len(rows)))
        assert len(dd.expected(rank, codes, dd.CH_K)[0]) == dd.CH_K
    assert "B" in stages and "C" not in stages, stages


@pytest.mark.parametrize("metric", dd.METRICS)
def test_dominated_needs_an_exclusion_round(metric, abi_depth):
    rows, q, members = rd.separated()
    codes = dd.dominated_codes()
    assert (codes == -1).sum() > 600 and all((codes[m] == j).all() for j, m in enumerate(members))
    assert abi_depth(dd.DOM_K, len(rows), 0) == 32
    stages = []
    for b in range(rd.NQ):
        rank = rd.ranking(("sep", b), metric, rows, q[b])
        stages.append(dd.stage_of(rank, codes, dd.DOM_K, len(rows)))
        if b % 4 == 3:                                                         # the 3000-row cluster owns every one of the first 1024 ranks
            assert dd.groups_within(rank, codes, 1024) == 1 and stages[-1] == "C", (b, stages)
            e = dd.expected(rank, codes, dd.DOM_K)
            assert len(e[0]) == dd.DOM_K and e[2][0] == 3 and 3 not in e[2][1:].tolist()
    print(metric, stages)
    assert stages.count("C") == 3
    # the second coding: after the cluster is excluded the background owns the next 1024 ranks -- a second round
    giant = dd.giant_codes()
    rank = rd.ranking(("sep", 3), metric, rows, q[3])
    keep, c = dd.kept(rank, giant)
    first = np.nonzero(keep)[0]
    assert c[first[:2]].tolist() == [3, dd.GIANT_BG] and first[1] == 3000
    rest = rank[0][~np.isin(c, (3,))]
    assert (dd.codes_of(rest[:1024], giant) == dd.GIANT_BG).all()
    assert sorted(dd.expected(rank, giant, dd.DOM_K)[2].tolist()) == [0, 1, 2, 3, dd.GIANT_BG]


@pytest.mark.parametrize("metric", dd.METRICS)
def test_tied_rows_are_decided_by_the_lower_id(metric):
    rows, q = rd.tied()
    rank = rd.ranking(("tied", 0), metric, rows, q[0])
    assert rank[0][:5].tolist() == sorted(rd.TIE_ROWS) and len({int(x) for x in rank[1][:5].view(np.uint32)}) == 1
    one = dd.expected(rank, dd.tied_codes(True), 5)
    assert one[0][0] == min(rd.TIE_ROWS) and not set(one[0][1:].tolist()) & set(rd.TIE_ROWS)
    five = dd.expected(rank, dd.tied_codes(False), 5)
    assert five[0].tolist() == sorted(rd.TIE_ROWS)


def test_small_family_has_rows_beyond_the_column():
    rows, q, codes = dd.small()
    for b in range(dd.SM_NQ):
        rank = rd.ranking(("distinct small", b), dd.EUCLID, rows, q[b])
        e = dd.expected(rank, codes, 60)
        assert len(e[0]) == 60
        beyond = e[0] >= U64(dd.SM_COL)
        assert beyond.any() and (e[2][beyond] == -1).all() and (e[2][~beyond] == codes[e[0][~beyond].astype(np.int64)]).all()
        grouped = e[2][e[2] != -1]
        assert len(set(grouped.tolist())) == len(grouped)


@pytest.mark.parametrize("metric", dd.METRICS)
def test_prefix_property(metric):
    rows, q, codes = dd.chunks()
    rank = rd.ranking(("distinct chunks", 0), metric, rows, q[0])
    full = dd.expected(rank, codes, 200)
    for k in (0, 1, 7, 10, 199):
        e = dd.expected(rank, codes, k)
        assert all(np.array_equal(x, y[:k]) for x, y in zip(e, full)) and len(e[0]) == k
    every = dd.expected(rank, codes, 10 ** 9)
    assert len(every[0]) == dd.CH_N // dd.CH_PER                               # count = min(k, groups)


@pytest.mark.parametrize("metric", dd.METRICS)
def test_excluding_kept_groups_equals_deleting_their_rows(metric):
    """The identity stage C rests on: the ranking under "mask minus the groups already kept" is the ranking with those groups'
    rows deleted -- so walking it continues the walk of the full ranking exactly where the kept groups left off."""
    rows, q, _ = rd.separated()
    codes = dd.dominated_codes()
    ok = np.arange(len(rows)) % 3 != 1                                         # the caller's mask
    rank = rd.ranking(("sep mod3", 3), metric, rows, q[3], live=ok.astype(np.uint8))
    assert not (~ok[rank[0].astype(np.int64)]).any()
    e = dd.expected(rank, codes, 3)
    gone = np.isin(codes, e[2][e[2] != -1])                                     # every row of a kept group ...
    gone[e[0][e[2] == -1].astype(np.int64)] = True                             # ... and every kept row without a group
    under = rd.ranking(("sep mod3 minus kept", 3), metric, rows, q[3], live=(ok & ~gone).astype(np.uint8))
    deleted = ~gone[rank[0].astype(np.int64)]
    assert np.array_equal(under[0], rank[0][deleted]) and np.array_equal(under[1].view(np.uint32), rank[1][deleted].view(np.uint32))
    # ... and the walk of the remainder, appended, is the walk of the whole
    more = dd.expected(under, codes, 4)
    whole = dd.expected(rank, codes, 7)
    assert all(np.array_equal(np.concatenate([a, b]), w) for a, b, w in zip(e, more, whole))
