"""CPU proofs behind tests/test_gpu_range.py: the data of tests/range_data.py does under the ORACLE what the GPU tests assume --
the totals of the separated family at the chosen radii, radii taken at a neighbour hitting that neighbour bit for bit, the
boundary rows of the value families, and the inclusion rule d <= r itself."""
import numpy as np
import pytest

import oracle
import range_data as rd
import value_families as vf

F32 = np.float32
METRICS = (rd.EUCLID, rd.COSINE, rd.DOT)


@pytest.mark.parametrize("metric", METRICS)
def test_separated_totals_are_the_cluster_sizes(metric):
    rows, q, members = rd.separated()
    r = rd.ENCLOSE[metric]
    for b in range(rd.NQ):
        j = b % len(rd.CLUSTERS)
        oi, od, c, total = rd.cut(rd.ranking(("sep", b), metric, rows, q[b]), r, rd.N)
        assert total == rd.CLUSTERS[j], (b, total)
        assert np.array_equal(np.sort(oi), members[j].astype(np.uint64)), b
    # the totals the GPU tests rely on: 0, 1, max_results - 1, max_results, max_results + 1, (2048, 32768], above 32768
    rank0, rank1 = rd.ranking(("sep", 0), metric, rows, q[0]), rd.ranking(("sep", 1), metric, rows, q[1])
    assert rd.cut(rank0, rd.below(rd.radius_at(rank0, 1)), 8)[3] == 0
    assert rd.cut(rank0, rd.radius_at(rank0, 1), 8)[3] == 1 and rd.cut(rank0, r, 8)[3] == 1
    for mr in (39, 40, 41):                                         # total 40 = max_results + 1, max_results, max_results - 1
        assert rd.cut(rank1, r, mr)[2:] == (min(40, mr), 40)
    assert rd.MAX_SELECT < rd.cut(rd.ranking(("sep", 3), metric, rows, q[3]), r, 8)[3] <= rd.SCAN_CAP
    dense = rd.cut(rank0, rd.radius_at(rank0, rd.DENSE_RANK), 8)[3]
    assert dense >= rd.DENSE_RANK > rd.SCAN_CAP


@pytest.mark.parametrize("metric", METRICS)
def test_separated_gap_is_far_above_the_bf16_error_budget(metric):
    """In score units: how many bf16 error budgets lie between the radius and the nearest row outside it."""
    rows, q, members = rd.separated()
    worst = np.inf
    for b in range(rd.NQ):
        own = members[b % len(rd.CLUSTERS)]
        out = np.ones(rd.N, dtype=bool)
        out[own] = False
        gap = rd.score(metric, q[b], rows[out]) - rd.radius_score(metric, q[b], rd.ENCLOSE[metric])
        worst = min(worst, float((gap / rd.bf16_budget(metric, q[b], rows[out])).min()))
        inside = rd.radius_score(metric, q[b], rd.ENCLOSE[metric]) - rd.score(metric, q[b], rows[own])
        assert (inside > 0).all()
    print(f"metric {metric}: nearest excluded row lies {worst:.1f} bf16 error budgets above the radius")
    assert worst >= 20.0


@pytest.mark.parametrize("metric", METRICS)
def test_radius_at_a_neighbour_is_that_neighbours_distance_bit_for_bit(metric):
    rows, q = rd.gaussian()
    for b in (0, rd.NQ - 1):
        rank = rd.ranking(("gauss", b), metric, rows, q[b])
        for m in (1, 10, 200):
            r = rd.radius_at(rank, m)
            assert r.view(np.uint32) == rank[1][m - 1].view(np.uint32)
            assert F32(oracle.distance(metric, q[b], rows[int(rank[0][m - 1])])).view(np.uint32) == r.view(np.uint32)
            total = rd.cut(rank, r, 1)[3]
            group = int((rank[1] == r).sum())
            assert total >= m and rd.cut(rank, rd.below(r), 1)[3] == total - group
    rows, q = rd.tied()
    rank = rd.ranking(("tied", 0), metric, rows, q[0])
    r = rd.radius_at(rank, 1)
    assert rd.cut(rank, r, 8)[3] == len(rd.TIE_ROWS) and rd.cut(rank, rd.below(r), 8)[3] == 0
    assert list(rank[0][:5]) == sorted(rd.TIE_ROWS)                 # the group comes out ordered by id


def _total(family, metric, b, r, shape="direct"):
    n, d, nq, _ = vf.SHAPES[shape]
    rows, q = vf.make(family, n, d, nq, metric)
    return rd.cut(rd.ranking((family, shape, b), metric, rows, q[b]), r, n), n


def test_value_families_put_rows_on_the_boundary_radii():
    inf, ninf = F32(np.inf), F32(-np.inf)
    (oi, od, c, total), n = _total("inf_tail", rd.EUCLID, 0, inf)
    assert total == n and od[-1] == inf
    assert 0 < _total("inf_tail", rd.EUCLID, 0, F32(1e30))[0][3] <= vf.F_FINITE
    (oi, od, c, total), n = _total("inf_tail", rd.DOT, 0, ninf)
    assert n - vf.F_FINITE <= total < n and (od == ninf).all()
    # overflow: Euclid +inf for every row under query 0; Dot -inf first; Cosine the group at exactly 1.0
    assert _total("overflow", rd.EUCLID, 0, F32(3e38))[0][3] == 0 and _total("overflow", rd.EUCLID, 0, inf)[0][3] == 3000
    assert _total("overflow", rd.DOT, 1, ninf)[0][3] >= 80
    (oi, od, c, total), n = _total("overflow", rd.COSINE, 1, F32(1.0))
    assert total >= 160 and (od == F32(1.0)).all() and _total("overflow", rd.COSINE, 1, rd.below(1.0))[0][3] == 0
    # subnormal: exact 0.0 distances under query 0 (Euclid), +0.0 and -0.0 admit the same rows
    z = _total("subnormal", rd.EUCLID, 0, F32(0.0))[0][3]
    assert z >= 40 and _total("subnormal", rd.EUCLID, 0, F32(-0.0))[0][3] == z
    (oi, od, c, total), n = _total("dot_zero", rd.DOT, 0, F32(0.0))
    assert total > 0.4 * n and np.signbit(od[-1]) and od[-1] == 0.0  # the tie group at -0.0 is inside a radius of +0.0
    assert _total("dot_zero", rd.DOT, 0, F32(-0.0))[0][3] == total
    assert _total("dot_zero", rd.DOT, 0, rd.below(-0.0))[0][3] == 4  # only the tiny positive dots lie below it
    # cos_den_clamp: along +u three rows at 0.0 (and those of the four awkward multiples that round there), the rest up to exactly
    # 2.0; along -u one tie group at 0.0
    assert 3 <= _total("cos_den_clamp", rd.COSINE, 0, F32(0.0))[0][3] <= 7
    (oi, od, c, total), n = _total("cos_den_clamp", rd.COSINE, 0, F32(2.0))
    assert total == n and od[-1] == F32(2.0) and _total("cos_den_clamp", rd.COSINE, 0, rd.below(2.0))[0][3] <= 7
    assert n - 7 <= _total("cos_den_clamp", rd.COSINE, 1, F32(0.0))[0][3] <= n - 3


@pytest.mark.parametrize("metric", METRICS)
def test_inclusion_rule_against_the_oracles_distance(metric):
    """d <= r in IEEE arithmetic: a row at exactly r is in, -0.0 equals +0.0, nothing is within a NaN radius."""
    rows, q = rd.gaussian()
    rank = rd.ranking(("gauss", 0), metric, rows, q[0])
    r = rd.radius_at(rank, 10)
    oi, od, c, total = rd.cut(rank, r, rd.N)
    inside = set(int(i) for i in oi)
    for row in list(rank[0][:14]) + [123, 45678]:
        d = F32(oracle.distance(metric, q[0], rows[int(row)]))
        assert (d <= r) == (int(row) in inside), row
    assert F32(oracle.distance(metric, q[0], rows[int(rank[0][9])])) == r       # the 10th neighbour lies AT the radius: included
    assert F32(-0.0) <= F32(0.0) and F32(0.0) <= F32(-0.0)
    zero = (np.zeros(1, dtype=np.uint64), np.array([-0.0], dtype=F32))
    assert rd.cut(zero, F32(0.0), 4)[3] == 1 and rd.cut(zero, F32(-0.0), 4)[3] == 1
    assert rd.cut(rank, F32(np.nan), 4)[3] == 0                     # (the call refuses a NaN radius: INVALID_ARGUMENT)
