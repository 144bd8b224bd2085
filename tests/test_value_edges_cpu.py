"""Every value family (tests/value_families.py) against the oracle, at the shapes tests/test_gpu_value_edges.py uses: what each
family's docstring claims about the oracle's top-k is asserted here, so that no family degenerates silently.  No GPU needed."""
import numpy as np
import pytest

import oracle
import value_families as vf
from conftest import load_package

MIN_NORMAL = np.float32(1.17549435e-38)
NEG_ZERO = 0x80000000


def _shapes():
    L = load_package()._ffi.lib()
    out = [(name,) + s[:3] + (k,) for name, s in vf.SHAPES.items() for k in s[3]]
    n, d, nq, ks = vf.large_k_shape(L.vdb_flat_large_k_min_rows(vf.K_LARGE))
    return out + [("large_k", n, d, nq, ks[0])]


SHAPES = _shapes()


def top(metric, rows, q, k, live):
    """The oracle's first k + 1: (ids, dists); the extra entry shows whether the tie group is wider than the result."""
    oi, od = oracle.flat_search(metric, rows, q, k + 1, live=live)
    assert len(od) == k + 1 and not np.isnan(od).any()
    return oi, od, od.view(np.uint32)


def ids_decide(bits, k):
    return bits[k - 1] == bits[k]


def lowest_live(sel, live, m):
    return np.nonzero(sel & (live != 0))[0][:m].astype(np.uint64)


def claim_inf_tail(metric, rows, q, k, live, first=1, some_finite=True):
    has_inf = np.isinf(rows).any(1)
    nfin = int((~has_inf & (live != 0)).sum())
    assert (0 < nfin or not some_finite) and nfin < k      # fewer than k rows have a finite distance: no finite threshold exists
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        if metric == vf.EUCLID:
            assert np.isfinite(od[:nfin]).all() and np.isposinf(od[nfin:]).all()
            assert np.array_equal(oi[nfin:], lowest_live(has_inf, live, k + 1 - nfin))
        else:
            assert np.isneginf(od).all() and np.array_equal(oi, lowest_live(has_inf, live, k + 1))
        assert ids_decide(bits, k) and int(oi[nfin if metric == vf.EUCLID else 0]) == first   # rows 0 and 2 are dead: the group starts at id 1


def claim_overflow(metric, rows, q, k, live):
    with np.errstate(over="ignore"):
        big = np.isinf((rows.astype(np.float32) ** 2).sum(1, dtype=np.float32)) | np.isinf(np.abs(rows[:, :4]).sum(1, dtype=np.float32))
    assert k < int((big & (live != 0)).sum()) // 2 and abs(int(big.sum()) - max(rows.shape[0] // 100, 160)) <= 1
    assert np.isfinite(rows).all() and np.isfinite(q).all() and np.isinf(oracle.norm(q[0])) and np.isfinite(oracle.norm(q[1]))
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        if metric == vf.COSINE:
            assert (od == 1.0).all() and (b == 0 or big[oi.astype(np.int64)].all())
        elif metric == vf.DOT:
            assert np.isneginf(od).all() and big[oi.astype(np.int64)].all()
        elif b == 0:
            assert np.isposinf(od).all() and np.array_equal(oi, lowest_live(np.ones(len(live), bool), live, k + 1))
        else:
            assert np.isfinite(od).all() and not big[oi.astype(np.int64)].any()
            r = int(np.nonzero(big)[0][-1])
            assert np.isposinf(oracle.distance(metric, q[b], rows[r])) and np.isposinf(oracle.distance(metric, q[b], rows[1]))
        assert ids_decide(bits, k) or (metric == vf.EUCLID and b > 0)


def claim_subnormal(metric, rows, q, k, live):
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        if metric == vf.EUCLID and b % 2 == 0:
            assert (od * od < MIN_NORMAL).all()                               # the sum of squares under the root is 0 or subnormal
            if b == 0:
                assert int((bits[:k] == 0).sum()) == min(k, 40) and (ids_decide(bits, k) or k >= 40)
        elif metric == vf.EUCLID:
            r = oi[-1].astype(np.int64)
            assert ids_decide(bits, k) and od[k] >= 1.0                        # a normal distance, shared by the tiny rows ...
            assert 0 < np.abs(rows[r]).max() ** 2 < MIN_NORMAL                 # ... whose own squares are subnormal
        elif b % 2 == 0:
            assert (np.abs(od) < MIN_NORMAL).all() and (od[:k] != 0).any()    # subnormal distances (or -0.0)
            assert not (bits == 0).any()                                      # a zero dot is +0.0: its distance is -0.0, never +0.0
        else:
            assert (np.abs(od) >= MIN_NORMAL).all()


def claim_cos_den_tiny(metric, rows, q, k, live):
    den = np.float32(oracle.norm(rows[1])) * np.float32(oracle.norm(q[0]))
    assert 0 < den < MIN_NORMAL and 0 < oracle.norm(rows[1]) < 1e-21
    sub = np.float32(np.float32(2.0 ** -75) * np.float32(1.41421354))         # the smallest positive norm: its square is not 0
    assert sub * sub > 0
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        if b % 2 == 0:
            assert ids_decide(bits, k) and (od < 0.1).all()
            assert (np.abs(rows[oi.astype(np.int64)]).max(1) < 1e-21).all()   # the top-k is made of rows at the bottom of f32


def test_the_cosine_denominator_is_never_zero_or_inf_between_positive_finite_norms():
    """Why no family has n1 * n2 == 0 or == inf with both norms positive and finite: neither exists in f32.  The smallest
    positive norm is sqrtf(2^-149) and its square rounds back to 2^-149; the largest finite one is sqrtf(FLT_MAX), which rounds
    DOWN to 2^64 (1 - 2^-24), and its square is finite.  (cos_den_zero and overflow hold the neighbouring cases: a norm that
    underflows to 0, a norm that is inf.)"""
    lo = np.zeros(4, dtype=np.float32)
    lo[2] = 4e-23                                                             # 1.6e-45 rounds to 2^-149
    n_lo = np.float32(oracle.norm(lo))
    assert lo[2] * lo[2] == np.float32(2.0 ** -149) and n_lo > 0 and n_lo * n_lo == np.float32(2.0 ** -149)
    assert oracle.norm(np.full(4, 2.6e-23, dtype=np.float32)) == 0            # one step further down the norm itself is 0
    a, b = vf.fltmax_pair()
    hi = np.array([a, 0, b, 0], dtype=np.float32)
    with np.errstate(over="ignore"):
        assert np.float32(a * a) + np.float32(b * b) == np.finfo(np.float32).max
        n_hi = np.float32(oracle.norm(hi))
        assert n_hi == np.float32(2.0 ** 64 * (1 - 2.0 ** -24)) and np.isfinite(n_hi * n_hi)
        assert np.isinf(oracle.norm(np.array([a, 0, np.nextafter(b, np.float32(np.inf)), 0], dtype=np.float32)))


def claim_cos_den_clamp(metric, rows, q, k, live):
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        if b % 2 == 0:
            below = int((od < 2.0).sum())
            assert 3 <= int((bits == 0).sum()) <= below <= 7 < k and (od[below:] == 2.0).all() and ids_decide(bits, k)
            assert int(oi[below]) == 1
        else:
            assert (bits == 0).all() and int(oi[0]) == 1
    u = q[0]
    s = vf._fold(u)
    assert np.float32(s / np.float32(np.sqrt(s) * np.sqrt(s))) > 1.0           # sim really leaves [-1, 1]: the clamp made the 0.0 and 2.0


def claim_dot_zero(metric, rows, q, k, live):
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        assert not (bits == 0).any()
        if b % 2 == 0:
            assert ((od[:4] < 0) & (od[:4] > -MIN_NORMAL)).all() and (bits[4:] == NEG_ZERO).all() and ids_decide(bits, k)
            assert int(oi[4]) == 1
        else:
            assert (od < 0).all() and (od > -1e-20).all()
    h = rows.shape[1] // 2                                                    # behind the -0.0 group: tiny and ordinary positive distances
    far = oracle.flat_search(metric, rows, q[0], rows.shape[0], live=live)[1]
    assert int((far.view(np.uint32) == NEG_ZERO).sum()) > rows.shape[0] // 2 and (far[-10:] > 0).all() and h >= 4


def claim_hidden_error(metric, rows, q, k, live, code):
    for b in vf.checked_queries(q.shape[0]):
        top(metric, rows, q[b], k, live)                                      # hidden: fine
    n = rows.shape[0]
    alive = vf.live_bytes(n, hide=False)
    assert alive[vf.HIDDEN(n)] == 1 and live[vf.HIDDEN(n)] == 0
    with pytest.raises(oracle.OracleError) as e:
        oracle.flat_search(metric, rows, q[0], k, live=alive)
    assert e.value.code == code
    # the reference's own filtered search (storage.rs search_with_filter) searches every row first and filters afterwards,
    # so there a row that the filter excludes still fails it; the pre-filter model (live=) below never computes that distance
    with pytest.raises(oracle.OracleError) as e:
        oracle.search_with_filter(metric, rows[alive != 0], q[0], k, vf.id_mask(n, 0.5, 7)[0][alive != 0])
    assert e.value.code == code
    for sel in (0.5, 0.01):                                                   # excluded by the mask alone: fine; eligible: the error
        on, _ = vf.id_mask(n, sel, 7)
        oracle.flat_search(metric, rows, q[0], k, live=alive & on)
        on, _ = vf.id_mask(n, sel, 7, hide=False)
        with pytest.raises(oracle.OracleError) as e:
            oracle.flat_search(metric, rows, q[0], k, live=alive & on)
        assert e.value.code == code


def claim_tame(metric, rows, q, k, live):
    assert np.isfinite(rows).all()
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)
        assert np.isfinite(od).all() and len(set(bits.tolist())) == k + 1 and (np.abs(od) >= MIN_NORMAL).all()


CLAIMS = {
    "inf_tail": claim_inf_tail, "overflow": claim_overflow, "subnormal": claim_subnormal, "cos_den_tiny": claim_cos_den_tiny,
    "cos_den_clamp": claim_cos_den_clamp, "dot_zero": claim_dot_zero, "tame": claim_tame,
    "cos_den_zero": lambda *a: claim_hidden_error(*a, code=oracle.ERR_INVALID_VECTOR),
    "nan_hidden": lambda *a: claim_hidden_error(*a, code=oracle.ERR_NAN),
}


@pytest.mark.parametrize("shape", SHAPES, ids=["%s-k%d" % (s[0], s[4]) for s in SHAPES])
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_family_has_its_property_under_the_oracle(family, metric, shape):
    _, n, d, nq, k = shape
    rows, q = vf.make(family, n, d, nq, metric)
    CLAIMS[family](metric, rows, q, k, vf.live_bytes(n))


@pytest.mark.parametrize("family,metric", [c for c in vf.CASES if c[0] in ("inf_tail", "overflow", "subnormal", "dot_zero")],
                         ids=lambda v: str(v))
def test_masked_variants_keep_the_tie_groups(family, metric):
    """Under the masks of the GPU tests (about 50 % and about 1 %) fewer than k eligible rows of inf_tail are finite and its
    tie group starts at id 3 (0 and 2 are dead, 1 is masked out); at 50 % the other tie groups still outnumber their slots."""
    n, d, nq, ks = vf.SHAPES["tiered"]
    rows, q = vf.make(family, n, d, nq, metric)
    for sel in (0.5, 0.01):
        on, words = vf.id_mask(n, sel, 7)
        live = vf.live_bytes(n) & on
        assert not on[vf.masked_out(n)].any() and abs(on.mean() - sel) < 0.2 * sel + 0.001 and words.size * 64 >= n
        if family == "inf_tail":
            claim_inf_tail(metric, rows, q, ks[0], live, first=3, some_finite=False)
        elif sel == 0.5 and (family, metric) != ("subnormal", vf.DOT):
            oi, od, bits = top(metric, rows, q[0], ks[0], live)
            assert ids_decide(bits, ks[0]) and 1 not in oi.tolist(), (family, metric, sel)


def test_sharded_deal_and_short_parts():
    """The inf_tail tie group lies in all three contiguous shards, and the mask of the short case leaves fewer than k rows."""
    n, d, nq, ks = vf.SHAPES["tiered"]
    for metric in (vf.EUCLID, vf.DOT):
        rows, _ = vf.make("inf_tail", n, d, nq, metric)
        has_inf = np.isinf(rows).any(1)
        assert all(has_inf[lo:lo + n // 3].sum() > ks[0] for lo in (0, n // 3, 2 * (n // 3)))
    on = vf.short_mask(n)[0]
    assert 0 < int((on & (vf.live_bytes(n) != 0)).sum()) < ks[0]
    assert len({int(r) * 3 // n for r in np.nonzero(on)[0]}) == 3


def row_to_row(metric, rows):
    """Every row-to-row distance by the oracle's sequential f32 fold (Euclid, Dot), all pairs at once."""
    n, d = rows.shape
    s = np.zeros((n, n), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j in range(d):
            a, b = rows[:, j][:, None], rows[:, j][None, :]
            t = (a - b) if metric == vf.EUCLID else None
            s = s + (t * t if metric == vf.EUCLID else a * b)
        return np.sqrt(s) if metric == vf.EUCLID else -s


@pytest.mark.parametrize("n,d", vf.HNSW_SHAPES)
@pytest.mark.parametrize("family,metric", vf.HNSW_CASES, ids=["%s-m%d" % c for c in vf.HNSW_CASES])
def test_hnsw_families_hold_no_nan_and_keep_their_extremes(family, metric, n, d):
    rows, q = vf.make_hnsw(family, n, d, metric)
    assert not np.isnan(rows).any() and not np.isnan(q).any()
    pair = row_to_row(metric, rows)                                           # the graph build compares rows with rows
    for a, b in ((0, 1), (1, n - 1), (n // 2, 3), (7, n // 3)):               # (the fold below is the oracle's, bit for bit)
        assert pair[a, b].view(np.uint32) == oracle.distance(metric, rows[a], rows[b]).view(np.uint32)
    assert not np.isnan(pair[~np.eye(n, dtype=bool)]).any()
    dist = np.array([[oracle.distance(metric, q[b], rows[r]) for r in range(0, n, 7)] for b in range(q.shape[0])], dtype=np.float32)
    assert not np.isnan(dist).any()
    if family == "inf_tail":
        assert 0 < np.isinf(rows).any(1).mean() <= 0.10 and np.isinf(dist).any()
    elif family == "overflow":
        assert np.isinf(dist).any() or (metric == vf.COSINE and (dist == 1.0).any())
    elif family == "subnormal":
        assert ((np.abs(dist) < MIN_NORMAL) | (dist * dist < MIN_NORMAL)).any()
    else:
        assert (dist.view(np.uint32) == NEG_ZERO).any() and not (dist.view(np.uint32) == 0).any()


def test_merge_parts_hold_every_special_value():
    for W, k in vf.MERGE_SHAPES:
        ids, d, counts = vf.merge_parts(W, 5, k, seed=W * k)
        bits = set(d.view(np.uint32).ravel().tolist())
        assert {0x7f800000, 0xff800000, 0, NEG_ZERO, 1, 0x80000001} <= bits and not np.isnan(d).any()
        assert counts.min() == 0 and counts.max() == k and (counts < k).any()
        for p in range(W):
            for b in range(5):
                c = counts[p, b]
                o = vf.merge_order(ids[p, b, :c], d[p, b, :c])
                assert np.array_equal(o, np.arange(c))                        # every part is sorted the way the reference merges
        # -0.0 and +0.0 are EQUAL to the oracle's comparator (cmp_pair): between them the id decides
        o = vf.merge_order(np.array([5, 4], dtype=np.uint64), np.array([-0.0, 0.0], dtype=np.float32))
        assert list(o) == [1, 0]
