"""Every value family (tests/value_families.py) against the oracle, at the shapes tests/test_gpu_value_edges.py uses: what each
family's docstring claims about the oracle's top-k is asserted here, so that no family degenerates silently.  The second half
does the same for the five later read kinds (tests/test_gpu_value_edges_reads.py): which stored rows the oracle answers as queries,
what the recommend fold holds at the edges of f32 and which wrong fold shows, the outcome classes of the MMR model, the stages of
the distinct search, the bindings of the grouped one.  No GPU needed."""
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
    out.append(("large_k", n, d, nq, ks[0]))
    n, d, nq, ks = vf.large_k_split_shape(L.vdb_flat_large_k_min_rows(vf.K_LARGE))     # tests/test_gpu_value_edges_split.py
    return out + [("large_k_split", n, d, nq, ks[0])]


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


def split_hi(bits):
    """the hi word of the SPLIT layout (csrc/row_split.h): the upper half plus bit 15, modulo 2^16"""
    bits = np.asarray(bits, dtype=np.uint32)
    return ((bits >> 16) + ((bits >> 15) & 1)) & 0xffff


def bf16_rne(bits):
    """the bf16 word of a finite f32 by round-to-nearest-even"""
    bits = np.asarray(bits, dtype=np.uint64)
    return ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16) & 0xffff


def claim_bf16_edge(metric, rows, q, k, live):
    col = rows.view(np.uint32)[:, 0]
    mag = col & 0x7fffffff
    alive = live != 0
    assert np.isfinite(rows).all() and np.isfinite(q).all() and (q[:, 0] > 0).all() and (q[:, 0] < 1).all()
    for pat in vf.BF16_EDGE_BITS:                                             # every pattern in a live row, the large ones with both signs
        assert (alive & (col == pat)).any() and (pat not in vf.BF16_EDGE_LARGE or (alive & (col == pat | 0x80000000)).any()), hex(pat)
    large = np.isin(mag, vf.BF16_EDGE_LARGE)
    assert not np.isin(rows.view(np.uint32)[:, 1:] & 0x7fffffff, vf.BF16_EDGE_LARGE).any()       # column 0 alone
    special = np.isin(mag, vf.BF16_EDGE_BITS)
    assert abs(int(special.sum()) - max(rows.shape[0] // 100, 160)) <= 1
    assert ((rows.view(np.uint32)[special, 1:] & 0xffff) == 0x8000).all()      # ordinary ties everywhere else in a special row
    top_row = alive & (col == vf.BF16_EDGE_LARGE[2])
    for b in vf.checked_queries(q.shape[0]):
        oi, od, bits = top(metric, rows, q[b], k, live)                       # (asserts that no distance is NaN)
        at = oi.astype(np.int64)
        if metric == vf.EUCLID:                                               # the square of a large element overflows: +inf away
            assert np.isfinite(od).all() and not large[at].any()
            assert all(np.isposinf(oracle.distance(metric, q[b], rows[r])) for r in np.nonzero(large)[0][:12])
        elif metric == vf.DOT:                                                # finite products: +FLT_MAX first, one distance, ids decide
            lead = alive & large & (rows[:, 0] > 0)
            m, mc = min(k + 1, int(lead.sum())), min(k + 1, int(top_row.sum()))
            assert np.isfinite(od).all() and (od[:m] < -1e38).all() and lead[at[:m]].all() and (od[m:] > -1e38).all()
            assert len(set(bits[:mc].tolist())) == 1 and np.array_equal(oi[:mc], lowest_live(top_row, live, mc)) and int(oi[0]) == 1
            assert int(top_row.sum()) > 12 and (mc < k + 1 or ids_decide(bits, k))
        else:                                                                 # the row norm is inf, the dot finite: exactly 1.0
            assert (od == 1.0).all() and np.array_equal(oi, lowest_live(large, live, k + 1)) and int(oi[0]) == 1 and ids_decide(bits, k)
            assert np.isinf(oracle.norm(rows[1])) and np.isfinite(np.float32(rows[1, 0]) * q[b, 0])


def test_bf16_edge_patterns_in_the_hi_plane():
    """What the screening tier reads for each pattern of bf16_edge: the hi word of the SPLIT layout equals the round-to-nearest-even
    bf16 word for all of them but the two ties, where it is the other neighbour; the tie below FLT_MAX and FLT_MAX itself -- finite
    elements, which the forward conversion accepts -- read as the bf16 infinity in both."""
    pats = np.array(vf.BF16_EDGE_BITS, dtype=np.uint32)
    assert split_hi(pats).tolist() == [0x7f7f, 0x7f80, 0x7f80, 0x0000, 0x0001, 0x0080]
    assert bf16_rne(pats).tolist() == [0x7f7f, 0x7f80, 0x7f80, 0x0000, 0x0000, 0x0080]
    assert split_hi(pats | 0x80000000).tolist() == [0xff7f, 0xff80, 0xff80, 0x8000, 0x8001, 0x8080]
    assert np.isfinite(pats.view(np.float32)).all() and ((pats & 0x7f800000) != 0x7f800000).all()
    tie = np.uint32(0x3f808000)                                               # an ordinary tie: half up in magnitude against ties-to-even
    assert split_hi(tie) == 0x3f81 and bf16_rne(tie) == 0x3f80


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
    "inf_tail": claim_inf_tail, "overflow": claim_overflow, "bf16_edge": claim_bf16_edge, "subnormal": claim_subnormal, "cos_den_tiny": claim_cos_den_tiny,
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


# ================================================================== the five read kinds that came after the plain search
# (tests/test_gpu_value_edges_reads.py; the expectations are those of tests/value_edge_reads.py)
import by_id_data as bd
import distinct_data as dd
import mmr_data as md
import recommend_data as rd
import value_edge_reads as ver

ROW_CASES = list(zip(vf.ROW_QUERY_CASES, vf.ROW_QUERY_IDS))
BOTH_STRIKES = {("overflow", vf.DOT), ("cos_den_tiny", vf.COSINE), ("cos_den_clamp", vf.COSINE), ("dot_zero", vf.DOT)}
# families whose top-k is one tie group for (nearly) every stored row that becomes a query: the cut or the strike falls inside it
ROW_TIE_GROUPS = {("inf_tail", vf.DOT): 40, ("overflow", vf.DOT): 40, ("cos_den_clamp", vf.COSINE): 40, ("overflow", vf.EUCLID): 1,
                  ("subnormal", vf.EUCLID): 1, ("cos_den_tiny", vf.COSINE): 1}


@pytest.mark.parametrize("shape", vf.READ_SHAPES)
@pytest.mark.parametrize("case", vf.ROW_QUERY_CASES, ids=vf.ROW_QUERY_IDS)
def test_by_id_which_stored_rows_the_oracle_answers_as_queries(case, shape):
    family, metric, kw = case
    rows, q, n, d, nq = ver.case_data(case, shape)
    live = vf.live_bytes(n)
    ids = vf.by_id_ids(n)
    assert len(ids) == 50 and len(set(ids.tolist())) == 50 and live[ids].all()
    good, want, bad = ver.by_id_split(case, shape, ids, ver.K, live)
    refused = {r for r, _ in bad}
    assert all(e == "NanDistance" for _, e in bad)
    has_inf = {int(r) for r in ids if np.isinf(rows[r]).any()}
    if family == "inf_tail" and not kw:                            # plain: +inf meets +inf in nearly every pair
        assert len(refused) >= len(ids) - 1
    elif family == "inf_tail" and metric == vf.EUCLID:             # row-safe, but a row that holds an inf is inf - inf away from ITSELF
        assert refused == has_inf and {1, 3, 4, 6, 7} <= refused and len(good) >= 40
    elif (family, metric) == ("overflow", vf.COSINE):              # a row whose norm is inf: inf / inf against itself and its like
        big = {int(r) for r in ids if np.isinf(oracle.norm(rows[r]))}
        assert big and big <= refused and 12 <= len(refused) <= 20 and len(good) >= 30
    elif (family, metric) == ("bf16_edge", vf.COSINE):             # likewise, and only there: every other row stays below 1 in column 0
        big = {int(r) for r in ids if np.isinf(oracle.norm(rows[r]))}
        assert {1, 3, 4, 6, 7} <= big and refused == big and len(good) >= 40
    else:
        assert not refused, bad
    if family == "inf_tail" and kw and metric == vf.DOT:
        assert has_inf and has_inf <= set(good.tolist())          # rows that carry +inf ARE queries here
    struck, cut = sum(1 for w in want if w[2]), sum(1 for w in want if w[3])
    assert struck + cut == len(good)
    if (family, metric) in BOTH_STRIKES:
        assert struck >= 5 and cut >= 5, (struck, cut)
    if (family, metric) in ROW_TIE_GROUPS and kw == ({"frac": 0.10} if family == "inf_tail" else {}):
        lists = ver.by_id_lists(case, shape, good, ver.K, live)
        tied = sum(1 for oi, od in lists if len(od) == ver.K + 1 and ids_decide(od.view(np.uint32), ver.K))
        assert tied >= ROW_TIE_GROUPS[(family, metric)], tied
    print(family, metric, shape, "refused", len(bad), "struck/cut", struck, cut)


def test_by_id_under_the_half_mask_a_row_that_holds_an_inf_is_answered_once_it_is_ineligible_itself():
    """row 1 of the row-safe inf_tail (Euclid) is NaN away from itself only: under a mask that excludes it the search succeeds"""
    case = ("inf_tail", vf.EUCLID, {"frac": 0.10})
    n = vf.SHAPES["direct"][0]
    on, _ = vf.id_mask(n, 0.5, 7)
    assert not on[1]
    good, want, bad = ver.by_id_split(case, "direct", [1, 3], ver.K, vf.live_bytes(n) & on, tag="half")
    assert good.tolist() == [1] and bad == [(3, "NanDistance")] and np.isposinf(want[0][1]).any()


# ------------------------------------------------------------------ recommend: the fold at the bottom and the top of f32
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def flushed(x):
    x = np.array(x, dtype=np.float32, copy=True)
    x[np.abs(x) < MIN_NORMAL] = 0.0
    return x


def wrong_fold(rows, pos, neg, flush=False, from_zero=False, divide=False):
    """recommend_data.fold restated with one deliberate mistake"""
    def avg(lst):
        with np.errstate(all="ignore"):
            src = (lambda r: flushed(rows[r])) if flush else (lambda r: rows[r])
            s = np.zeros(rows.shape[1], dtype=np.float32) + src(lst[0]) if from_zero else src(lst[0]).astype(np.float32, copy=True)
            for r in lst[1:]:
                s = s + src(r)
                s = flushed(s) if flush else s
            if len(lst) > 1:
                s = s / np.float32(len(lst)) if divide else s * (np.float32(1) / np.float32(len(lst)))
            return flushed(s) if flush else s
    with np.errstate(all="ignore"):
        ap = avg(list(pos))
        if not len(neg):
            return ap
        t = ap - avg(list(neg))
        out = ap + (flushed(t) if flush else t)
        return flushed(out) if flush else out


def fold_answers(metric, rows, reqs, live, fold=None):
    """per request the oracle's outcome and its struck top 10, with recommend_data's fold or a wrong one"""
    out = []
    for p, n in reqs:
        qv = rd.fold(rows, p, n) if fold is None else fold(rows, p, n)
        o, res = ver.outcome(lambda: oracle.flat_search(metric, rows, qv, ver.K + len(p) + len(n), live=live))
        out.append((o, None if res is None else rd.strike(res[0], res[1], list(p) + list(n), ver.K)))
    return out


def answers_differ(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b))
            if x[0] != y[0] or (x[1] is not None and not (np.array_equal(x[1][0], y[1][0]) and np.array_equal(_bits(x[1][1]), _bits(y[1][1]))))]


@pytest.mark.parametrize("d", [33, 32])
def test_fold_edges_hold_every_phenomenon_and_a_wrong_fold_shows(d):
    rows, reqs = vf.fold_edges(d)
    names = [r[0] for r in vf.FOLD_REQUESTS]
    live = vf.live_bytes(vf.FOLD_N)
    assert rows.shape == (64, d) and not np.isnan(rows).any() and not np.isinf(rows).any()
    assert all(live[list(p + n)].all() for p, n in reqs)
    assert {1, 2, 5, 9} <= {len(p) for p, n in reqs} and {1, 2, 5, 9} <= {len(n) for p, n in reqs}
    qs = rd.queries(rows, reqs)
    at = {name: qs[i] for i, name in enumerate(names)}
    c = vf.FOLD_COLS
    sub = at["subnormal_5"][c["subnormal"]]
    assert 0 < sub < MIN_NORMAL and 0 < at["subnormal_9_2"][c["subnormal"]] < MIN_NORMAL
    s5 = np.float32(sum(np.float64(rows[r, 0]) for r in reqs[0][0]))              # the sum is exact; times 0.2f it is not: it rounds
    assert np.float64(s5) * np.float64(np.float32(1) / np.float32(5)) != np.float64(sub)      # inside the subnormal range
    assert _bits(at["minus_zero"])[c["zero"]] == NEG_ZERO
    assert (_bits(at["cancel_to_plus_zero"] - rows[19]) == 0).all() and (_bits(rows[19] - rows[20]) == 0).all()
    assert np.isposinf(at["overflow_mid_fold"][c["overflow"]]) and np.isinf(at["overflow_mid_fold"]).sum() == 1
    assert abs(float(np.float64(rows[[22, 23, 24, 25, 46], c["overflow"]]).sum())) < 10                 # the true average is finite
    assert np.isnan(at["inf_minus_inf"][c["inf_minus_inf"]]) and np.isnan(at["inf_minus_inf"]).sum() == 1
    fm = np.finfo(np.float32).max
    assert at["fltmax_times_rp"][c["fltmax"]] == np.float32(fm * (np.float32(1) / np.float32(3))) > np.float32(1e38)
    z = at["cosine_norm_underflows"]
    assert z.any() and oracle.norm(z) == 0 and oracle.norm(rows[32]) > 0 and oracle.norm(rows[33]) > 0
    assert sum(np.isnan(qv).any() for qv in qs) == 1 and sum(np.isinf(qv).any() for qv in qs) == 1
    # what the oracle answers: exactly the intended errors
    for metric in vf.ALL:
        right = fold_answers(metric, rows, reqs, live)
        got = {name: o for name, (o, _) in zip(names, right) if o != "ok"}
        assert got == {name: e[metric] for name, e in vf.FOLD_ERRORS.items() if metric in e}, (metric, got)
    # three wrong folds, each visible in some answer
    seen = {}
    for what, kw in (("flush", dict(flush=True)), ("divide", dict(divide=True)), ("from_zero", dict(from_zero=True))):
        seen[what] = {metric: answers_differ(fold_answers(metric, rows, reqs, live),
                                             fold_answers(metric, rows, reqs, live, lambda r, p, n: wrong_fold(r, p, n, **kw)))
                      for metric in vf.ALL}
    print(d, seen)
    assert seen["flush"][vf.DOT] and set(seen["flush"][vf.DOT]) <= {0, 1}         # subnormal * 2^127 is an ordinary number under Dot
    assert all(seen["divide"][m] for m in vf.ALL)
    # A fold started from +0.0 differs from one started from the first row in ONE way: +0.0 + -0.0 = +0.0.  The query differs ...
    zq = wrong_fold(rows, *reqs[names.index("minus_zero")], from_zero=True)
    assert _bits(zq)[c["zero"]] == 0 and (_bits(zq) != _bits(at["minus_zero"])).sum() == 1
    # ... but no distance of the reference can see the sign of a zero in a query: x * +-0 is added to a sum that starts at +0.0,
    # (+-0 - x)^2 and the norms square it.  So this mistake is caught where the GPU test looks for it: in the QUERY BITS, which
    # it compares through `recommend == search with the numpy fold`, and here.
    assert not any(seen["from_zero"].values())


def test_row_requests_cover_the_lengths_and_both_outcomes():
    for shape in vf.READ_SHAPES:
        n = vf.SHAPES[shape][0]
        reqs = vf.row_requests(n)
        live = vf.live_bytes(n)
        assert len(reqs) == 12 and {len(p) for p, _ in reqs} == {1, 2, 5, 9} and {len(x) for _, x in reqs} == {0, 1, 2}
        assert all(live[list(p + x)].all() for p, x in reqs) and 1 in reqs[3][0]
        refused = {}
        for case, name in ROW_CASES:
            rows = ver.case_data(case, shape)[0]
            good, want, bad = ver.recommend_split(case[1], rows, reqs, ver.K, live, ver.case_key(case, shape))
            refused[name] = len(bad)
            if case[0] == "inf_tail" and not case[2]:
                assert len(bad) == 12 and all(e == "NanDistance" for _, e in bad)
            elif (case[0], case[1]) in (("overflow", vf.COSINE), ("overflow", vf.DOT), ("bf16_edge", vf.COSINE)) or case[0] == "inf_tail":
                assert 1 <= len(good) and all(e == "NanDistance" for _, e in bad)
            elif case[0] == "cos_den_clamp":                       # multiples of one direction can cancel exactly: the all-zero fold
                assert len(bad) <= 2 and all(e == "InvalidVector" for _, e in bad)
            else:
                assert not bad, (name, bad)
        print(shape, refused)
        assert refused["overflow-m1"] >= 3 and refused["inf_tail-rowsafe-m0"] >= 1


# ------------------------------------------------------------------ MMR: the outcome classes of the model
def select_variant(metric, cand_vecs, cand_ids, d, k, lam, nan_first=False, tie_by_id=False):
    """mmr_data.select restated with one deliberate mistake in the choice of the next pick"""
    c = len(d)
    count = min(int(k), c)
    lam = np.float32(lam)
    mu = np.float32(1) - lam
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(all="ignore"):
        picks = [0]
        near = np.full(c, np.inf, dtype=np.float32)
        picked = np.zeros(c, dtype=bool)
        picked[0] = True
        for _ in range(1, count):
            s = picks[-1]
            rest = np.nonzero(~picked)[0]
            D = np.array([md.pair_distance(metric, cand_vecs[i], cand_vecs[s]) for i in rest], dtype=np.float32)
            near[rest] = np.minimum(near[rest], D)
            score = (lam * d[rest]).astype(np.float32) - (mu * near[rest]).astype(np.float32)
            best = None
            for j, i in enumerate(rest):
                isn = bool(np.isnan(score[j]))
                cls = (not isn) if nan_first else isn
                better = best is None or cls < best[0] or (cls == best[0] and not isn and score[j] < best[1])
                if not better and tie_by_id and cls == best[0] and (isn or score[j] == best[1]) and cand_ids[i] < cand_ids[best[2]]:
                    better = True
                if better:
                    best = (cls, score[j], int(i))
            picks.append(best[2])
            picked[best[2]] = True
    return picks


def test_mmr_outcome_classes_are_the_pinned_ones():
    """Every case x lambda x shape at k = 10, m = 40: whether a NaN pair is evaluated, and how many picks of each checked query
    were chosen with a NaN, an infinite or a subnormal score (tests/golden/value_edges_mmr_classes.json, written by
    tests/value_edge_reads.py from the model)."""
    got, pinned = ver.mmr_classes(), ver.golden_mmr_classes()
    assert got == pinned, [k for k in got if got[k] != pinned.get(k)]
    allowed = {"inf_tail-m0", "inf_tail-m2", "overflow-m1", "bf16_edge-m1"}
    errors = {k.split("/")[0] for k, v in got.items() if any(c["nan_pair"] for c in v)}
    assert errors == allowed
    for name in allowed:                                           # ... and there EVERY checked query evaluates one
        for shape in vf.READ_SHAPES:
            assert all(c["nan_pair"] for c in got["%s/%s/0.5" % (name, shape)]), (name, shape)
    ok = {k: v for k, v in got.items() if k.split("/")[0] not in allowed}
    total = lambda key, keys=None: sum(c[key] for k, v in ok.items() if keys is None or k.endswith(keys) for c in v)
    assert total("nan") > 0 and total("inf") > 0 and total("subnormal") > 0
    assert total("nan", "/0") > 0 and total("nan", "/1") > 0        # 0 * inf under lambda = 0 and under mu = 0
    assert total("nan", "/0.5") > 0                                 # inf - inf
    assert any(c["subnormal"] for k, v in ok.items() if k.startswith(("subnormal-m2", "dot_zero")) for c in v)
    # lambda = 1 is the plain order wherever the pairs are finite -- and not for query 0 of overflow under Euclid (mu * near = 0 * inf)
    assert not ok["overflow-m0/direct/1"][0]["plain_order"] and ok["overflow-m0/direct/1"][1]["plain_order"]
    assert all(c["plain_order"] for v in (ok["tame-m0/direct/1"], ok["tame-m1/tiered/1"], ok["dot_zero-m2/direct/1"]) for c in v)


def test_mmr_wrong_selections_differ_from_the_model():
    fused = nan_first = by_id = 0
    shape = "direct"
    n, _, nq, _ = vf.SHAPES[shape]
    live = vf.live_bytes(n)
    for family, metric in vf.CASES:
        case = ver.plain_case(family, metric)
        rows, q, _, _, _ = ver.case_data(case, shape)
        for lam in ver.LAMBDAS:
            want = ver.mmr_want(case, shape, vf.checked_queries(nq), ver.MMR_K, ver.MMR_M, lam, live)
            for b, w in zip(vf.checked_queries(nq), want):
                if w["nan"]:
                    continue
                oi, od = oracle.flat_search(metric, rows, q[b], ver.MMR_M, live=live)
                vecs = rows[oi.astype(np.int64)]
                if lam == 0.5:
                    p, s, _, _ = md.select(metric, vecs, od, ver.MMR_K, lam, fused=True)
                    fused += p != w["picks"] or not np.array_equal(_bits(s[~np.isnan(s)]), _bits(w["scores"][~np.isnan(w["scores"])]))
                nan_first += select_variant(metric, vecs, oi, od, ver.MMR_K, lam, nan_first=True) != w["picks"]
                by_id += select_variant(metric, vecs, oi, od, ver.MMR_K, lam, tie_by_id=True) != w["picks"]
                assert select_variant(metric, vecs, oi, od, ver.MMR_K, lam) == w["picks"]
    print("queries where a contracted score / NaN-first / ties-by-id changes the answer:", fused, nan_first, by_id)
    assert fused > 0 and nan_first > 0 and by_id > 0


# ------------------------------------------------------------------ one row per group
DISTINCT_TIES = {"inf_tail", "overflow", "cos_den_clamp", "dot_zero"}


@pytest.mark.parametrize("shape", vf.READ_SHAPES)
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_distinct_codes_reach_the_three_stages(family, metric, shape):
    n, d, nq, _ = vf.SHAPES[shape]
    case = ver.plain_case(family, metric)
    live = vf.live_bytes(n)
    codes = vf.distinct_codes(family, metric, n, d, nq)
    assert codes.shape == (n,) and (codes[vf.dead_rows(n)] == -1).all() and 3 < int((codes[live != 0] == -1).sum()) < n // 50
    rank = ver.ranking(case, shape, 0, live, "live")
    length = int(live.sum())
    assert len(rank[0]) == length
    for stage, k in vf.DISTINCT_KS.items():
        assert dd.stage_of(rank, codes, k, length) == stage, (stage, k)
        assert len(dd.expected(rank, codes, k)[0]) == k
    keep, c = dd.kept(rank, codes)
    bits = rank[1].view(np.uint32)
    by_id_alone = [p for p in np.nonzero(keep)[0][:16] if p + 1 < length and bits[p] == bits[p + 1] and c[p + 1] != c[p]]
    if family in DISTINCT_TIES:                                    # a representative whose distance the next row, of another group, shares
        assert by_id_alone, (family, metric)


# ------------------------------------------------------------------ a filter per query
@pytest.mark.parametrize("shape", vf.READ_SHAPES)
def test_group_masks_bind_every_kind_and_only_one_mask_admits_the_hidden_row(shape):
    n, d, nq, _ = vf.SHAPES[shape]
    for hide in (True, False):
        on, words, binding = vf.group_masks(n, hide)
        assert on.shape == (4, n) and words.shape == (4, (n + 63) // 64)
        for g in range(4):
            assert np.array_equal(np.unpackbits(words[g].view(np.uint8), bitorder="little")[:n].astype(bool), on[g])
        live = vf.live_bytes(n, hide)
        elig = (on & (live != 0)).sum(1)
        assert elig[0] > n // 3 and n // 200 < elig[1] < n // 50 and elig[2] == 6 and elig[3] == 0
        assert on[:, vf.HIDDEN(n)].tolist() == [not hide, False, False, False]
    for family in vf.ERROR_FAMILIES:
        for metric in vf.FAMILIES[family][1]:
            rows, q = vf.make(family, n, d, nq, metric)
            qs = vf.group_queries(q)
            go = binding(len(qs))
            assert len(qs) >= 10 and all((go == g).sum() >= 2 for g in (0, 1, 2, 3, vf.GROUP_NONE))
            on, _, _ = vf.group_masks(n, hide=False)
            live = vf.live_bytes(n, hide=False)
            for b in range(len(qs)):
                elig = live if go[b] == vf.GROUP_NONE else live & on[go[b]]
                o, _ = ver.outcome(lambda: oracle.flat_search(metric, rows, qs[b], ver.K, live=elig))
                admits = go[b] in (vf.GROUP_HOLDS_HIDDEN, vf.GROUP_NONE)         # (to an unfiltered query every live row is eligible)
                assert o == (vf.FAMILIES[family][2] if admits else "ok"), (family, metric, b, o)
