"""The model, data and expectations of the diverse top-k tests (tests/test_mmr_cpu.py proves on the CPU what
tests/test_gpu_mmr.py assumes).  The model is the contract of include/vdb_flat.h "DIVERSE TOP-K" restated in numpy f32, a Python
loop per query:

    candidates   (id_i, d_i) = oracle.search_batch(metric, rows, q, m, ids=, live=)         ascending by (distance, unsigned id)
    pair         D(i, j) = oracle.distance(metric, row of candidate i, row of candidate j)
    pick 1       candidate 0, score F32(lam) * d_0
    after pick s, if another pick follows, for every unpicked i:
                 near_i = min(near_i, D(i, s));  score_i = F32(lam) * d_i - (F32(1) - F32(lam)) * near_i       elementwise f32
    next pick    the unpicked candidate with the smallest (isnan(score), score, position)

A NaN pair among those EVALUATED makes the request an error (`nan` of the result); the number of evaluated pairs is
sum_{t=1}^{count-1} (c - t) with count = min(k, c) -- what vdb_flat_mmr_stats reports in [3].

check() compares ids, order, distance bits, SCORE BITS and counts.  One liberty: where the model's score is a NaN (inf - inf), any
NaN of the engine matches it -- the sign and payload of a NaN an operation produces are not defined by IEEE 754 and differ between
an x86 host (0xffc00000) and the device (0x7fc00000).

THE CLUSTER FAMILY (600 x dim): 60 centres x 10 rows at spread 0.05, shuffled; queries = a centre + 0.3 * noise.  The ten nearest
rows of a query are mostly one cluster, so any lam < 1 has to leave it: the picks differ from the plain top 10.

THE TIE FAMILY is by_id_data.triplicates(): every vector three times.  After a copy is picked, its siblings have D = 0 (Euclid) to
it and equal d: they tie in score bit for bit and are taken in position order.

THE INF CASE: one finite row and two rows with +inf in element 0, Euclid.  d = (finite, inf, inf); after the finite pick both inf
rows score inf - inf = NaN and the lower position wins; a third pick would evaluate D(inf row, inf row) = NaN."""
import numpy as np

import oracle
import by_id_data as bd

F32 = np.float32
U64 = np.uint64
EUCLID, COSINE, DOT = bd.EUCLID, bd.COSINE, bd.DOT
METRICS = bd.METRICS
MAX_CANDIDATES = 1024
CL_CENTRES, CL_PER, CL_SPREAD, CL_N = 60, 10, 0.05, 600
K, M = 10, 40

_once = bd._once


def pair_distance(metric, a, b):
    """D of the contract; NaN where the reference's distance is NaN (the oracle reports that as an error of a search)"""
    with np.errstate(all="ignore"):
        return F32(oracle.distance(metric, a, b))


def select(metric, cand_vecs, d, k, lam, fused=False):
    """The greedy selection over c candidates (their vectors [c, dim] and query distances d[c], in list order).
    Returns (positions picked, scores f32, pairs evaluated, a NaN pair was evaluated).  fused=True scores with
    fma(lam, d, -(mu * near)) instead -- what a contracting compiler would make of it (tests/test_mmr_cpu.py)."""
    c = len(d)
    count = min(int(k), c)
    lam = F32(lam)
    mu = F32(1) - lam
    if count == 0:
        return [], np.zeros(0, dtype=F32), 0, False
    d = np.asarray(d, dtype=F32)
    with np.errstate(all="ignore"):
        picks, scores = [0], [F32(lam * d[0])]
        near = np.full(c, np.inf, dtype=F32)
        picked = np.zeros(c, dtype=bool)
        picked[0] = True
        pairs, nan_pair = 0, False
        for _ in range(1, count):
            s = picks[-1]
            rest = np.nonzero(~picked)[0]
            D = np.array([pair_distance(metric, cand_vecs[i], cand_vecs[s]) for i in rest], dtype=F32)
            pairs += len(rest)
            nan_pair = nan_pair or bool(np.isnan(D).any())
            near[rest] = np.minimum(near[rest], D)
            if fused:
                prod = (mu * near[rest]).astype(F32)
                score = (lam.astype(np.float64) * d[rest].astype(np.float64) - prod.astype(np.float64)).astype(F32)   # one rounding: exact in f64
            else:
                score = (lam * d[rest]).astype(F32) - (mu * near[rest]).astype(F32)
            best = None
            for j, i in enumerate(rest):                              # ascending position: a tie keeps the earlier one
                sc, isn = score[j], bool(np.isnan(score[j]))
                if best is None or isn < best[0] or (isn == best[0] and not isn and sc < best[1]):   # IEEE <: -0 == +0
                    best = (isn, sc, int(i))
            picks.append(best[2])
            scores.append(F32(best[1]))
            picked[best[2]] = True
    return picks, np.asarray(scores, dtype=F32), pairs, nan_pair


def row_of_ids(n, ids=None, live=None):
    """id -> row over the eligible-or-not LIVE rows (an id stored twice lives in its last live row)"""
    own = np.arange(n, dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    return {int(own[r]): r for r in range(n) if live is None or live[r]}


def expected(metric, rows, queries, k, m, lam, ids=None, live=None, stored=None):
    """Per query a dict: ids, dists, scores (pick order), c, pairs, nan.  k and lam: a scalar or one value per query.  live: what
    the search may return (stored and eligible); stored: what is stored (default: live) -- the rows the ids resolve to."""
    queries = np.ascontiguousarray(queries, dtype=F32)
    nq = len(queries)
    ks = [int(k)] * nq if np.isscalar(k) else [int(x) for x in k]
    lams = [lam] * nq if np.isscalar(lam) else list(lam)
    where = row_of_ids(len(rows), ids, live if stored is None else stored)
    out = []
    for b, (oi, od) in enumerate(oracle.search_batch(metric, rows, queries, min(int(m), len(rows)), ids=ids, live=live)):
        vecs = rows[[where[int(i)] for i in oi]] if len(oi) else rows[:0]
        picks, scores, pairs, nan = select(metric, vecs, od, ks[b], lams[b])
        out.append({"ids": oi[picks], "dists": od[picks], "scores": scores, "c": len(oi), "pairs": pairs, "nan": nan, "picks": picks})
    return out


def expected_cached(key, *a, **kw):
    return _once(("mmr", key), lambda: tuple(expected(*a, **kw)))


def stats(want, depth):
    """[0..4] of vdb_flat_mmr_stats for a batch whose expectation is `want`, searched at `depth`"""
    return [len(want), int(depth), sum(w["c"] for w in want), sum(w["pairs"] for w in want), sum(len(w["ids"]) for w in want)]


def check(got, want, what=""):
    """(ids [nq, >= k], dists, scores, counts) of the engine against expected(): ids, order, distance bits, score bits, counts"""
    gi, gd, gs, gc = got
    assert len(gc) == len(want), (what, len(gc), len(want))
    for b, w in enumerate(want):
        c = int(gc[b])
        assert c == len(w["ids"]), (what, b, c, len(w["ids"]))
        assert np.array_equal(gi[b, :c], w["ids"]), (what, b, gi[b, :c], w["ids"])
        assert np.array_equal(gd[b, :c].view(np.uint32), w["dists"].view(np.uint32)), (what, b, gd[b, :c], w["dists"])
        nan = np.isnan(w["scores"])
        assert np.array_equal(np.isnan(gs[b, :c]), nan), (what, b, gs[b, :c], w["scores"])
        assert np.array_equal(gs[b, :c][~nan].view(np.uint32), w["scores"][~nan].view(np.uint32)), (what, b, gs[b, :c], w["scores"])


# ------------------------------------------------------------------ the cluster family
def cluster(dim, nq=9):
    """(rows f32[600, dim], queries f32[nq, dim])"""
    def make():
        rng = np.random.default_rng(20281 + dim)
        centres = rng.standard_normal((CL_CENTRES, dim)).astype(F32)
        rows = np.repeat(centres, CL_PER, axis=0) + F32(CL_SPREAD) * rng.standard_normal((CL_N, dim)).astype(F32)
        rows = rows[rng.permutation(CL_N)].astype(F32)
        qs = centres[rng.choice(CL_CENTRES, nq, replace=False)] + F32(0.3) * rng.standard_normal((nq, dim)).astype(F32)
        return np.ascontiguousarray(rows), np.ascontiguousarray(qs.astype(F32))
    return _once(("cluster", dim, nq), make)


LAMBDA_MIX = (0.0, 0.5, 0.7, 1.0)
KS_MIX = (1, 3, 10)


def mixed(nq):
    """the per-query lambda and k arrays of the GPU cluster test"""
    lams = np.array([LAMBDA_MIX[b % 4] for b in range(nq)], dtype=F32)
    ks = np.array([KS_MIX[(b // 2) % 3] for b in range(nq)], dtype=np.uintp)
    return lams, ks


# ------------------------------------------------------------------ the inf case
def inf_case():
    """(rows f32[3, 4], query): row 0 finite, rows 1 and 2 with +inf in element 0"""
    rows = np.array([[1, 2, 3, 4], [np.inf, 0, 1, 0], [np.inf, 5, 5, 5]], dtype=F32)
    return rows, np.array([[1, 2, 3, 5]], dtype=F32)
