"""Data and expectations of the recommend tests (tests/test_recommend_cpu.py proves on the CPU what
tests/test_gpu_recommend.py assumes).  A request is (positive rows, negative rows): ROW numbers of the case's row block, at least
one positive.  Its query is the numpy restatement of include/vdb_flat.h -- elementwise f32, a Python loop over the examples in
list order, F32(1) / F32(n) for the reciprocal:

    sp = p_1; sp = sp + p_i (i = 2..np); ap = sp if np == 1 else sp * rp; q = ap, or ap + (ap - an) with negatives

and the expected answer of every case is ONE expression, computed by the oracle:

    oracle.search_batch(metric, rows, q, kcut + m, ids=, live=), every entry whose id is among the examples struck, cut to k

with m the NUMBER of examples listed (repeats counted) and kcut = min(k, rows): ids, order, distance bits and counts.  `live`
carries everything that makes a row ineligible (removed, masked out).

THE FOLD FAMILY (600 x dim).  by_id_data.scaled(600, dim) with element 0 of rows 0 and 1 set to -0.0; twelve requests whose lengths
1, 2, 5, 9 and 64 put every remainder of the four-deep load unrolling on either side, with and without negatives side by side, an
id listed twice and an id on both sides.

THE SCALED FAMILY (by_id_data.scaled(), 20000 x 32).  Row i is a gaussian scaled by (0.25, 1, 4)[i % 3]: under Dot a fold that
contains a large row points along it and finds it, while the small and medium examples of the same request are nowhere near
their own fold's top -- both outcomes of the strike (an example is in the list / is not) occur in one batch.

THE STRIKE FAMILY (by_id_data.triplicates(), 2100 x 16, every vector stored three times at one distance, in id order)."""
import numpy as np

import oracle
import by_id_data as bd

F32 = np.float32
U64 = np.uint64
EUCLID, COSINE, DOT = bd.EUCLID, bd.COSINE, bd.DOT
METRICS = bd.METRICS
MAX_EXAMPLES = 64
FOLD_N = 600
K = 10

_once = bd._once


def average(rows, lst):
    """left fold in list order from the FIRST row (not from 0), then one multiply by the f32 reciprocal"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = rows[lst[0]].astype(F32, copy=True)
        for r in lst[1:]:
            s = s + rows[r]
        if len(lst) == 1:
            return s
        return s * (F32(1) / F32(len(lst)))


def fold(rows, pos, neg):
    ap = average(rows, list(pos))
    if len(neg) == 0:
        return ap
    with np.errstate(over="ignore", invalid="ignore"):
        return ap + (ap - average(rows, list(neg)))


def queries(rows, requests):
    return np.ascontiguousarray(np.stack([fold(rows, p, n) for p, n in requests]).astype(F32))


def strike(oi, od, example_ids, k):
    """one k + m list -> (ids, dists): every entry whose id is among the examples removed, cut to k"""
    keep = ~np.isin(oi, np.asarray(example_ids, dtype=U64))
    return oi[keep][:k], od[keep][:k]


def expected(metric, rows, requests, k, ids=None, live=None):
    """per request (ids, dists); k an int or one value per request"""
    own = np.arange(len(rows), dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    ks = [int(k)] * len(requests) if np.isscalar(k) else [int(x) for x in k]
    ms = [len(p) + len(n) for p, n in requests]
    res = oracle.search_batch(metric, rows, queries(rows, requests), [min(kb, len(rows)) + m for kb, m in zip(ks, ms)], ids=ids, live=live)
    return [strike(oi, od, own[list(p) + list(n)], kb) for (oi, od), (p, n), kb in zip(res, requests, ks)]


def expected_cached(key, metric, rows, requests, k, ids=None, live=None):
    return _once(("rec", key, metric), lambda: tuple(expected(metric, rows, requests, k, ids=ids, live=live)))


def stats(metric, rows, requests, k, n_stored, ids=None, live=None):
    """what recommend_stats reports for the batch: [requests, examples, struck, depth].  The device searches ONE depth for the
    whole batch, min(max k, stored) + the longest request (at most stored), and counts the examples that stand in front of the
    cut of that list: entries with fewer than min(max k, stored) kept entries before them."""
    own = np.arange(len(rows), dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    kmax = int(k) if np.isscalar(k) else max(int(x) for x in k)
    kcut = min(kmax, max(n_stored, 1))
    depth = min(kcut + max(len(p) + len(n) for p, n in requests), n_stored)
    struck = 0
    for (oi, _), (p, n) in zip(oracle.search_batch(metric, rows, queries(rows, requests), depth, ids=ids, live=live), requests):
        hit = np.isin(oi, own[list(p) + list(n)])
        kept_before = np.cumsum(~hit) - (~hit)
        struck += int((hit & (kept_before < kcut)).sum())
    return [len(requests), sum(len(p) + len(n) for p, n in requests), struck, depth]


def check(got, want, what=""):
    """(ids [nq, >= k], dists, counts) of the engine against expected(): ids, order, distance bits, counts"""
    gi, gd, gc = got
    assert len(gc) == len(want), (what, len(gc), len(want))
    for b, (oi, od) in enumerate(want):
        c = int(gc[b])
        assert c == len(oi), (what, b, c, len(oi))
        assert np.array_equal(gi[b, :c], oi), (what, b, gi[b, :c], oi)
        assert np.array_equal(gd[b, :c].view(np.uint32), od.view(np.uint32)), (what, b, gd[b, :c], od)


def split(requests, ids=None):
    """the (positive, negative) id lists GpuFlatIndex.recommend_batch takes"""
    name = (lambda r: [int(x) for x in r]) if ids is None else (lambda r: [int(ids[x]) for x in r])
    return [name(p) for p, _ in requests], [name(n) for _, n in requests]


# ------------------------------------------------------------------ the fold family
def fold_rows(dim):
    def make():
        rows = bd.scaled(FOLD_N, dim).copy()
        rows[0, 0] = F32(-0.0)
        rows[1, 0] = F32(-0.0)
        return rows
    return _once(("foldrows", dim), make)


def fold_requests():
    """twelve requests over 600 rows: m = 1, 1, 2, 2, 5, 9, 64, 64, 3 + 1 (an id twice), 2 + 2 (an id on both sides), 6, 4 + 7"""
    def make():
        rng = np.random.default_rng(20271)
        pick = lambda n: [int(x) for x in rng.choice(np.arange(2, FOLD_N), n, replace=False)]
        a, b, c = 17, 301, 599
        big = pick(64)
        reqs = [([0], []), ([a], []), ([0, 1], []), ([a], [b]), (pick(3), pick(2)), (pick(5), pick(4)),
                (big[:40], big[40:]), (pick(64), []), ([a, a, b], [c]), ([a, b], [b, c]), (pick(6), []), (pick(4), pick(7))]
        assert sorted(len(p) + len(n) for p, n in reqs) == [1, 1, 2, 2, 4, 4, 5, 6, 9, 11, 64, 64]
        return tuple((tuple(p), tuple(n)) for p, n in reqs)
    return _once("foldreqs", make)


# ------------------------------------------------------------------ the scaled family
def scaled_requests(nreq=24):
    """request b: 3 positives of scale (4, 1, 0.25) in that order -- rows 3 j + 2, 3 j' + 1, 3 j'' -- and, for odd b, 2 small negatives"""
    def make():
        rng = np.random.default_rng(20272)
        third = bd.N // 3 - 1
        reqs = []
        for b in range(nreq):
            j = [int(x) for x in rng.choice(third, 5, replace=False)]
            pos = (3 * j[0] + 2, 3 * j[1] + 1, 3 * j[2])
            neg = (3 * j[3], 3 * j[4]) if b % 2 else ()
            reqs.append((pos, neg))
        return tuple(reqs)
    return _once(("scaledreqs", nreq), make)


# ------------------------------------------------------------------ the strike family
TRI_K, TRI_M = 250, 20


def tri_row(v, c):
    return 3 * v + c


def tri_straddle():
    """one request of 20 positives over the triplicates (Euclid) whose k + m = 270 list has examples in front of position 255 AND
    at or behind 256: the compaction's second chunk strikes and keeps.  Found by trying seeds against the oracle; the CPU test
    asserts the property."""
    def make():
        rows, ids = bd.triplicates()
        for seed in range(4000):
            rng = np.random.default_rng(30000 + seed)
            pos = tuple(int(x) for x in rng.choice(len(rows), TRI_M, replace=False))
            (oi, _), = oracle.search_batch(EUCLID, rows, queries(rows, [(pos, ())]), TRI_K + TRI_M, ids=ids)
            at = np.nonzero(np.isin(oi, ids[list(pos)]))[0]
            if (at < 255).sum() >= 2 and (at >= 256).sum() >= 1:
                return (pos, ())
        raise AssertionError("no seed puts examples on both sides of position 255 / 256")
    return _once("tristraddle", make)
