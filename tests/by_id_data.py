"""Data and expectations of the search-by-stored-id tests (tests/test_by_id_cpu.py proves on the CPU what
tests/test_gpu_by_id.py assumes).  The expected answer of every case is ONE sentence, computed by the oracle:

    oracle.search_batch(metric, rows, rows[sel], k + 1, ids=, live=), the query's own id struck if it is there,
    otherwise the last entry dropped, cut to k

-- ids, order, distance bits and counts.  `live` carries everything that makes a row ineligible (removed, masked out).

THE SCALED GAUSSIAN FAMILY (20000 x 32).  Row i is a unit gaussian scaled by (0.25, 1, 4)[i % 3].  Under Dot the distance of a
row to itself is -|x|^2: about -2, -32 and -512 for the three scales, while a large row nearby reaches far below -32 -- so a
small or medium row is NOT among its own k + 1 nearest, and a large one is.  The 96 evenly spaced query rows (stride 208 = 1 mod 3)
take each scale 32 times: both branches of the strike (the id is found / the list is cut) run in one batch, and
"drop the first hit" is wrong for two thirds of it.

THE TRIPLICATE FAMILY (2100 x 16).  Every vector is stored three times, copy c of vector v in row 3 v + c under id c * 700 + v:
the three ids of a vector interleave with everybody else's.  The copies are at exactly the same distance from any query, so they
come out in id order: for the query with copy 0 both twins FOLLOW its own row, with copy 2 both PRECEDE it, with copy 1 one does
each -- under Euclid and Cosine the own row is therefore first, third or second, never reliably "the first hit"."""
import numpy as np

import oracle

F32 = np.float32
U64 = np.uint64
EUCLID, COSINE, DOT = 0, 1, 2
METRICS = (EUCLID, COSINE, DOT)
N, D, K = 20000, 32, 10
SCALES = (0.25, 1.0, 4.0)
NSEL = 96
TRI_V, TRI_D = 700, 16

_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def scaled(n=N, d=D):
    """rows f32[n, d]: row i = gaussian * SCALES[i % 3]"""
    def make():
        rng = np.random.default_rng(20261 + n * 131 + d)
        rows = rng.standard_normal((n, d)).astype(F32)
        rows *= np.asarray(SCALES, dtype=F32)[np.arange(n) % 3][:, None]
        return np.ascontiguousarray(rows)
    return _once(("scaled", n, d), make)


def spaced(n, m):
    """m evenly spaced row numbers of an n-row index"""
    return (np.arange(m) * (n // m)).astype(np.int64)


def triplicates():
    """(rows f32[3 V, D], ids u64[3 V]): copy c of vector v in row 3 v + c under id c * V + v"""
    def make():
        rng = np.random.default_rng(20262)
        base = rng.standard_normal((TRI_V, TRI_D)).astype(F32)
        rows = np.repeat(base, 3, axis=0)
        r = np.arange(3 * TRI_V)
        ids = ((r % 3) * TRI_V + r // 3).astype(U64)
        return np.ascontiguousarray(rows), ids
    return _once("tri", make)


def strike(oi, od, own, k):
    """one k + 1 list -> (ids, dists, struck, cut): the own id removed if it is there, else the last of k + 1 dropped"""
    hit = np.nonzero(oi == U64(own))[0]
    if hit.size:
        keep = np.delete(np.arange(len(oi)), hit[0])
        return oi[keep][:k], od[keep][:k], True, False
    return oi[:k], od[:k], False, len(oi) > k


def expected(metric, rows, sel, k, ids=None, live=None):
    """per query row in sel: (ids, dists, struck, cut); k an int or one value per query"""
    own = np.arange(len(rows), dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    ks = [int(k)] * len(sel) if np.isscalar(k) else [int(x) for x in k]
    res = oracle.search_batch(metric, rows, rows[np.asarray(sel)], [min(x, len(rows)) + 1 for x in ks], ids=ids, live=live)
    return [strike(oi, od, own[r], kb) for (oi, od), r, kb in zip(res, sel, ks)]


def expected_cached(key, metric, rows, sel, k, ids=None, live=None):
    return _once(("exp", key, metric), lambda: tuple(expected(metric, rows, sel, k, ids=ids, live=live)))


def check(got, want, what=""):
    """(ids [nq, >= k], dists, counts) of the engine against expected(): ids, order, distance bits, counts"""
    gi, gd, gc = got
    assert len(gc) == len(want), (what, len(gc), len(want))
    for b, (oi, od, _, _) in enumerate(want):
        c = int(gc[b])
        assert c == len(oi), (what, b, c, len(oi))
        assert np.array_equal(gi[b, :c], oi), (what, b, gi[b, :c], oi)
        assert np.array_equal(gd[b, :c].view(np.uint32), od.view(np.uint32)), (what, b, gd[b, :c], od)
