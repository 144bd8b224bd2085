"""Data and the model of the late-interaction (MaxSim) tests (vdb_flat_search_batch_maxsim).
THE DEFINITION (expected()): d(t, x) is the CPU oracle's distance of token t and row x (one full oracle ranking per token over the
eligible rows, scattered back by row; pair by pair, the NaN kept, where the oracle refuses the ranking).  A row is eligible when it
is live, admitted and has a code >= 0.  m(t, c) = the minimum over the eligible rows of code c of the ORDERED u32 image of d(t, x);
score(c) = a sequential np.float32 sum of m(t_1, c), m(t_2, c), ... from the first term; the answer is the codes by (ordered
score, code), cut to k.  A NaN d(t, x) at an eligible row, or a NaN score, is NanDistance.
THE DATA: rows(n, dim) gaussian rows in three scales (tie-free); tokens(dim, Ts) one block per T; layout(name, n) the code of every
ROW: one-row documents | 16 adjacent rows a document | the same under a permutation | mixed: one-row documents, rows without a
code, a run across the wave boundary (rows 60..69), runs of 16, a run across the workgroup boundary (250..261), five interleaved
codes, ONE run of 300 rows, 37 interleaved codes, with N_CODES = 500 larger than the codes in use."""
import numpy as np

import oracle
import by_id_data as bd
from recommend_best_data import NanDistance, ordered

F32, U32, I32 = np.float32, np.uint32, np.int32
EUCLID, COSINE, DOT = bd.EUCLID, bd.COSINE, bd.DOT
METRICS = bd.METRICS
T_EDGES = (1, 7, 8, 9, 16, 17, 32)
N_CODES = 500
LAYOUTS = ("single", "adjacent", "scattered", "mixed")
rows = bd.scaled


def tokens(dim, Ts=T_EDGES):
    rng = np.random.default_rng(27270 + dim)
    return [np.ascontiguousarray(rng.standard_normal((T, dim)), dtype=F32) for T in Ts]


def layout(name, n):
    """(codes i32[n] by row, n_codes)"""
    r = np.arange(n)
    if name == "single":
        return r.astype(I32), n
    if name in ("adjacent", "scattered"):
        return ((np.random.default_rng(20271).permutation(n) if name == "scattered" else r) // 16).astype(I32), n // 16 + 1
    c = (400 + r % 37).astype(I32)
    c[:50], c[50:60], c[60:70], c[250:262], c[300:600] = r[:50], -1, 100, 101, 102
    c[70:250] = 200 + (r[70:250] - 70) // 16
    c[262:300] = 300 + (r[262:300] * 7) % 5
    return c[:n].copy(), N_CODES


def from_ordered(u):
    return np.where(u & U32(0x80000000), u & U32(0x7fffffff), ~u).astype(U32).view(F32)


def distances(metric, rows_, toks, elig):
    """d(t, x) f32[T, n]; +inf at rows that are not eligible (never read)"""
    out = np.full((len(toks), len(rows_)), np.inf, dtype=F32)
    for t, q in enumerate(toks):
        try:
            oi, od = oracle.flat_search(metric, rows_, q, len(rows_), live=np.ascontiguousarray(elig, dtype=np.uint8))
            out[t, oi.astype(np.int64)] = od
        except oracle.OracleError as err:
            if "NaN" not in str(err):
                raise
            for x in np.nonzero(elig)[0]:
                out[t, x] = oracle.distance(metric, q, rows_[x])
    return out


def eligible(row_codes, ok):
    return (np.asarray(row_codes) >= 0) & (True if ok is None else np.asarray(ok, dtype=bool))


def expected(metric, rows_, row_codes, token_lists, k, ok=None):
    """per query (codes i32[m], scores f32[m]); k an int or one per query; ok: the live, admitted rows"""
    elig = eligible(row_codes, ok)
    docs, at = np.unique(np.asarray(row_codes)[elig], return_inverse=True)
    out = []
    for toks, kb in zip(token_lists, np.broadcast_to(k, len(token_lists))):
        d = distances(metric, rows_, toks, elig)[:, elig]
        m = np.full((len(toks), docs.size), 0xffffffff, dtype=U32)
        for t in range(len(toks)):
            np.minimum.at(m[t], at, ordered(d[t]))
        m = from_ordered(m)
        score = m[0].copy()
        with np.errstate(invalid="ignore"):
            for t in range(1, len(toks)):
                score = (score + m[t]).astype(F32)
        if np.isnan(d).any() or np.isnan(score).any():
            raise NanDistance(metric)
        o = np.lexsort((docs, ordered(score)))[:int(kb)]
        out.append((docs[o].astype(I32), score[o]))
    return out


def stats(row_codes, token_lists, want, chunks=1, ok=None):
    """vdb_flat_maxsim_stats predicted"""
    elig, nq = eligible(row_codes, ok), len(token_lists)
    return [nq, sum(len(t) for t in token_lists), chunks, nq * int(elig.sum()), nq * np.unique(np.asarray(row_codes)[elig]).size,
            sum(len(c) for c, _ in want), 0, 0]


def check(got, want, what=""):
    """codes, order, score bits and counts of every query against the model: no tolerance"""
    codes, scores, counts = got
    for b, (wc, ws) in enumerate(want):
        c = int(counts[b])
        assert c == len(wc) and np.array_equal(codes[b, :c], wc), (what, b, codes[b, :c], wc)
        assert np.array_equal(scores[b, :c].view(U32), ws.view(U32)), (what, b, scores[b, :c], ws)
