"""The sparse-vector search restated in numpy (include/vdb_flat.h "Sparse vectors"), and a seeded builder of small corpora.

Rows are held densified -- X[row, d] the value, P[row, d] whether the row has index d (an explicit zero has) -- so one query is
a loop over its indices in ascending order with one f32 multiply and one f32 add per step, over all rows at once."""
import numpy as np

VOCAB = 512


class NanScore(Exception):
    pass


def ordered(d):
    """the index's order-preserving map f32 -> u32 (-0.0 in front of +0.0)"""
    b = np.asarray(d, dtype=np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def scores(X, P, query):
    """(touched bool [n], s f32 [n]): s = 0.0f; for d in the shared indices, ascending: s = s + (q_d * x_d)"""
    idx, val = np.asarray(query[0], dtype=np.int64), np.asarray(query[1], dtype=np.float32)
    s = np.zeros(X.shape[0], dtype=np.float32)
    touched = np.zeros(X.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for j in np.argsort(idx, kind="stable"):
            if idx[j] < X.shape[1]:
                m = P[:, idx[j]]
                s[m] = s[m] + val[j] * X[m, idx[j]]
                touched |= m
    return touched, s


def search(ids, X, P, query, k, eligible=None):
    """the k candidates by (distance = -s, id): (ids u64, dists f32); NanScore if an eligible candidate's score is NaN"""
    touched, s = scores(X, P, query)
    if eligible is not None:
        touched &= eligible
    rows = np.flatnonzero(touched)
    if np.isnan(s[rows]).any():
        raise NanScore()
    d = -s[rows]
    order = np.lexsort((ids[rows], ordered(d)))[:k]
    return ids[rows][order], d[order]


def vectors(X, P):
    """the rows as (indices, values) pairs, indices in DESCENDING order (the index sorts on entry)"""
    return [(np.flatnonzero(p)[::-1].astype(np.uint32), x[np.flatnonzero(p)[::-1]]) for x, p in zip(X, P)]


def id_mask(ids, eligible, bits):
    """the id bitmask (u64 words, LSB first) that admits exactly the eligible rows with an id below `bits`"""
    m = np.zeros((bits + 63) // 64, dtype=np.uint64)
    for i in ids[eligible & (ids < bits)]:
        m[int(i) >> 6] |= np.uint64(1) << np.uint64(int(i) & 63)
    return m


def corpus(seed=0, n=6000):
    """ids u64 [n] (shuffled, some >= 2^32), X f32 [n, VOCAB], P bool: 1-40 indices per row out of 0..479 without 100; indices
    7, 8 and 9 each in about 2500 rows; rows 10-13 identical (ids on both sides of 2^32); negative weights; row 20 has an
    explicit zero at index 7; rows 30-39 hold only index 470, which no other row has."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, VOCAB), dtype=np.float32)
    P = np.zeros((n, VOCAB), dtype=bool)
    pool = np.array([d for d in range(480) if d not in (7, 8, 9, 100, 470)])
    for r in range(n):
        P[r, rng.choice(pool, size=rng.integers(1, 38), replace=False)] = True
    for d in (7, 8, 9):
        P[rng.choice(n, size=2500 + 20 * d, replace=False), d] = True
    P[30:40] = False
    P[30:40, 470] = True
    X[P] = rng.standard_normal(int(P.sum())).astype(np.float32)
    X[10] *= 16                                          # (so that a query equal to row 10 ranks the four copies first)
    P[11:14] = P[10]
    X[11:14] = X[10]
    P[20, 7], X[20, 7] = True, 0.0
    ids = (rng.permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(1))
    ids[11], ids[12], ids[13] = (1 << 32) + 5, (1 << 63) + 1, 2      # ids[10] stays small: the tie order crosses 2^32
    return ids, X, P
