"""The int8 index's definition (include/vdb_flat.h "Int8 vectors") in numpy: integer sums in int64, the distance through np.float32
operations in the stated order, the answer by np.lexsort over (distance bits in total order, id as uint64)."""
import numpy as np

F32, U64 = np.float32, np.uint64
EUCLID, COSINE, DOT = 0, 1, 2


class ZeroNorm(Exception):
    """a live zero-norm row or a zero-norm query under Cosine: the call fails with VDB_ERR_INVALID_VECTOR"""


def ordered(d):
    b = np.ascontiguousarray(d, dtype=F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def distances(metric, q, rows):
    """f32 [n]: the distances of the int8 rows [n, dim] from the int8 query [dim]"""
    q, x = q.astype(np.int64), rows.astype(np.int64)
    s, nq, nx = x @ q, q @ q, (x * x).sum(axis=1)
    if metric == DOT:
        return -s.astype(F32)
    if metric == EUCLID:
        return np.sqrt((nq + nx - 2 * s).astype(F32))
    sim = s.astype(F32) / (np.sqrt(F32(nq)) * np.sqrt(nx.astype(F32)))
    return F32(1.0) - np.clip(sim, F32(-1.0), F32(1.0))


def search(metric, ids, rows, live, queries, ks, eligible=None):
    """[(ids u64, dists f32), ...] per query over the live (and eligible) rows; ks an int or one k per query"""
    ids, live = np.asarray(ids, dtype=U64), np.asarray(live, dtype=bool)
    ks = np.full(len(queries), ks) if np.isscalar(ks) else np.asarray(ks)
    if metric == COSINE and live.any() and ks.max(initial=0) > 0:
        if not rows[live].any(axis=1).all() or not queries.any(axis=1).all():
            raise ZeroNorm
    keep = np.flatnonzero(live if eligible is None else live & eligible)
    out = []
    for q, k in zip(queries, ks):
        d = distances(metric, q, rows[keep])
        order = np.lexsort((ids[keep], ordered(d)))[:int(k)]
        out.append((ids[keep][order], d[order]))
    return out


def check(ix, metric, ids, rows, live, queries, ks, eligible=None, **mask):
    """ix.search_batch_arrays against search(): ids, order, distance bits and counts"""
    want = search(metric, ids, rows, live, queries, ks, eligible)
    got_ids, got_d, counts = ix.search_batch_arrays(queries, ks, **mask)
    for b, (wi, wd) in enumerate(want):
        assert counts[b] == wi.size, (b, counts[b], wi.size)
        assert np.array_equal(got_ids[b, :wi.size], wi), (b, got_ids[b, :wi.size][:8], wi[:8])
        assert np.array_equal(got_d[b, :wi.size].view(np.uint32), wd.view(np.uint32)), (b, got_d[b, :wi.size][:8], wd[:8])
    return got_ids, got_d, counts


def random_rows(rng, n, dim, metric):
    """full-range int8 rows; under Cosine a row of zeros gets a 1 (a zero norm is an error there)"""
    x = rng.integers(-128, 128, size=(n, dim), dtype=np.int8)
    if metric == COSINE:
        x[~x.any(axis=1), 0] = 1
    return x
