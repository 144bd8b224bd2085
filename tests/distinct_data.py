"""Data and expectations of the "one nearest row per group" tests (tests/test_distinct_cpu.py proves on the CPU what
tests/test_gpu_distinct.py assumes).  The expected answer of every case is the contract sentence executed literally: the oracle's
FULL ranking of the eligible rows (range_data.ranking: oracle.flat_search with k = len, ascending by (distance, id)), walked from
the front, a row kept iff its group code is -1 or no earlier row of the ranking has the same code, cut after k kept rows.

THE FAMILIES
  chunks     65536 x 64: 8192 "documents" of 8 rows each (document centre + 0.05 * gaussian), rows shuffled, code = document.  A
             query lies near a document centre, so its ranking starts with runs of about 8 rows per document: the first 40 ranks
             hold about 5 documents, the first 1024 about 128.  At k = 10 stage A (depth 40) is too shallow and stage B suffices.
  dominated  range_data.separated(): clusters of 1, 40, 300 and 3000 rows around four anchors, query b at anchor b % 4.  Cluster j
             has code j, a background row r has code 4 + r % 50, every 97th background row has no code (-1).  The query at the
             3000-row cluster sees ONE group in its first 1024 ranks: only an exclusion round can answer it.
             "giants" is a second coding of the same rows: the big cluster is one group and the WHOLE background another, so the
             first exclusion round again returns one group only and a second round is needed.
  tied       range_data.tied(): five identical rows nearest to query 0, once sharing a code, once with five codes.
  small      4096 x 32 with a column of 3000 codes: ids beyond the column have no group."""
import numpy as np

import range_data as rd

F32, U64 = np.float32, np.uint64
EUCLID, COSINE, DOT = 0, 1, 2
METRICS = (EUCLID, COSINE, DOT)
MAX_LIST = 1024

CH_N, CH_D, CH_PER, CH_NQ, CH_K = 65536, 64, 8, 12, 10
DOM_K, DOM_BG, DOM_STRIDE = 5, 50, 97
GIANT_BG = 99
SM_N, SM_D, SM_COL, SM_NQ = 4096, 32, 3000, 5


def depth(k, length, stage):
    """vdb_flat_distinct_depth restated (test_distinct_cpu compares it with the ABI's)"""
    return min(length, min(MAX_LIST, max(4 * k, 32))) if stage == 0 else min(length, MAX_LIST)


def chunks():
    """(rows f32[N, D], queries f32[NQ, D], codes i32[N])"""
    def make():
        rng = np.random.default_rng(20261)
        n_docs = CH_N // CH_PER
        centres = rng.standard_normal((n_docs, CH_D)).astype(F32)
        doc = np.repeat(np.arange(n_docs, dtype=np.int32), CH_PER)
        rows = centres[doc] + F32(0.05) * rng.standard_normal((CH_N, CH_D)).astype(F32)
        perm = rng.permutation(CH_N)
        rows, doc = np.ascontiguousarray(rows[perm], dtype=F32), np.ascontiguousarray(doc[perm])
        at = rng.choice(n_docs, CH_NQ, replace=False)
        q = centres[at] + F32(0.05) * rng.standard_normal((CH_NQ, CH_D)).astype(F32)
        return rows, np.ascontiguousarray(q, dtype=F32), doc
    return rd._once("distinct chunks", make)


def dominated_codes():
    """i32[N]: cluster j -> j, background row r -> 4 + r % 50, every 97th background row -> -1"""
    def make():
        rows, _, members = rd.separated()
        r = np.arange(len(rows))
        codes = (4 + r % DOM_BG).astype(np.int32)
        background = np.ones(len(rows), dtype=bool)
        for j, m in enumerate(members):
            codes[m] = j
            background[m] = False
        codes[background & (r % DOM_STRIDE == 0)] = -1
        return codes
    return rd._once("distinct dominated codes", make)


def giant_codes():
    """i32[N]: cluster j -> j, the whole background one group"""
    def make():
        rows, _, members = rd.separated()
        codes = np.full(len(rows), GIANT_BG, dtype=np.int32)
        for j, m in enumerate(members):
            codes[m] = j
        return codes
    return rd._once("distinct giant codes", make)


def tied_codes(shared):
    """i32[N] over range_data.tied(): the five identical rows share code 7 (shared) or have codes 1000..1004; row r else 10 + r % 500"""
    n = len(rd.tied()[0])
    codes = (10 + np.arange(n) % 500).astype(np.int32)
    for i, r in enumerate(rd.TIE_ROWS):
        codes[r] = 7 if shared else 1000 + i
    return codes


def small():
    """(rows f32[4096, 32], queries f32[5, 32], codes i32[3000]): the column is shorter than the id range; some codes are -1"""
    def make():
        rng = np.random.default_rng(20262)
        rows = rng.standard_normal((SM_N, SM_D)).astype(F32)
        q = rows[rng.integers(0, SM_N, SM_NQ)] + F32(0.1) * rng.standard_normal((SM_NQ, SM_D)).astype(F32)
        codes = (np.arange(SM_COL) % 37).astype(np.int32)
        codes[::11] = -1
        return rows, np.ascontiguousarray(q, dtype=F32), codes
    return rd._once("distinct small", make)


def codes_of(ids, codes):
    """the group code of every id: codes[id], -1 at or beyond the column"""
    ids = np.asarray(ids, dtype=U64)
    out = np.full(ids.shape, -1, dtype=np.int32)
    inside = ids < U64(len(codes))
    out[inside] = np.asarray(codes, dtype=np.int32)[ids[inside].astype(np.int64)]
    return out


def kept(rank, codes):
    """bool per rank: the walk of the contract sentence over a whole ranking"""
    c = codes_of(rank[0], codes)
    keep = c == -1
    grouped = np.nonzero(~keep)[0]
    if grouped.size:
        _, first = np.unique(c[grouped], return_index=True)               # (the first occurrence of every code)
        keep[grouped[first]] = True
    return keep, c


def expected(rank, codes, k):
    """(ids u64[m], dists f32[m], codes i32[m]) with m = min(k, groups among the ranking, each -1 row counting as one)"""
    keep, c = kept(rank, codes)
    at = np.nonzero(keep)[0][:int(k)]
    return rank[0][at], rank[1][at], c[at]


def groups_within(rank, codes, depth_):
    """how many rows the walk keeps among the first depth_ ranks"""
    keep, _ = kept((rank[0][:depth_], rank[1][:depth_]), codes)
    return int(keep.sum())


def stage_of(rank, codes, k, length):
    """'A', 'B' or 'C': the stage in which the driver completes this query"""
    for name, stage in (("A", 0), ("B", 1)):
        d = depth(k, length, stage)
        if groups_within(rank, codes, d) >= k or len(rank[0]) < d or d >= length:
            return name
    return "C"


def id_mask(ok):
    """(words u64, bits): the id mask of a bool array by id"""
    ok = np.asarray(ok, dtype=bool)
    packed = np.zeros((ok.size + 63) // 64 * 8 + 8, dtype=np.uint8)
    pb = np.packbits(ok, bitorder="little")
    packed[:pb.size] = pb
    return packed.view(U64), int(ok.size)
