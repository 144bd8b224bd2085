"""Data and expectations of the "k nearest groups with up to g rows of each" tests (tests/test_per_group_cpu.py proves on the CPU
what tests/test_gpu_per_group.py assumes).  The expected answer of every case is the contract executed literally: the oracle's
FULL ranking of the eligible rows (range_data.ranking), the groups that distinct_data's walk keeps, and as the members of a group
with code c >= 0 the first g positions of the ranking whose code is c; a row with code -1 is its own group of one.

THE SCATTERED FAMILY (65536 x 64, the screening tier's row floor): 8192 documents of 8 rows.  Row 0 of a document lies at the
document's centre + 0.05 * gaussian; rows 1..7 are independent unit gaussians, so they lie ANYWHERE in a query's ranking.  Rows
shuffled, code = document.  A query at a centre finds the document by its row 0; the 2nd and 3rd best chunk of the document are
ordinary rows thousands of ranks deep -- no plain search, however deep (1024 at most), returns them."""
import numpy as np

import distinct_data as dd
import range_data as rd

F32, U64, I32 = np.float32, np.uint64, np.int32
METRICS = dd.METRICS
MAX_SIZE = 32
SCAN_CAP = 131072                                                  # rows of a member list the fill takes by default
LOW_CAP = 1024                                                     # what the tests lower it to: lists above it take the giants' route
NONE = 0xFFFFFFFF

SC_N, SC_D, SC_PER, SC_NQ, SC_K, SC_G = 65536, 64, 8, 12, 10, 3
ODD_N, ODD_D, ODD_NQ = 2048, 33, 4


def scattered():
    """(rows f32[N, D], queries f32[NQ, D], codes i32[N])"""
    def make():
        rng = np.random.default_rng(20271)
        n_docs = SC_N // SC_PER
        centres = rng.standard_normal((n_docs, SC_D)).astype(F32)
        doc = np.repeat(np.arange(n_docs, dtype=I32), SC_PER)
        rows = rng.standard_normal((SC_N, SC_D)).astype(F32)
        rows[::SC_PER] = centres + F32(0.05) * rng.standard_normal((n_docs, SC_D)).astype(F32)
        perm = rng.permutation(SC_N)
        rows, doc = np.ascontiguousarray(rows[perm], dtype=F32), np.ascontiguousarray(doc[perm])
        at = rng.choice(n_docs, SC_NQ, replace=False)
        q = centres[at] + F32(0.05) * rng.standard_normal((SC_NQ, SC_D)).astype(F32)
        return rows, np.ascontiguousarray(q, dtype=F32), doc
    return rd._once("per group scattered", make)


def odd():
    """(rows f32[2048, 33], queries f32[4, 33], codes i32[2048]): the row pitch is not the dimension; 64 rows per code, every 9th none"""
    def make():
        rng = np.random.default_rng(20272)
        rows = rng.standard_normal((ODD_N, ODD_D)).astype(F32)
        q = rows[rng.integers(0, ODD_N, ODD_NQ)] + F32(0.1) * rng.standard_normal((ODD_NQ, ODD_D)).astype(F32)
        codes = (np.arange(ODD_N) % 32).astype(I32)
        codes[::9] = -1
        return rows, np.ascontiguousarray(q, dtype=F32), codes
    return rd._once("per group odd", make)


def expected(rank, codes, k, g):
    """[(code, ids u64[m], dists f32[m])] per group, nearest group first, m = min(g, eligible rows of the code) (1 for code -1)"""
    keep, c = dd.kept(rank, codes)
    out = []
    for at in np.nonzero(keep)[0][:int(k)]:
        code = int(c[at])
        pos = np.array([at]) if code == -1 else np.nonzero(c == code)[0][:int(g)]
        assert pos[0] == at, "a group's first member is its representative"
        out.append((code, rank[0][pos], rank[1][pos]))
    return out


def member_ranks(rank, codes, k, g):
    """the 0-based position in the full ranking of every expected member, per group"""
    keep, c = dd.kept(rank, codes)
    return [np.array([at]) if c[at] == -1 else np.nonzero(c == c[at])[0][:int(g)] for at in np.nonzero(keep)[0][:int(k)]]


def routes(ranks, codes, ks, g, cap=SCAN_CAP):
    """what vdb_flat_per_group_stats reports for these rankings: [groups returned, pairs filled, pairs of a giant, wanted codes,
    member rows listed, pair distances evaluated].  A code's list holds the eligible rows (those of the ranking) with that code."""
    groups = filled = giant = evaluated = 0
    size = {}
    for b, rank in enumerate(ranks):
        kb = int(ks if np.isscalar(ks) else ks[b])
        keep, c = dd.kept(rank, codes)
        at = np.nonzero(keep)[0][:kb]
        groups += len(at)
        if g == 1:
            continue
        for code in c[at]:
            if code < 0:
                continue
            e = int((c == code).sum())
            size[int(code)] = e
            if e <= cap:
                filled += 1
                evaluated += e
            else:
                giant += 1
    if g == 1:
        wanted = {int(x) for b, rank in enumerate(ranks) for x in dd.expected(rank, codes, int(ks if np.isscalar(ks) else ks[b]))[2] if x >= 0}
        return [groups, 0, 0, len(wanted), 0, 0]
    return [groups, filled, giant, len(size), sum(e for e in size.values() if e <= cap), evaluated]


def plan(codes, kept, ks=None):
    """vdb_flat_debug_per_group_plan restated with numpy.unique: (wanted i32[U], index u32[nq, kmax])"""
    codes = np.asarray(codes, dtype=I32)
    nq, kmax = codes.shape
    count = np.minimum(np.asarray(kept, dtype=np.int64), kmax)
    if ks is not None:
        count = np.minimum(count, np.asarray(ks, dtype=np.int64))
    counted = (np.arange(kmax)[None, :] < count[:, None]) & (codes >= 0)
    wanted = np.unique(codes[counted]).astype(I32)
    index = np.full((nq, kmax), NONE, dtype=np.uint32)
    index[counted] = np.searchsorted(wanted, codes[counted]).astype(np.uint32)
    return wanted, index
