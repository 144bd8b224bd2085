"""Data and the model of the recommend-by-best-score tests (tests/test_recommend_best_cpu.py proves on the CPU what
tests/test_gpu_recommend_best.py assumes).  A request is (positive rows, negative rows): ROW numbers of the case's row block, at
least one positive.

THE DEFINITION (definition()).  For every example e one oracle.search_batch(metric, rows, rows[e], k = rows) full ranking gives
d(e, .) over the eligible rows (live, admitted by the mask; the examples are still among them).  Then, in numpy f32:
    dp = d(p_1, .); for i = 2..np: dp = where(d(p_i, .) < dp, d(p_i, .), dp)          (IEEE <: the earlier positive's bits on a tie)
    kept = eligible, id not among the request's example ids, and dp < d(n_j, .) for every j   (a tie or a NaN is a veto)
    dn = the same fold over the negatives, +inf without
and the answer is the kept rows ascending by (ordered dp, id) -- the order the engine's searches give equal distances -- cut to
min(k_b, len).  A NaN d(p_i, x) at an eligible row raises NanDistance.

THE LISTS RESTATEMENT (lists_route()).  Route A of DESIGN.md 4.17 from the same rankings cut at the stage depths: the frontier F
(the smallest last distance of the lists that came back with `depth` entries), the settled entries (d < F), the entry capacity
(WALK_ENTRIES: when the settled entries are more, only those whose ordered distance lies below that of the first entry past the
capacity), the fold per id in list order, the strike, the walk of at most WALK_ROWS rows, the veto, answered / escalate.  It returns
the answers AND the stage every request ended at, from which stats() predicts vdb_flat_recommend_best_stats.

THE FAMILIES (all small; sizes were adjusted on the CPU until the veto families end where they should under Euclid and Cosine):
    fold       recommend's own (600 x dim, dim = 33 is ragged): lengths 1, 2, 5, 9, 64, repeats, an id on both sides, -0.0 elements
    two-blob   900 x 24: positives in two distant clusters, 60 rows around the midpoint; the answer interleaves both clusters
    trap       700 x 16: a negative inside a tight far-away cluster -- nothing is vetoed, stage 0 answers
    veto-100   2000 x 16: a negative beside a positive vetoes the ~100 nearest rows: stage 0 falls short, stage 1 answers
    veto-1500  4000 x 16: a 1500-row cluster around the negative next to the positive: the 1024 nearest are vetoed, the scan answers
    tri        by_id_data.triplicates(): ties exactly at a frontier, and dp == dn for every row (twins on both sides)
    inf        300 x 16 with +inf elements (Euclid): dp = +inf rows at the end of a k > len answer; a positive with +inf is NaN"""
import numpy as np

import oracle
import by_id_data as bd
import recommend_data as rd

F32, U64, U32 = np.float32, np.uint64, np.uint32
EUCLID, COSINE, DOT = bd.EUCLID, bd.COSINE, bd.DOT
METRICS = bd.METRICS
MAX_K = 1024
WALK_ROWS, WALK_ENTRIES = 1024, 4096
K = 10
AUTO, LISTS, SCAN = 0, 1, 2
STAGE_SCAN = 2

_once = bd._once


class NanDistance(Exception):
    pass


def ordered(d):
    """the engine's order-preserving map f32 -> u32 (-0.0 in front of +0.0)"""
    b = np.asarray(d, dtype=F32).view(U32)
    return np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)


def depth(k, m, n_live, stage):
    if stage == 0:
        return min(n_live, min(1024, max(2 * (min(k, 1024) + min(m, 1024)), 32)))
    return min(n_live, 1024) if stage == 1 else 0


# ------------------------------------------------------------------ d(e, .)
def ranking(key, metric, rows, e, ids, elig):
    """(ids, dists) of the full ranking of example row e over the eligible rows, and the distances scattered by row (+inf at rows
    that are not eligible: they are never read).  None for a ranking the oracle refuses with a NaN."""
    def make():
        n = len(rows)
        try:
            (oi, od), = oracle.search_batch(metric, rows, rows[[e]], n, ids=ids, live=elig)
        except oracle.OracleError as err:
            if "NaN" not in str(err):
                raise
            return None
        own = np.arange(n, dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
        at = {int(x): i for i, x in enumerate(own) if elig is None or elig[i]}
        table = np.full(n, np.inf, dtype=F32)
        table[[at[int(x)] for x in oi]] = od
        return oi, od, table
    return _once(("rbrank", key, metric, int(e)), make)


def pair_table(metric, rows, e, elig):
    """d(e, .) row by row, NaN kept: for a NEGATIVE whose ranking holds a NaN (a veto at that row, not an error)"""
    out = np.full(len(rows), np.inf, dtype=F32)
    for i in range(len(rows)):
        if elig is None or elig[i]:
            out[i] = F32(oracle.distance(metric, rows[e], rows[i]))
    return out


def _tables(key, metric, rows, req, ids, elig):
    p, n = req
    pt = []
    for e in p:
        r = ranking(key, metric, rows, e, ids, elig)
        if r is None:
            raise NanDistance((key, metric, e))
        pt.append(r)
    nt = []
    for e in n:
        r = ranking(key, metric, rows, e, ids, elig)
        nt.append(r[2] if r is not None else pair_table(metric, rows, e, elig))
    return pt, nt


def _row_facts(rows, req, ids, elig, pt, nt):
    """dp, dn, kept per row of the block"""
    n = len(rows)
    own = np.arange(n, dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    p, ng = req
    dp = pt[0][2].copy()
    for r in pt[1:]:
        dp = np.where(r[2] < dp, r[2], dp)
    kept = np.ones(n, dtype=bool) if elig is None else np.asarray(elig, dtype=bool).copy()
    kept &= ~np.isin(own, own[list(p) + list(ng)])
    dn = np.full(n, np.inf, dtype=F32)
    with np.errstate(invalid="ignore"):
        for j, t in enumerate(nt):
            kept &= dp < t
            dn = t.copy() if j == 0 else np.where(t < dn, t, dn)
    return own, dp, dn, kept


def _answer(own, dp, dn, rows_kept, kb):
    """the rows `rows_kept` (row numbers) ascending by (ordered dp, id), cut to kb"""
    rows_kept = np.asarray(rows_kept, dtype=np.int64)
    o = np.lexsort((own[rows_kept], ordered(dp[rows_kept])))[:kb]
    sel = rows_kept[o]
    return own[sel], dp[sel], dn[sel]


def _ks(requests, k, n_live):
    ks = [int(k)] * len(requests) if np.isscalar(k) else [int(x) for x in k]
    kcut = min(max(ks) if ks else 0, n_live)
    return [min(x, kcut) for x in ks], kcut


def n_live_of(rows, live):
    return len(rows) if live is None else int(np.asarray(live, dtype=bool).sum())


def _elig(live, mask):
    if live is None and mask is None:
        return None
    e = np.ones(len(live if live is not None else mask), dtype=np.uint8)
    if live is not None:
        e &= np.asarray(live, dtype=np.uint8)
    if mask is not None:
        e &= np.asarray(mask, dtype=np.uint8)
    return e


def definition(key, metric, rows, requests, k, ids=None, live=None, mask=None, tables=None):
    """per request (ids, dp, dn).  live: the stored rows (len counts them); mask: the rows the caller's mask admits.  tables: what
    gives d(e, .) in place of _tables -- same arguments, same result, NOT cached by case name (tests/lifecycle.py: a life of the
    index changes the rows under one name, so its model passes rankings of its own, kept until the next mutation)"""
    elig = _elig(live, mask)
    ks, _ = _ks(requests, k, n_live_of(rows, live))
    out = []
    for req, kb in zip(requests, ks):
        pt, nt = (tables or _tables)(key, metric, rows, req, ids, elig)
        own, dp, dn, kept = _row_facts(rows, req, ids, elig, pt, nt)
        out.append(_answer(own, dp, dn, np.nonzero(kept)[0], kb))
    return out


# ------------------------------------------------------------------ route A, restated
def _walk(req, own_of, pt, D):
    """the candidates of one request at depth D: (ids in walk order, open)"""
    p, ng = req
    lists = [(r[0][:D], r[1][:D]) for r in pt]
    full = [len(oi) == D for oi, _ in lists]
    fronts = [od[-1] for (oi, od), f in zip(lists, full) if f]
    is_open = bool(fronts)
    ent = []                                                       # (ordered d, id, list, d)
    F = None
    if fronts:
        F = fronts[0]
        for f in fronts[1:]:
            if f < F:
                F = f
    for i, (oi, od) in enumerate(lists):
        s = np.ones(len(od), dtype=bool) if F is None else od < F
        for x, d, o in zip(oi[s], od[s], ordered(od[s])):
            ent.append((int(o), int(x), i, d))
    if len(ent) > WALK_ENTRIES:
        ent.sort(key=lambda t: (t[0], t[1], t[2]))
        cut = ent[WALK_ENTRIES][0]
        ent = [t for t in ent if t[0] < cut]
        is_open = True
    best = {}
    for o, x, i, d in sorted(ent, key=lambda t: t[2]):             # list order: the fold
        if x not in best or d < best[x][1]:
            best[x] = (o, d)
    ex = set(int(own_of[e]) for e in list(p) + list(ng))
    walk = sorted((o, x) for x, (o, d) in best.items() if x not in ex)
    if len(walk) > WALK_ROWS:
        walk = walk[:WALK_ROWS]
        is_open = True
    return [x for _, x in walk], is_open


def lists_route(key, metric, rows, requests, k, ids=None, live=None, mask=None, route=AUTO, tables=None):
    """(answers, stages, stats): the engine's routes restated on the oracle's rankings (tables: as in definition())"""
    n = len(rows)
    elig = _elig(live, mask)
    nl = n_live_of(rows, live)
    ks, kcut = _ks(requests, k, nl)
    own = np.arange(n, dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    row_of = {int(x): i for i, x in enumerate(own) if live is None or live[i]}
    mmax = max(len(p) + len(g) for p, g in requests)
    D0, D1 = depth(kcut, mmax, nl, 0), depth(kcut, mmax, nl, 1)
    use_lists = route == LISTS or (route == AUTO and D0 < nl)
    depths = ([D0] + ([D1] if D1 > D0 else [])) if use_lists else []
    answers, stages, searches = [], [], 0
    for req, kb in zip(requests, ks):
        pt, nt = (tables or _tables)(key, metric, rows, req, ids, elig)
        own_, dp, dn, kept = _row_facts(rows, req, ids, elig, pt, nt)
        done = None
        for stage, D in enumerate(depths):
            searches += len(req[0])
            walk, is_open = _walk(req, own, pt, D)
            cand = [row_of[x] for x in walk]
            good = [r for r in cand if kept[r]]
            if len(good) >= kb or not is_open:
                # (the walk is in (ordered dp, id) order already; _answer sorts the same rows by the same key)
                done = (stage, _answer(own, dp, dn, good, kb))
                break
        if done is None:
            done = (STAGE_SCAN, _answer(own, dp, dn, np.nonzero(kept)[0], kb))
        stages.append(done[0])
        answers.append(done[1])
    st = [len(requests), sum(len(p) + len(g) for p, g in requests), stages.count(0), stages.count(1), stages.count(STAGE_SCAN),
          D0, searches, 0]
    return answers, stages, st


def expected(key, metric, rows, requests, k, ids=None, live=None, mask=None, route=AUTO):
    """(answers by the definition, predicted stats of the route), cached: the GPU tests share it"""
    def make():
        want = definition(key, metric, rows, requests, k, ids=ids, live=live, mask=mask)
        _, stages, st = lists_route(key, metric, rows, requests, k, ids=ids, live=live, mask=mask, route=route)
        return tuple(want), tuple(stages), tuple(st)
    return _once(("rbexp", key, metric, route, repr(k)), make)


def same(a, b, what=""):
    for i, ((ai, ad, an), (bi, bd_, bn)) in enumerate(zip(a, b)):
        assert np.array_equal(ai, bi), (what, i, ai, bi)
        assert np.array_equal(ad.view(U32), bd_.view(U32)), (what, i)
        assert np.array_equal(an.view(U32), bn.view(U32)), (what, i)
    assert len(a) == len(b), what


def check(got, want, what=""):
    """(ids, dists, neg_dists, counts) of the engine against the definition: ids, order, dp bits, dn bits, counts"""
    gi, gd, gn, gc = got
    assert len(gc) == len(want), (what, len(gc), len(want))
    for b, (oi, od, on) in enumerate(want):
        c = int(gc[b])
        assert c == len(oi), (what, b, c, len(oi))
        assert np.array_equal(gi[b, :c], oi), (what, b, gi[b, :c], oi)
        assert np.array_equal(gd[b, :c].view(U32), od.view(U32)), (what, b, gd[b, :c], od)
        assert np.array_equal(gn[b, :c].view(U32), on.view(U32)), (what, b, gn[b, :c], on)


split = rd.split


# ------------------------------------------------------------------ the families: (rows, ids or None, requests)
def fold_family(dim):
    return rd.fold_rows(dim), None, rd.fold_requests()


BLOB_N, BLOB_D, BLOB_EACH, BLOB_MID = 900, 24, 300, 60


def two_blob():
    """rows [0, 300) around +c, [300, 600) around -c, [600, 660) around the midpoint 0, the rest far away.  How evenly the answer
    draws from the two clusters depends on how crowded the positives' neighbourhoods are: the seed was found by trying a few against
    the model, the CPU test asserts the property."""
    def make():
        rng = np.random.default_rng(20293)
        c = np.zeros(BLOB_D, dtype=F32)
        c[0] = 6.0
        rows = rng.standard_normal((BLOB_N, BLOB_D)).astype(F32) * F32(0.5)
        rows[:BLOB_EACH] += c
        rows[BLOB_EACH:2 * BLOB_EACH] -= c
        rows[2 * BLOB_EACH + BLOB_MID:, 1] += F32(40.0)
        reqs = (((5, 17, BLOB_EACH + 3, BLOB_EACH + 40), ()), ((11, BLOB_EACH + 11), (2 * BLOB_EACH + BLOB_MID + 1,)))
        return np.ascontiguousarray(rows), reqs
    rows, reqs = _once("rbblob", make)
    return rows, None, reqs


def trap():
    """rows [0, 550): a cloud around 0; [550, 700): a tight cluster (sigma 0.01) around 50 e_1; the negative is row 600 inside it"""
    def make():
        rng = np.random.default_rng(20282)
        rows = rng.standard_normal((700, 16)).astype(F32)
        rows[550:] *= F32(0.01)
        rows[550:, 0] += F32(50.0)
        return np.ascontiguousarray(rows), (((3, 77), (600,)),)
    rows, reqs = _once("rbtrap", make)
    return rows, None, reqs


VETO_D = 16
VETO100_N, VETO100_CLUSTER = 2000, 100
VETO1500_N, VETO1500_CLUSTER = 4000, 1500


def _veto(n, cluster, seed):
    """row 0: the positive, c + 0.3 e_1; row 1: the negative, c; rows [2, 2 + cluster): sigma 0.02 around c; the rest sigma 2 around c
    (c = 5 in every coordinate: directions mean something under Cosine)"""
    rng = np.random.default_rng(seed)
    c = np.full(VETO_D, 5.0, dtype=F32)
    rows = rng.standard_normal((n, VETO_D)).astype(F32)
    rows[2:2 + cluster] *= F32(0.02)
    rows[2 + cluster:] *= F32(2.0)
    rows += c
    rows[0] = c
    rows[0, 0] += F32(0.3)
    rows[1] = c
    return np.ascontiguousarray(rows), (((0,), (1,)),)


def veto100():
    rows, reqs = _once("rbveto100", lambda: _veto(VETO100_N, VETO100_CLUSTER, 20283))
    return rows, None, reqs


def veto1500():
    rows, reqs = _once("rbveto1500", lambda: _veto(VETO1500_N, VETO1500_CLUSTER, 20284))
    return rows, None, reqs


def tri():
    """request 0: two positives, no negative -- depth 32 cuts a triple: ties exactly at the frontier; request 1: the twins of one
    vector on both sides -- dp == dn at every row, everything is vetoed; request 2: a positive, a far negative"""
    rows, ids = bd.triplicates()
    reqs = (((rd.tri_row(5, 0), rd.tri_row(300, 1)), ()), ((rd.tri_row(40, 0),), (rd.tri_row(40, 2),)), ((rd.tri_row(9, 2),), (rd.tri_row(600, 0),)))
    return rows, ids, reqs


INF_N = 300
INF_ROWS = (50, 120, 121)


def inf_rows():
    def make():
        rows = bd.scaled(INF_N, 16).copy()
        for r in INF_ROWS:
            rows[r, 3] = F32(np.inf)
        return np.ascontiguousarray(rows)
    return _once("rbinf", make)


def inf_family():
    """Euclid only.  Finite positives: the +inf rows have dp = +inf and close a k > len answer"""
    return inf_rows(), None, (((4, 200), (9,)), ((7,), ()))


def inf_nan_request():
    """a positive with a +inf element: inf - inf at the other +inf rows (and at itself) is NaN"""
    return (((INF_ROWS[0],), ()),)


FAMILIES = {
    "fold33": lambda: fold_family(33), "fold64": lambda: fold_family(64), "blob": two_blob, "trap": trap,
    "veto100": veto100, "veto1500": veto1500, "tri": tri,
}
