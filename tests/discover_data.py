"""Data and the model of the discovery-search tests (tests/test_discover_cpu.py proves on the CPU what tests/test_gpu_discover.py
assumes).  A request is (target row, ((positive row, negative row), ...)): ROW numbers of the case's row block, 0 to 16 pairs.

THE DEFINITION (definition()).  For every example e one oracle.search_batch(metric, rows, rows[e], k = rows) full ranking gives
d(e, .) over the eligible rows (live, admitted by the mask; the examples are still among them); a context example whose ranking
the oracle refuses with a NaN is evaluated pair by pair with oracle.distance instead.  Then, in numpy f32:
    rank = sum over the pairs of (d(p_i, .) < d(n_i, .))          (IEEE <: a tie or a NaN on either side does not count)
    eligible = live, admitted, id not among {t, p_i, n_i}
and the answer is the eligible rows by (rank descending, ordered d(t, .) ascending, id ascending) -- the order the engine's
searches give equal distances -- cut to min(k_b, len).  A NaN d(t, x) at a live admitted row raises NanDistance.

THE LISTS RESTATEMENT (lists_route()).  The list route of DESIGN.md 4.18 from the target's ranking cut at the stage depths
(depth(): min(len, min(1024, max(2 k 2^P' + 2 P' + 1, 64))) with P' = min(P, 10), then min(len, 1024)): the strike of the example set, the ranks of the
candidates, ANSWERED when k_b candidates have rank P (the first k_b of them) or when the list is complete (the search returned
fewer than its depth, or the depth is the whole index: the stable sort by rank descending), otherwise the next stage, at last
the scan (the definition).  It returns the answers AND the stage every request ended at, from which the stats are predicted.

THE FAMILIES (all small; each is (rows, ids or None, requests, k); sizes were adjusted on the CPU until every family ends at the
stage its name says under Euclid and Cosine in the automatic route -- tests/test_discover_cpu.py asserts it):
    ragged     600 x 33 (recommend's fold rows, -0.0 elements): P = 0, 1, 3, 16
    loose      700 x 16 (recommend-by-best's trap rows): every negative sits in a far tight cluster -- stage 0 answers
    half       2000 x 16: the pair (c + 0.6 e_1, c) cuts away the ~100 rows around c nearest the target c + 0.3 e_1 -- stage 1 answers
    deep       4000 x 16: the same with 1500 rows around c -- more than 1024 of the nearest fail the pair, the scan answers
    contra     the half rows: pairs (a, b) and (b, a) beside a third that few rows satisfy: no row has rank P, the scan answers and
               its answer mixes rank levels
    tri        by_id_data.triplicates(): twins as a pair (d(p, x) == d(n, x) everywhere), equal target distances decided by id, a
               list frontier inside a triple
    repeats    ragged rows: a pair with both ids equal, a pair twice, the target as a context example, an id on both sides
    inf        300 x 16 with +inf elements (Euclid): a context example with +inf gives NaN pair distances (not satisfied, no
               error); a target with +inf is NanDistance"""
import numpy as np

import oracle
import by_id_data as bd
import recommend_data as rd
import recommend_best_data as rb

F32, U64, U32 = np.float32, np.uint64, np.uint32
EUCLID, COSINE, DOT = bd.EUCLID, bd.COSINE, bd.DOT
METRICS = bd.METRICS
MAX_K, MAX_PAIRS = 1024, 16
K = 10
AUTO, LISTS, SCAN = 0, 1, 2
STAGE_SCAN = 2

_once = bd._once
NanDistance = rb.NanDistance
ordered = rb.ordered


def depth(k, P, n_live, stage):
    if stage == 0:
        Pc = min(P, 10)
        return min(n_live, min(1024, max(2 * min(k, 1024) * 2 ** Pc + 2 * Pc + 1, 64)))
    return min(n_live, 1024) if stage == 1 else 0


def examples(req):
    """the rows of a request as the engine lays them out: t, p_1, n_1, p_2, n_2, ..."""
    t, pairs = req
    return [int(t)] + [int(e) for pn in pairs for e in pn]


# ------------------------------------------------------------------ d(e, .)
def _tables(key, metric, rows, req, ids, elig):
    """(ranking of the target, [(d(p_i, .), d(n_i, .)) by row])"""
    t, pairs = req
    tr = rb.ranking(key, metric, rows, int(t), ids, elig)
    if tr is None:
        raise NanDistance((key, metric, t))

    def table(e):
        r = rb.ranking(key, metric, rows, int(e), ids, elig)
        return r[2] if r is not None else rb.pair_table(metric, rows, int(e), elig)
    return tr, [(table(p), table(n)) for p, n in pairs]


def _row_facts(rows, req, ids, elig, tr, pt):
    """own ids, d(t, .), rank, eligible -- per row of the block"""
    n = len(rows)
    own = np.arange(n, dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    ok = np.ones(n, dtype=bool) if elig is None else np.asarray(elig, dtype=bool).copy()
    ok &= ~np.isin(own, own[examples(req)])
    rank = np.zeros(n, dtype=U32)
    with np.errstate(invalid="ignore"):
        for dp, dn in pt:
            rank += (dp < dn).astype(U32)
    return own, tr[2], rank, ok


def _answer(own, dt, rank, sel, kb):
    """the rows `sel` (row numbers) by (rank descending, ordered d(t, .), id), cut to kb"""
    sel = np.asarray(sel, dtype=np.int64)
    o = np.lexsort((own[sel], ordered(dt[sel]), -rank[sel].astype(np.int64)))[:kb]
    s = sel[o]
    return own[s], dt[s], rank[s]


_ks, n_live_of, _elig = rb._ks, rb.n_live_of, rb._elig


def definition(key, metric, rows, requests, k, ids=None, live=None, mask=None):
    """per request (ids, d(t, .), ranks).  live: the stored rows (len counts them); mask: the rows the caller's mask admits"""
    elig = _elig(live, mask)
    ks, _ = _ks(requests, k, n_live_of(rows, live))
    out = []
    for req, kb in zip(requests, ks):
        tr, pt = _tables(key, metric, rows, req, ids, elig)
        own, dt, rank, ok = _row_facts(rows, req, ids, elig, tr, pt)
        out.append(_answer(own, dt, rank, np.nonzero(ok)[0], kb))
    return out


# ------------------------------------------------------------------ the list route, restated
def lists_route(key, metric, rows, requests, k, ids=None, live=None, mask=None, route=AUTO):
    """(answers, stages, stats): the engine's routes restated on the oracle's rankings"""
    n = len(rows)
    elig = _elig(live, mask)
    nl = n_live_of(rows, live)
    ks, kcut = _ks(requests, k, nl)
    total = sum(len(examples(r)) for r in requests)
    own = np.arange(n, dtype=U64) if ids is None else np.asarray(ids, dtype=U64)
    if kcut == 0 or not requests:
        zero = (np.zeros(0, dtype=U64), np.zeros(0, dtype=F32), np.zeros(0, dtype=U32))
        return [zero] * len(requests), [None] * len(requests), [len(requests), total, 0, 0, 0, 0, 0, 0]
    row_of = {int(x): i for i, x in enumerate(own) if live is None or live[i]}
    pmax = max(len(p) for _, p in requests)
    D0, D1 = depth(kcut, pmax, nl, 0), depth(kcut, pmax, nl, 1)
    use_lists = route == LISTS or (route == AUTO and D0 < nl)
    depths = ([D0] + ([D1] if D1 > D0 else [])) if use_lists else []
    answers, stages = [], [None] * len(requests)
    facts = []
    for req in requests:
        tr, pt = _tables(key, metric, rows, req, ids, elig)
        facts.append((tr, _row_facts(rows, req, ids, elig, tr, pt)))
    answers = [None] * len(requests)
    todo, searches = list(range(len(requests))), 0
    for stage, D in enumerate(depths):                             # (a stage runs for the requests the one before left over)
        left = []
        for b in todo:
            req, kb = requests[b], ks[b]
            tr, (own_, dt, rank, ok) = facts[b]
            searches += 1
            raw = tr[0][:D]
            complete = len(raw) < D or D >= nl
            ex = set(int(own[e]) for e in examples(req))
            cand = [row_of[int(x)] for x in raw if int(x) not in ex]
            P = len(req[1])
            full = [r for r in cand if rank[r] == P]
            if len(full) >= kb:
                sel = np.asarray(full[:kb], dtype=np.int64)
            elif complete:
                c = np.asarray(cand, dtype=np.int64)
                sel = c[np.argsort(-rank[c].astype(np.int64), kind="stable")][:kb]
            else:
                left.append(b)
                continue
            stages[b] = stage
            answers[b] = (own[sel], dt[sel], rank[sel])
        todo = left
    for b in todo:
        tr, (own_, dt, rank, ok) = facts[b]
        stages[b] = STAGE_SCAN
        answers[b] = _answer(own, dt, rank, np.nonzero(ok)[0], ks[b])
    st = [len(requests), total, stages.count(0), stages.count(1), stages.count(STAGE_SCAN), D0, searches, 0]
    return answers, stages, st


def expected(key, metric, rows, requests, k, ids=None, live=None, mask=None, route=AUTO):
    """(answers by the definition, stages and predicted stats of the route), cached: the GPU tests share it"""
    def make():
        want = definition(key, metric, rows, requests, k, ids=ids, live=live, mask=mask)
        _, stages, st = lists_route(key, metric, rows, requests, k, ids=ids, live=live, mask=mask, route=route)
        return tuple(want), tuple(stages), tuple(st)
    return _once(("discexp", key, metric, route, repr(k)), make)


def same(a, b, what=""):
    assert len(a) == len(b), what
    for i, ((ai, ad, ar), (bi, bd_, br)) in enumerate(zip(a, b)):
        assert np.array_equal(ai, bi), (what, i, ai, bi)
        assert np.array_equal(ad.view(U32), bd_.view(U32)), (what, i)
        assert np.array_equal(ar, br), (what, i, ar, br)


def check(got, want, what=""):
    """(ids, dists, ranks or None, counts) of the engine against the definition: ids, order, distance bits, ranks, counts"""
    gi, gd, gr, gc = got
    assert len(gc) == len(want), (what, len(gc), len(want))
    for b, (oi, od, orank) in enumerate(want):
        c = int(gc[b])
        assert c == len(oi), (what, b, c, len(oi))
        assert np.array_equal(gi[b, :c], oi), (what, b, gi[b, :c], oi)
        assert np.array_equal(gd[b, :c].view(U32), od.view(U32)), (what, b, gd[b, :c], od)
        if gr is not None:
            assert np.array_equal(gr[b, :c], orank), (what, b, gr[b, :c], orank)


def split(requests, ids=None):
    """the (targets, pair lists) GpuFlatIndex.discover_batch takes"""
    name = (lambda r: int(r)) if ids is None else (lambda r: int(ids[r]))
    return [name(t) for t, _ in requests], [[(name(p), name(n)) for p, n in pairs] for _, pairs in requests]


# ------------------------------------------------------------------ the families: (rows, ids or None, requests, k)
def ragged():
    def make():
        rng = np.random.default_rng(20301)
        pick = lambda m: [int(x) for x in rng.choice(np.arange(2, rd.FOLD_N), m, replace=False)]
        pairs = lambda m: tuple((a, b) for a, b in zip(pick(m), pick(m)))
        reqs = ((0, ()), (17, pairs(1)), (301, pairs(3)), (599, pairs(16)), (1, ((0, 5),)), (44, pairs(16)))
        assert sorted(len(p) for _, p in reqs) == [0, 1, 1, 3, 16, 16]
        return reqs
    return rd.fold_rows(33), None, _once("discragged", lambda: (make(),))[0], K


def loose():
    rows, _, _ = rb.trap()
    return rows, None, ((3, ((77, 600), (10, 650), (200, 610))), (500, ((20, 699),))), K


CUT_D = 16
HALF_N, HALF_CLUSTER = 2000, 100
DEEP_N, DEEP_CLUSTER = 4000, 1500


def _cut(n, cluster, seed):
    """row 0: the target, c + 0.3 e_1; row 1: the negative, c; row 2: the positive, c + 0.6 e_1; rows [3, 3 + cluster): sigma 0.02
    around c -- the rows nearest the target, every one nearer to the negative --; the rest sigma 2 around c (c = 5 in every
    coordinate: directions mean something under Cosine)"""
    rng = np.random.default_rng(seed)
    c = np.full(CUT_D, 5.0, dtype=F32)
    rows = rng.standard_normal((n, CUT_D)).astype(F32)
    rows[3:3 + cluster] *= F32(0.02)
    rows[3 + cluster:] *= F32(2.0)
    rows += c
    rows[0] = c
    rows[0, 0] += F32(0.3)
    rows[1] = c
    rows[2] = c
    rows[2, 0] += F32(0.6)
    return np.ascontiguousarray(rows)


def half_rows():
    return _once("dischalf", lambda: _cut(HALF_N, HALF_CLUSTER, 20302))


def half():
    return half_rows(), None, ((0, ((2, 1),)),), K


def deep():
    return _once("discdeep", lambda: _cut(DEEP_N, DEEP_CLUSTER, 20303)), None, ((0, ((2, 1),)),), K


CONTRA_K = 100


def contra():
    """(a, b) and (b, a) contradict each other: rank 3 does not exist.  The third pair's positive is the row farthest from c, its
    negative c itself: few rows satisfy it, so the first CONTRA_K rows hold rank 2 and rank 1."""
    rows = half_rows()
    far = int(np.argmax(((rows - rows[1]) ** 2).sum(axis=1)))
    return rows, None, ((500, ((700, 900), (900, 700), (far, 1))), (0, ((2, 1),))), CONTRA_K


def tri():
    """request 0: twins as the pair -- d(p, x) == d(n, x) bit for bit at every row, nobody has rank 1 --; request 1: no pair, depth
    64 cuts a triple of equal distances; request 2: two ordinary pairs, triples share (rank, distance) and the id decides"""
    rows, ids = bd.triplicates()
    t = rd.tri_row
    reqs = ((t(5, 0), ((t(40, 0), t(40, 2)),)), (t(300, 1), ()), (t(9, 2), ((t(9, 0), t(600, 0)), (t(77, 1), t(123, 2)))))
    return rows, ids, reqs, K


def repeats():
    """a pair with both ids equal (never satisfied), the same pair twice (counts twice), the target as a positive and as a
    negative, an id that is positive in one pair and negative in the next"""
    reqs = ((7, ((30, 30),)), (7, ((12, 40), (12, 40), (30, 30))), (9, ((9, 100), (200, 9))), (50, ((60, 70), (70, 80), (80, 60))),
            (3, ((3, 3),)))
    return rd.fold_rows(33), None, reqs, K


INF_N, INF_ROWS = rb.INF_N, rb.INF_ROWS


def inf_family():
    """Euclid only.  Finite targets: the +inf rows end a k > len answer with d(t, x) = +inf.  Request 1 has +inf rows among its
    context examples: d(e, x) is +inf at finite rows and NaN at the other +inf rows -- an unsatisfied pair, not an error"""
    return rb.inf_rows(), None, ((4, ((200, 9),)), (7, ((INF_ROWS[0], 9), (9, INF_ROWS[0]), (11, INF_ROWS[1])))), 1000


def inf_nan_request():
    """a target with a +inf element: inf - inf at the other +inf rows (and at itself) is NaN"""
    return ((INF_ROWS[0], ((4, 9),)),)


FAMILIES = {"ragged": ragged, "loose": loose, "half": half, "deep": deep, "contra": contra, "tri": tri, "repeats": repeats}
# the stage the request(s) named here must end at in the automatic route, Euclid and Cosine (family -> {request: stage})
STAGES = {"loose": {0: 0, 1: 0}, "half": {0: 1}, "deep": {0: STAGE_SCAN}, "contra": {0: STAGE_SCAN}, "tri": {0: STAGE_SCAN}}
