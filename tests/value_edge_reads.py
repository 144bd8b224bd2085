"""What the CPU oracle and the existing models (by_id_data, recommend_data, distinct_data, mmr_data) say about the value families
(tests/value_families.py) under the five read kinds that came after the plain search: by stored id, recommend, one row per group,
a filter per query, MMR.  tests/test_value_edges_cpu.py proves on the CPU that the data bites; tests/test_gpu_value_edges_reads.py
compares the engine with exactly these expectations.  Nothing here computes a distance of its own."""
import json
import os

import numpy as np

import oracle
import by_id_data as bd
import mmr_data as md
import recommend_data as rd
import value_families as vf

F32, U64 = np.float32, np.uint64
ERROR_NAMES = {oracle.ERR_INVALID_VECTOR: "InvalidVector", oracle.ERR_NAN: "NanDistance"}
K, MMR_K, MMR_M = 10, 10, 40
LAMBDAS = (0.0, 0.5, 1.0)
MIN_NORMAL = F32(1.17549435e-38)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "value_edges_mmr_classes.json")

_CACHE = {}


def once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def outcome(call):
    """("ok", value) or (the name of the engine's exception class for the oracle's error, None)"""
    try:
        return "ok", call()
    except oracle.OracleError as e:
        return ERROR_NAMES[e.code], None


def case_data(case, shape):
    family, metric, kw = case
    n, d, nq, _ = vf.SHAPES[shape]
    rows, q = vf.make(family, n, d, nq, metric, **kw)
    return rows, q, n, d, nq


def case_key(case, shape):
    return (case[0], case[1], tuple(sorted(case[2].items())), shape)


def plain_case(family, metric):
    return (family, metric, {})


# ------------------------------------------------------------------ by stored id
BY_ID_DEPTH = 65                                                   # the deepest list any test asks for: k = 64, plus the row itself


def by_id_deep(case, shape, ids, live, tag):
    """per id: ("ok", (oi, od)) -- the oracle's list of the stored row at depth 65, before any strike -- or (error, None).  The
    list for a smaller k + 1 is its prefix (one comparator, (distance, unsigned id)), and whether the oracle errors does not
    depend on k: it computes every eligible row's distance."""
    rows = case_data(case, shape)[0]
    return [once(("by_id", case_key(case, shape), int(r), tag),
                 lambda: outcome(lambda: oracle.flat_search(case[1], rows, rows[int(r)], BY_ID_DEPTH, live=live))) for r in ids]


def by_id_lists(case, shape, ids, k, live, tag="plain"):
    """the k + 1 lists of the ids the oracle answers"""
    return [(lst[0][:int(k) + 1], lst[1][:int(k) + 1]) for o, lst in by_id_deep(case, shape, ids, live, tag) if o == "ok"]


def by_id_split(case, shape, ids, ks, live, tag="plain"):
    """(answered ids, their expectation by by_id_data.strike (ids, dists, struck, cut), [(refused id, error)]); ks: an int, or one
    k per ANSWERED id"""
    deep = by_id_deep(case, shape, ids, live, tag)
    good = np.array([int(r) for r, (o, _) in zip(ids, deep) if o == "ok"], dtype=np.int64)
    bad = [(int(r), o) for r, (o, _) in zip(ids, deep) if o != "ok"]
    kk = [int(ks)] * len(good) if np.isscalar(ks) else [int(x) for x in ks]
    assert len(kk) == len(good) and max(kk + [0]) < BY_ID_DEPTH
    lists = [lst for o, lst in deep if o == "ok"]
    want = [bd.strike(oi[:kb + 1], od[:kb + 1], int(r), kb) for (oi, od), r, kb in zip(lists, good, kk)]
    return good, want, bad


def by_id_stats(want_at_kmax):
    """[queries, struck, cut, 0] of by_id_stats() from the expectation at max(ks): the device searches max(k) + 1 for every query"""
    return [len(want_at_kmax), sum(1 for w in want_at_kmax if w[2]), sum(1 for w in want_at_kmax if w[3]), 0]


# ------------------------------------------------------------------ recommend
def recommend_split(metric, rows, requests, k, live, key):
    """(answered requests, their recommend_data expectation, [(request, error)])"""
    def make():
        good, want, bad = [], [], []
        for req in requests:
            o, w = outcome(lambda: rd.expected(metric, rows, [req], k, live=live))
            if o == "ok":
                good.append(req)
                want.append(w[0])
            else:
                bad.append((req, o))
        return good, want, bad
    return once(("rec", key, metric, k), make)


# ------------------------------------------------------------------ one row per group
def ranking(case, shape, b, live, tag):
    rows, q, n, _, _ = case_data(case, shape)
    return once(("rank", case_key(case, shape), b, tag), lambda: oracle.flat_search(case[1], rows, q[b], n, live=live))


# ------------------------------------------------------------------ MMR
def mmr_want(case, shape, qsel, k, m, lam, live, stored=None, tag="plain"):
    rows, q, _, _, _ = case_data(case, shape)
    lam_key = lam if np.isscalar(lam) else tuple(float(x) for x in lam)
    k_key = k if np.isscalar(k) else tuple(int(x) for x in k)
    return once(("mmr", case_key(case, shape), tuple(qsel), k_key, m, lam_key, tag),
                lambda: md.expected(case[1], rows, q[list(qsel)], k, m, lam, live=live, stored=stored))


def mmr_class(w):
    """the outcome class of one query: NaN pair, and how many of its picks were chosen with a NaN / infinite / subnormal score"""
    s = w["scores"]
    return {"nan_pair": bool(w["nan"]), "nan": int(np.isnan(s).sum()), "inf": int(np.isinf(s).sum()),
            "subnormal": int(((np.abs(s) < MIN_NORMAL) & (s != 0)).sum()),
            "plain_order": [int(p) for p in w["picks"]] == list(range(len(w["picks"])))}


def mmr_classes():
    """{case id / shape / lambda: [class per checked query]} over vf.CASES at k = 10, m = 40"""
    out = {}
    for (family, metric), name in zip(vf.CASES, vf.CASE_IDS):
        case = plain_case(family, metric)
        for shape in vf.READ_SHAPES:
            n, _, nq, _ = vf.SHAPES[shape]
            qsel = vf.checked_queries(nq)
            for lam in LAMBDAS:
                want = mmr_want(case, shape, qsel, MMR_K, MMR_M, lam, vf.live_bytes(n))
                out["%s/%s/%g" % (name, shape, lam)] = [mmr_class(w) for w in want]
    return out


def golden_mmr_classes():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":                                         # PYTHONPATH=. python tests/value_edge_reads.py: rewrite the pinned classes
    with open(GOLDEN, "w") as f:
        json.dump(mmr_classes(), f, indent=0, sort_keys=True)
        f.write("\n")
