"""CPU side of tests/test_gpu_hnsw_limits.py: the exact walk counters of the restatement (hnsw_filter_restatement.Walker:
"pushed", "layer_visited") against a brute recount, the capacities tests/hnsw_limits.py states against the kernel source and
the documents, and the PRECONDITIONS of the GPU fixtures -- how many walks of each overflow batch land on each side of the cap
they are built to cross.  A data set that stops crossing its cap fails here, not silently on the GPU."""
import os
import re

import numpy as np
import pytest

import hnsw_limits as hl
import oracle
from conftest import ROOT
from hnsw_filter_restatement import Walker, eligible_fn


# ---------------------------------------------------------------------------------------------------------------------------
# the counters
# ---------------------------------------------------------------------------------------------------------------------------
def brute_walk(o, metric, rows, query, k, ef, elig):
    """search_knn written the slow way -- plain lists, min() / max() instead of heaps -- recording the length of the candidate
    list after every push and the size of every layer's visited set.  Without distance ties it makes the restatement's decisions."""
    after_push, layer_visited = [], []

    def layer_search(ep, ef, layer, elig):
        d0 = oracle.distance(metric, query, rows[ep])
        visited, cand = [ep], [(d0, ep)]
        after_push.append(len(cand))
        res = [(d0, ep)] if elig is None or elig[ep] else []
        while cand:
            c = min(cand)
            cand.remove(c)
            if res and c[0] > max(res)[0]:
                break
            for nid in o.neighbors(c[1], layer) or []:
                if nid in visited:
                    continue
                visited.append(nid)
                d = oracle.distance(metric, query, rows[nid])
                if len(res) < ef or d < max(res)[0]:
                    cand.append((d, nid))
                    after_push.append(len(cand))
                    if elig is None or elig[nid]:
                        res.append((d, nid))
                        if len(res) > ef:
                            res.remove(max(res))
        layer_visited.append(len(visited))
        return sorted(res)

    ep, top = o.entry_point()
    for layer in range(top, 0, -1):
        r = layer_search(ep, 1, layer, None)
        if r:
            ep = r[0][1]
    r = layer_search(ep, max(ef, k), 0, elig)[:k]
    return [i for _, i in r], max(after_push), layer_visited


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_exact_counters_equal_a_brute_recount(metric):
    n, d = 400, 12
    rows = hl.gauss(60 + metric, n, d)
    o = hl.build_oracle(metric, rows, 6, 48, seed=13)
    assert o.entry_point()[1] >= 1                                    # layers above 0 are searched and counted
    w = Walker(o, metric, {i: rows[i] for i in range(n)})
    rng = np.random.default_rng(70 + metric)
    for sel, ef, k in [(None, 50, 10), (None, 5, 20), (0.5, 50, 10), (0.05, 30, 10), (0.0, 20, 5)]:
        elig = None if sel is None else rng.random(n) < sel
        for q in rng.standard_normal((3, d)).astype(np.float32):
            peaks = {}
            wi, _ = w.search(q, k, ef, None if elig is None else eligible_fn(elig), peaks)
            bi, pushed, layer_visited = brute_walk(o, metric, rows, q, k, ef, elig)
            assert [int(i) for i in wi] == bi
            assert peaks["pushed"] == pushed, (sel, ef, peaks, pushed)
            assert peaks["layer_visited"] == layer_visited, (sel, ef, peaks, layer_visited)
            # the key that was there before keeps its meaning: layer 0's visited count
            assert peaks["visited"] == layer_visited[-1] and len(layer_visited) == o.entry_point()[1] + 1
            assert 1 <= peaks["pushed"] <= max(layer_visited)
    # nothing eligible: every reachable node is visited, and every one of them was pushed before the first pop could end the walk
    assert peaks["visited"] > n // 2


def test_a_reused_peaks_dict_keeps_maxima_and_the_last_walks_layers():
    rows = hl.gauss(3, 200, 8)
    o = hl.build_oracle(0, rows, 4, 32, seed=3)
    w = Walker(o, 0, {i: rows[i] for i in range(200)})
    qs = hl.gauss(4, 2, 8)
    a, b, both = {}, {}, {}
    w.search(qs[0], 5, 40, None, a); w.search(qs[1], 5, 40, None, b)
    w.search(qs[0], 5, 40, None, both); w.search(qs[1], 5, 40, None, both)
    assert both["pushed"] == max(a["pushed"], b["pushed"]) and both["visited"] == max(a["visited"], b["visited"])
    assert both["layer_visited"] == b["layer_visited"]


# ---------------------------------------------------------------------------------------------------------------------------
# the capacities, stated once in hnsw_limits.py, against the kernel and the documents
# ---------------------------------------------------------------------------------------------------------------------------
def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_stated_capacities_are_the_kernels():
    src = read("vectordb-from-scratch_amd", "csrc", "kernels_hnsw.hip")
    for name in ("CAND_CAP", "CAND_CAP_F", "RES_CAP", "VIS_CAP", "MAXP", "WAVE_POP_MAX"):
        found = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert found and int(found.group(1)) == getattr(hl, name), name
    assert "sNVis > (VCAP / 4) * 3" in src and "nc >= CCAP || nr >= RES_CAP" in src
    assert "(ef > k ? ef : k) + 1 <= RES_CAP && max_list <= MAXP" in src
    assert hl.VISITED_MAX == 12288 and hl.DEVICE_EF_MAX == 1023 and hl.DEVICE_M_MAX == 19
    # the insert walks' records hold what the visited set holds: record overflow is unreachable before the walk fails
    assert re.search(r"REC_CAP = (\d+)", read("vectordb-from-scratch_amd", "csrc", "vdb_hnsw.cpp")).group(1) == str(hl.VISITED_MAX)


def test_documents_state_the_routing_bounds_of_the_code():
    bound = f"ef > {hl.DEVICE_EF_MAX}"
    wrong = re.compile(r"ef > (?!%d\b)\d{4}\b" % hl.DEVICE_EF_MAX)
    for parts in (("include", "vdb_hnsw.h"), ("DESIGN.md",), ("vectordb-from-scratch_amd", "csrc", "vdb_hnsw.cpp")):
        text = read(*parts)
        assert bound in text, parts
        assert not wrong.search(text), (parts, wrong.search(text).group(0))
        assert f"m > {hl.DEVICE_M_MAX}" in text, parts


# ---------------------------------------------------------------------------------------------------------------------------
# preconditions of the GPU fixtures
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "dups"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_the_ef_graph_fills_the_largest_result_heap(metric, kind):
    s = hl.EF_SHAPE
    rows, queries, seed = hl.ef_data(metric, kind)
    o = hl.build_oracle(metric, rows, s["m"], s["efc"], seed)
    want = max(hl.EF_VALUES) if kind == "gauss" else max(hl.TIE_EF_VALUES)
    for q in queries:
        ids, ds = o.search(q, want, want)
        assert len(ids) == want                                        # more than ef nodes are reachable: the heap fills to ef + 1
        if kind == "dups":
            assert np.unique(ds).size < want // 2                      # exact ties inside the heap


@pytest.fixture(scope="module")
def overflow():
    c = hl.OVERFLOW
    rows, plain_q, elig, filt_q = hl.overflow_data()
    o = hl.build_oracle(c["metric"], rows, c["m"], c["efc"], c["graph_seed"])
    return o, rows, plain_q, elig, filt_q


def test_overflow_fixture_plain_walks_fall_on_both_sides_of_the_visited_cap(overflow):
    o, rows, plain_q, _, _ = overflow
    c, p = hl.OVERFLOW, hl.OVERFLOW_PLAIN
    assert plain_q.shape[0] == 16 and p["ef"] <= hl.DEVICE_EF_MAX
    res, ctr = hl.walk_counters(o, c["metric"], rows, plain_q, p["k"], p["ef"])
    visited = np.array([max(x["layer_visited"]) for x in ctr])
    pushed = np.array([x["pushed"] for x in ctr])
    print("visited", visited.tolist(), "pushed", pushed.tolist())
    assert pushed.max() <= hl.CAND_CAP                                 # the only cap these walks cross is the visited set's
    assert (visited > hl.VISITED_MAX).sum() >= 3 and (visited <= hl.VISITED_MAX).sum() >= 3
    assert all(max(x["layer_visited"]) == x["layer_visited"][-1] for x in ctr)
    fails = [hl.overflows(x, filtered=False) for x in ctr]
    assert fails == (visited > hl.VISITED_MAX).tolist()
    # without ties the restatement is the oracle: what the GPU test compares failed and passing rows with
    for (wi, wd), q in zip(res, plain_q):
        oi, od = o.search(q, p["k"], p["ef"])
        assert np.array_equal(wi, oi) and np.array_equal(wd.view(np.uint32), od.view(np.uint32))


def test_overflow_fixture_filtered_walks_fall_clear_of_the_candidate_cap(overflow):
    o, rows, _, elig, filt_q = overflow
    c, p = hl.OVERFLOW, hl.OVERFLOW_FILTERED
    assert 0.02 < elig.mean() < 0.05 and filt_q.shape[0] == p["near"] + p["far"]
    res, ctr = hl.walk_counters(o, c["metric"], rows, filt_q, p["k"], p["ef"], elig)
    pushed = np.array([x["pushed"] for x in ctr])
    print("pushed", pushed.tolist(), "upper-layer visited", [max(x["layer_visited"][:-1], default=0) for x in ctr])
    over, under = pushed >= 1.15 * hl.CAND_CAP_F, pushed <= 0.85 * hl.CAND_CAP_F
    assert np.all(over | under), pushed                                # every walk at least 15 % away from the cap
    assert over.sum() >= 3 and under.sum() >= 3
    assert not over[:p["near"]].any() and over[p["near"]:].all()       # near the eligible rows: fits; mirrored away from them: overflows
    assert [hl.overflows(x, filtered=True) for x in ctr] == over.tolist()
    assert all(len(i) == p["k"] and all(elig[int(j)] for j in i) for i, _ in res)
