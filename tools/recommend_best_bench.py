#!/usr/bin/env python3
"""Recommend by best score (vdb_flat_recommend_best_batch) against what a caller had to do without it, at the
headline shape: 1M x 768 Cosine, 256 requests of 8 positives + 4 negatives, k = 10, uniform rows as bench.py's config c2 draws
them, one process, one GPU, one handle.

    auto        ONE call: GpuFlatIndex.recommend_best_batch(positive, negative, k); the stage counts come from recommend_best_stats
    scan        the same call forced to the exact scan (debug_set_recommend_best_route(2)): one pass over the rows per request
    composed    what the parent commit offers: search_batch_by_id for every positive at the stage-0 depth (one call for all of
                them), the frontier / settled / fold / strike walk of tests/recommend_best_data.py on the host, get_vector for
                every candidate and every negative (one device-to-host copy and one synchronisation each), the distances to the
                negatives and the kept rule in numpy f32

The arms take host ids in and hand host arrays out and run on the same handle, round by round; mean, median and minimum of each
arm's wall time per call are reported.  The answers must be identical: ids, dp bits and counts of all three, dn bits of the two
device arms (the composed arm's numpy distances to the negatives decide the kept rule only; a request the stage-0 lists cannot
settle on the host fails the run instead of being escalated).  A record, not a bar: no pass / fail time is attached.

    python tools/recommend_best_bench.py [--rows N] [--dim D] [--requests B] [--pos P] [--neg Q] [--k K] [--rounds R]
                                         [--composed-rounds C] [--out profiles/recommend_best_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402

F32, U32 = np.float32, np.uint32


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def summary(v):
    return {"mean": round(sum(v) / len(v), 4), "median": round(med(v), 4), "min": round(min(v), 4)}


def ordered(d):
    b = np.asarray(d, dtype=F32).view(U32)
    return np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)


def cosine(a, b):
    """1 - clamp(a . b / (|a| |b|)) in numpy f32, one row of b per output"""
    sim = (b @ a) / (np.sqrt(F32((a * a).sum())) * np.sqrt((b * b).sum(axis=1, dtype=F32)))
    return (F32(1) - np.clip(sim, F32(-1), F32(1))).astype(F32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--pos", type=int, default=8)
    ap.add_argument("--neg", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--composed-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k, P, Q = a.rows, a.dim, a.requests, a.k, a.pos, a.neg
    m = P + Q
    g = torch.Generator(device=dev).manual_seed(21)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    ex = np.random.default_rng(23).choice(n, B * m, replace=False).astype(np.uint64).reshape(B, m)
    pos, neg = [r[:P] for r in ex], [r[P:] for r in ex]
    depth = int(vdb._ffi.lib().vdb_flat_recommend_best_depth(k, m, n, 0))

    def device(route):
        ix.debug_set_recommend_best_route(route)
        t0 = time.perf_counter()
        res = ix.recommend_best_batch(pos, neg, k)
        t = (time.perf_counter() - t0) * 1e3
        ix.debug_set_recommend_best_route(0)
        return t, res, ix.recommend_best_stats()

    def composed():
        t0 = time.perf_counter()
        # the list of a positive at depth `depth` holds the positive itself, an example: by id that is depth - 1 neighbours
        li, ld, lc = ix.search_batch_by_id(ex[:, :P].reshape(-1), depth - 1)
        t1 = time.perf_counter()
        cands = []
        for b in range(B):
            best = {}
            fronts = [ld[b * P + i, depth - 2] for i in range(P) if int(lc[b * P + i]) == depth - 1]
            F = min(fronts) if fronts else None
            for i in range(P):
                c = int(lc[b * P + i])
                for x, dist in zip(li[b * P + i, :c], ld[b * P + i, :c]):
                    if F is not None and not dist < F:
                        break
                    if int(x) not in best or dist < best[int(x)]:
                        best[int(x)] = dist
            mine = set(int(e) for e in ex[b])
            ids = np.array([x for x in best if x not in mine], dtype=np.uint64)
            dp = np.array([best[int(x)] for x in ids], dtype=F32)
            o = np.lexsort((ids, ordered(dp)))
            cands.append((ids[o], dp[o]))
        t2 = time.perf_counter()
        vec = {}
        for b in range(B):
            for i in list(cands[b][0]) + list(ex[b, P:]):
                if int(i) not in vec:
                    vec[int(i)] = np.asarray(ix.get_vector(int(i)).data, dtype=F32)
        t3 = time.perf_counter()
        oi = np.zeros((B, k), dtype=np.uint64)
        od = np.zeros((B, k), dtype=F32)
        oc = np.zeros(B, dtype=np.uintp)
        for b in range(B):
            ids, dp = cands[b]
            keep = np.ones(len(ids), dtype=bool)
            if len(ids):
                block = np.stack([vec[int(i)] for i in ids])
                for e in ex[b, P:]:
                    keep &= dp < cosine(vec[int(e)], block)
            sel = np.nonzero(keep)[0][:k]
            assert sel.size == k, (b, "the stage-0 lists do not settle this request on the host")
            oc[b] = sel.size
            oi[b, :sel.size] = ids[sel]
            od[b, :sel.size] = dp[sel]
        t4 = time.perf_counter()
        parts = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3)
        return (t4 - t0) * 1e3, (oi, od, oc), parts, len(vec)

    for _ in range(a.warmup):
        device(0)
    device(2)
    ta, ts, tc, parts = [], [], [], []
    for r in range(a.rounds):
        t, ra, sa = device(0)
        ta.append(t)
        t, rs, ss = device(2)
        ts.append(t)
        if r < a.composed_rounds:
            t, rc, p, fetched = composed()
            tc.append(t)
            parts.append(p)
    for b in range(B):
        c = int(ra[3][b])
        assert c == int(rs[3][b]) == int(rc[2][b]), b
        for x, y in ((ra[0], rs[0]), (ra[0], rc[0])):
            assert np.array_equal(x[b, :c], y[b, :c]), b
        for x, y in ((ra[1], rs[1]), (ra[1], rc[1]), (ra[2], rs[2])):
            assert np.array_equal(x[b, :c].view(U32), y[b, :c].view(U32)), b
    part = lambda i: round(med([p[i] for p in parts]), 4)
    doc = {"tool": "tools/recommend_best_bench.py", "rows": n, "dim": d, "requests": B, "positives": P, "negatives": Q, "k": k,
           "metric": "cosine", "rounds": a.rounds, "composed_rounds": len(tc), "stage0_depth": depth,
           "auto_ms": summary(ta), "auto_stats": sa, "scan_ms": summary(ts), "scan_stats": ss, "composed_ms": summary(tc),
           "composed_parts_ms": {"search_by_id": part(0), "host_walk": part(1), "get_vector": part(2), "host_veto": part(3)},
           "composed_vectors_fetched": fetched,
           "scan_over_auto": round(med(ts) / med(ta), 2), "composed_over_auto": round(med(tc) / med(ta), 2), "answers_identical": True}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
