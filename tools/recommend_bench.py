#!/usr/bin/env python3
"""Recommend from stored ids (vdb_flat_recommend_batch) against what a caller had to do without it, at the
headline shape: 1M x 768 Cosine, 256 requests of 8 positives + 4 negatives, k = 10, uniform rows as bench.py's config c2 draws
them, one process, one GPU, one handle.

    recommend    ONE call: GpuFlatIndex.recommend_batch(positive, negative, k)
    composed     what the parent commit offers: get_vector for every example (one device-to-host copy and one synchronisation
                 each), the fold in numpy f32 in the contract's order, search_batch_arrays with k + 12, the strike of the
                 examples on the host (by id, as the contract says)
    plain        search_batch_arrays with k + 12 on the folded vectors alone: recommend minus plain is what the fold, the strike
                 and the upload of the lists cost on top of the search

The arms take host ids in and hand host arrays out, run on the same handle and alternate round by round, so that clock and cache
state are shared; mean, median and minimum of each arm's wall time per call are reported, and the answers of the first two are
compared (ids and distance bits).  A record, not a bar: no pass / fail time is attached.

    python tools/recommend_bench.py [--rows N] [--dim D] [--requests B] [--pos P] [--neg Q] [--k K] [--rounds R]
                                    [--out profiles/r15_recommend_bench.json]"""
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

F32 = np.float32


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def summary(v):
    return {"mean": round(sum(v) / len(v), 4), "median": round(med(v), 4), "min": round(min(v), 4)}


def average(block):
    """[n][B, d] -> [B, d]: the left fold of include/vdb_flat.h, all requests at once"""
    s = block[0].copy()
    for x in block[1:]:
        s = s + x
    return s if len(block) == 1 else s * (F32(1) / F32(len(block)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--pos", type=int, default=8)
    ap.add_argument("--neg", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k, P, Q = a.rows, a.dim, a.requests, a.k, a.pos, a.neg
    m = P + Q
    g = torch.Generator(device=dev).manual_seed(21)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, a.metric), keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    ex = np.random.default_rng(23).choice(n, B * m, replace=False).astype(np.uint64).reshape(B, m)
    pos, neg = [r[:P] for r in ex], [r[P:] for r in ex]

    def recommend():
        t0 = time.perf_counter()
        res = ix.recommend_batch(pos, neg, k)
        return (time.perf_counter() - t0) * 1e3, res

    def composed():
        t0 = time.perf_counter()
        v = np.stack([ix.get_vector(int(i)).data for i in ex.reshape(-1)]).reshape(B, m, d)
        t1 = time.perf_counter()
        q = average([v[:, i] for i in range(P)])
        if Q:
            q = q + (q - average([v[:, P + i] for i in range(Q)]))
        q = np.ascontiguousarray(q, dtype=F32)
        t2 = time.perf_counter()
        ids, dists, counts = ix.search_batch_arrays(q, k + m)
        t3 = time.perf_counter()
        oi = np.zeros((B, k), dtype=np.uint64)
        od = np.zeros((B, k), dtype=np.float32)
        oc = np.zeros(B, dtype=np.uintp)
        for b in range(B):
            c = int(counts[b])
            keep = np.nonzero(~np.isin(ids[b, :c], ex[b]))[0][:k]
            oc[b] = keep.size
            oi[b, :keep.size] = ids[b, keep]
            od[b, :keep.size] = dists[b, keep]
        t4 = time.perf_counter()
        return (t4 - t0) * 1e3, (oi, od, oc), ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3), q

    def plain(q):
        t0 = time.perf_counter()
        ix.search_batch_arrays(q, k + m)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        recommend()
        plain(composed()[3])
    ta, tb, tc, parts = [], [], [], []
    for _ in range(a.rounds):
        t, ra = recommend()
        ta.append(t)
        t, rb, p, q = composed()
        tb.append(t)
        parts.append(p)
        tc.append(plain(q))
    stats = ix.recommend_stats()
    for b in range(B):
        c = int(ra[2][b])
        assert c == int(rb[2][b]) and np.array_equal(ra[0][b, :c], rb[0][b, :c]), b
        assert np.array_equal(ra[1][b, :c].view(np.uint32), rb[1][b, :c].view(np.uint32)), b
    part = lambda i: round(med([p[i] for p in parts]), 4)
    doc = {"tool": "tools/recommend_bench.py", "rows": n, "dim": d, "requests": B, "positives": P, "negatives": Q, "k": k,
           "metric": a.metric.lower(), "rounds": a.rounds,
           "recommend_ms": summary(ta), "composed_ms": summary(tb),
           "composed_parts_ms": {"get_vector": part(0), "host_fold": part(1), "search_k_plus_m": part(2), "host_strike": part(3)},
           "plain_search_k_plus_m_ms": summary(tc),
           "fold_and_strike_ms": round(med(ta) - med(tc), 4),
           "composed_over_recommend": round(med(tb) / med(ta), 2), "recommend_stats": stats, "answers_identical": True}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
