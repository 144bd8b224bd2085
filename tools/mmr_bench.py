#!/usr/bin/env python3
"""Diverse top-k (vdb_flat_search_batch_mmr) against what a caller had to do without it, at the headline shape:
1M x 768 Cosine, 256 queries, k = 10, m = 100 candidates, lambda = 0.5, uniform rows as bench.py's config c2 draws them, one
process, one GPU, one handle.

    mmr          ONE call: GpuFlatIndex.search_batch_mmr(queries, k, m, lambda)
    composed     what the parent commit offers: search_batch_arrays at depth m, get_vector for every candidate (one
                 device-to-host copy and one synchronisation each), and the greedy loop on the host in numpy f32 with the
                 contract's definition -- sequential f32 folds (np.cumsum accumulates strictly left to right), norms as
                 sqrt(fold(x * x)), score = lambda * d - mu * near in two roundings, ties by position -- all queries at once
    plain        search_batch_arrays at depth m alone: mmr minus plain is what the id -> row round trip, the selection kernel
                 and the copy-out of the picks cost on top of the search

The arms take host arrays in and hand host arrays out, run on the same handle and alternate round by round, so that clock and
cache state are shared; mean, median and minimum of each arm's wall time per call are reported, and the answers of the first two
are compared (ids, pick order, distance bits, score bits) into `answers_identical`.  A record, not a bar: no pass / fail time is
attached.

    python tools/mmr_bench.py [--rows N] [--dim D] [--queries B] [--k K] [--candidates M] [--lam L] [--rounds R]
                              [--out profiles/mmr_bench.json]"""
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


def fold(x):
    """[..., d] -> [...]: the sequential f32 left fold"""
    return np.cumsum(x, axis=-1, dtype=F32)[..., -1]


def pair_distances(metric, V, norms, s):
    """D(i, s_b) for every candidate i of every query b: V [B, m, d], s [B] the last pick's position"""
    B = V.shape[0]
    P = V[np.arange(B), s][:, None, :]                                          # [B, 1, d]
    if metric == "Euclidean":
        t = V - P
        return np.sqrt(fold(t * t))
    dot = fold(P * V)
    if metric == "DotProduct":
        return -dot
    den = norms[np.arange(B), s][:, None] * norms
    return F32(1) - np.clip(dot / den, F32(-1), F32(1))


def host_mmr(metric, V, d, counts, k, lam):
    """the greedy selection of include/vdb_flat.h for all queries at once; returns (positions [B, k], scores [B, k])"""
    B, m, _ = V.shape
    lam = F32(lam)
    mu = F32(1) - lam
    norms = np.sqrt(fold(V * V)) if metric == "Cosine" else None
    live = np.arange(m)[None, :] < counts[:, None]
    picked = ~live
    near = np.full((B, m), np.inf, dtype=F32)
    picks = np.zeros((B, k), dtype=np.int64)
    scores = np.zeros((B, k), dtype=F32)
    scores[:, 0] = lam * d[:, 0]
    picked[:, 0] = True
    for t in range(1, k):
        D = pair_distances(metric, V, norms, picks[:, t - 1])
        near = np.where(picked, near, np.minimum(near, D))
        score = (lam * d).astype(F32) - (mu * near).astype(F32)
        # (isnan, score, position): NaN scores and picked entries are pushed behind every number; argmin takes the first of equals
        key = np.where(picked | np.isnan(score), np.inf, score)
        best = np.argmin(key, axis=1)
        picks[:, t] = best
        scores[:, t] = score[np.arange(B), best]
        picked[np.arange(B), best] = True
    return picks, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k, m = a.rows, a.dim, a.queries, a.k, a.candidates
    g = torch.Generator(device=dev).manual_seed(21)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, a.metric), keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    qs = np.random.default_rng(23).random((B, d), dtype=F32)

    def mmr():
        t0 = time.perf_counter()
        res = ix.search_batch_mmr(qs, k, m, a.lam)
        return (time.perf_counter() - t0) * 1e3, res

    def composed():
        t0 = time.perf_counter()
        ids, dists, counts = ix.search_batch_arrays(qs, m)
        t1 = time.perf_counter()
        V = np.zeros((B, m, d), dtype=F32)
        for b in range(B):
            for i in range(int(counts[b])):
                V[b, i] = ix.get_vector(int(ids[b, i])).data
        t2 = time.perf_counter()
        picks, scores = host_mmr(a.metric, V, dists, counts.astype(np.int64), k, a.lam)
        rows_ = np.arange(B)[:, None]
        res = (ids[rows_, picks], dists[rows_, picks], scores, np.minimum(counts, k))
        t3 = time.perf_counter()
        return (t3 - t0) * 1e3, res, ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)

    def plain():
        t0 = time.perf_counter()
        ix.search_batch_arrays(qs, m)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        mmr()
        composed()
        plain()
    ta, tb, tc, parts, rstats = [], [], [], [], []
    for _ in range(a.rounds):
        t, ra = mmr()
        ta.append(t)
        rstats.append(ix.mmr_stats())
        t, rb, p = composed()
        tb.append(t)
        parts.append(p)
        tc.append(plain())
    same = True
    for b in range(B):
        c = int(ra[3][b])
        same = same and c == int(rb[3][b]) and np.array_equal(ra[0][b, :c], rb[0][b, :c])
        same = same and np.array_equal(ra[1][b, :c].view(np.uint32), rb[1][b, :c].view(np.uint32))
        same = same and np.array_equal(ra[2][b, :c].view(np.uint32), rb[2][b, :c].view(np.uint32))
    plain_ids = ix.search_batch_arrays(qs, k)[0]
    left = sum(int(set(ra[0][b].tolist()) != set(plain_ids[b].tolist())) for b in range(B))
    part = lambda i: round(med([p[i] for p in parts]), 4)
    doc = {"tool": "tools/mmr_bench.py", "rows": n, "dim": d, "queries": B, "k": k, "candidates": m, "lambda": a.lam,
           "metric": a.metric.lower(), "rounds": a.rounds,
           "mmr_ms": summary(ta), "composed_ms": summary(tb),
           "composed_parts_ms": {"search_depth_m": part(0), "get_vector": part(1), "host_loop": part(2)},
           "plain_search_depth_m_ms": summary(tc),
           "selection_and_round_trip_ms": round(med(ta) - med(tc), 4),
           "id_to_row_host_ms": round(med([s[5] for s in rstats]) / 1e6, 4),
           "composed_over_mmr": round(med(tb) / med(ta), 2), "mmr_stats": rstats[-1][:5],
           "queries_that_leave_the_plain_top_k": left, "answers_identical": bool(same)}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
