#!/usr/bin/env python3
"""Search by stored id (vdb_flat_search_batch_by_id) against what a caller had to do without it, at the headline
shape: 1M x 768 Cosine, 256 query ids, k = 10, uniform rows as bench.py's config c2 draws them, one process, one GPU, one handle.

    by_id        ONE call: GpuFlatIndex.search_batch_by_id(ids, k)
    three_step   what the parent commit offers: 256 x get_vector (one device-to-host copy and one synchronisation each), then
                 search_batch_arrays with k + 1, then the strike of the own id on the host (by id equality, as the contract says)

Both arms take host ids in and hand host arrays out, run on the same handle and alternate round by round, so that clock and
cache state are shared; the median and the minimum of each arm's wall time per call are reported, and the two answers are
compared (ids and distance bits).  A record, not a bar: no pass / fail time is attached.

    python tools/by_id_bench.py [--rows N] [--dim D] [--ids B] [--k K] [--rounds R] [--out profiles/r11_by_id_bench.json]"""
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


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--ids", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k = a.rows, a.dim, a.ids, a.k
    g = torch.Generator(device=dev).manual_seed(21)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, a.metric), keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    qid = np.random.default_rng(22).choice(n, B, replace=False).astype(np.uint64)

    def by_id():
        t0 = time.perf_counter()
        res = ix.search_batch_by_id(qid, k)
        return (time.perf_counter() - t0) * 1e3, res

    def three_step():
        t0 = time.perf_counter()
        q = np.stack([ix.get_vector(int(i)).data for i in qid])
        t1 = time.perf_counter()
        ids, dists, counts = ix.search_batch_arrays(q, k + 1)
        t2 = time.perf_counter()
        oi = np.zeros((B, k), dtype=np.uint64)
        od = np.zeros((B, k), dtype=np.float32)
        oc = np.zeros(B, dtype=np.uintp)
        for b in range(B):
            c = int(counts[b])
            keep = np.nonzero(ids[b, :c] != qid[b])[0][:k]
            oc[b] = keep.size
            oi[b, :keep.size] = ids[b, keep]
            od[b, :keep.size] = dists[b, keep]
        t3 = time.perf_counter()
        return (t3 - t0) * 1e3, (oi, od, oc), ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)

    for _ in range(a.warmup):
        by_id()
        three_step()
    ta, tb, parts = [], [], []
    for _ in range(a.rounds):
        t, ra = by_id()
        ta.append(t)
        t, rb, p = three_step()
        tb.append(t)
        parts.append(p)
    stats = ix.by_id_stats()
    for b in range(B):
        c = int(ra[2][b])
        assert c == int(rb[2][b]) and np.array_equal(ra[0][b, :c], rb[0][b, :c]), b
        assert np.array_equal(ra[1][b, :c].view(np.uint32), rb[1][b, :c].view(np.uint32)), b
    doc = {"tool": "tools/by_id_bench.py", "rows": n, "dim": d, "ids": B, "k": k, "metric": a.metric.lower(), "rounds": a.rounds,
           "by_id_ms": round(med(ta), 4), "by_id_ms_min": round(min(ta), 4),
           "three_step_ms": round(med(tb), 4), "three_step_ms_min": round(min(tb), 4),
           "three_step_parts_ms": {"get_vector": round(med([p[0] for p in parts]), 4), "search_k_plus_1": round(med([p[1] for p in parts]), 4),
                                   "host_strike": round(med([p[2] for p in parts]), 4)},
           "three_step_over_by_id": round(med(tb) / med(ta), 2), "by_id_stats": stats, "answers_identical": True}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
