#!/usr/bin/env python3
"""One nearest row per group (vdb_flat_search_batch_distinct) against what a caller had to do without it, at the
headline shape: 1M x 768 Cosine, 256 queries, k = 10, one process, one GPU, one handle.  The rows are "documents" of 8 chunks
each: document centre (uniform, as bench.py's config c2 draws its rows) + 0.05 * gaussian; row r belongs to document
r % (rows / 8), so the chunks of a document lie far apart in the store.  A query lies near a document centre.

    distinct     ONE call: GpuFlatIndex.search_batch_distinct(queries, k, table, slot)
    overfetch    what the parent commit offers: search_batch_arrays at the depth of stage A (4 k, at least 32) and a dedupe on the
                 host; an answer with fewer than k documents is SHORT, and the caller cannot tell whether more exist
    plain        search_batch_arrays(queries, k): the cost of the step the feature is built on

The arms take host queries in and hand host arrays out, run on the same handle and alternate round by round, so that clock and
cache state are shared; the median and the minimum of each arm's wall time per call are reported with distinct_stats -- how many
queries each stage completed at the depth factor 4.  Where overfetch is not short its answer is compared with distinct's.  A
record, not a bar: no pass / fail time is attached.

    python tools/distinct_bench.py [--rows N] [--dim D] [--queries B] [--k K] [--rounds R] [--out profiles/r12_distinct_bench.json]"""
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
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--per-doc", type=int, default=8)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k = a.rows, a.dim, a.queries, a.k
    n_docs = n // a.per_doc
    g = torch.Generator(device=dev).manual_seed(31)
    centres = torch.rand((n_docs, d), device=dev, generator=g, dtype=torch.float32)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, a.metric), keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        r = torch.arange(r0, min(r0 + chunk, n), device=dev)
        rows = centres[r % n_docs] + 0.05 * torch.randn((r.numel(), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    codes = (np.arange(n) % n_docs).astype(np.int32)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, codes)
    at = torch.from_numpy(np.random.default_rng(32).choice(n_docs, B, replace=False)).to(dev)
    q = (centres[at] + 0.05 * torch.randn((B, d), device=dev, generator=g, dtype=torch.float32)).cpu().numpy()
    del centres
    depth = vdb.GpuFlatIndex.distinct_depth(k, n, 0)

    def distinct():
        t0 = time.perf_counter()
        res = ix.search_batch_distinct(q, k, table, 0)
        return (time.perf_counter() - t0) * 1e3, res

    def overfetch():
        t0 = time.perf_counter()
        ids, dists, counts = ix.search_batch_arrays(q, depth)
        t1 = time.perf_counter()
        oi = np.zeros((B, k), dtype=np.uint64)
        od = np.zeros((B, k), dtype=np.float32)
        oc = np.zeros(B, dtype=np.uintp)
        for b in range(B):
            c = int(counts[b])
            _, first = np.unique(codes[ids[b, :c].astype(np.int64)], return_index=True)
            keep = np.sort(first)[:k]
            oc[b] = keep.size
            oi[b, :keep.size] = ids[b, keep]
            od[b, :keep.size] = dists[b, keep]
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (oi, od, oc), ((t1 - t0) * 1e3, (t2 - t1) * 1e3)

    def plain():
        t0 = time.perf_counter()
        ix.search_batch_arrays(q, k)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        distinct()
        overfetch()
        plain()
    ta, tb, tc, parts = [], [], [], []
    for _ in range(a.rounds):
        t, ra = distinct()
        ta.append(t)
        t, rb, p = overfetch()
        tb.append(t)
        parts.append(p)
        tc.append(plain())
    stats = ix.distinct_stats()
    assert (ra[3] == k).all()
    short = int((rb[2] < k).sum())
    for b in range(B):
        c = int(rb[2][b])                                                      # a prefix of the exact answer, as far as it goes
        assert np.array_equal(ra[0][b, :c], rb[0][b, :c]) and np.array_equal(ra[1][b, :c].view(np.uint32), rb[1][b, :c].view(np.uint32)), b
    doc = {"tool": "tools/distinct_bench.py", "rows": n, "dim": d, "queries": B, "k": k, "rows_per_document": a.per_doc,
           "metric": a.metric.lower(), "rounds": a.rounds,
           "distinct_ms": round(med(ta), 4), "distinct_ms_min": round(min(ta), 4),
           "overfetch_ms": round(med(tb), 4), "overfetch_ms_min": round(min(tb), 4), "overfetch_depth": depth,
           "overfetch_parts_ms": {"search": round(med([p[0] for p in parts]), 4), "host_dedupe": round(med([p[1] for p in parts]), 4)},
           "overfetch_short_answers": short, "overfetch_short_share": round(short / B, 4),
           "plain_ms": round(med(tc), 4), "plain_ms_min": round(min(tc), 4),
           "distinct_over_plain": round(med(ta) / med(tc), 2),
           "distinct_stats": stats,
           "share_completed": {"stage_a": round(stats[1] / B, 4), "stage_b": round(stats[2] / B, 4), "exclusion": round(stats[3] / B, 4)},
           "overfetch_is_a_prefix_of_distinct": True}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
