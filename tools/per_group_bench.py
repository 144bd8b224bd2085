#!/usr/bin/env python3
"""The k nearest groups with up to g rows of each (vdb_flat_search_batch_per_group) against the composition a caller
has without it, at the headline shape: 1M x 768 Cosine, 256 queries, k = 10, g = 3, one process, one GPU, one handle.  The rows
are "documents" of 16 chunks: chunk 0 lies at the document's centre (uniform, as bench.py's config c2 draws its rows) + 0.05 *
gaussian, the other 15 are independent uniform rows, so the 2nd and 3rd best chunk of a document lie anywhere in a query's
ranking; row r belongs to document r % (rows / 16).  A query lies near a document centre.

    per_group    ONE call: GpuFlatIndex.search_batch_per_group(queries, k, g, table, slot)
    composed     search_batch_distinct for the groups, then search_batch_grouped with one N-bit host mask per wanted document and
                 one query per (query, document) pair, in batches of at most 1024 masks (that call's limit); the masks are built
                 on the host inside the timed region, as a caller has to build them
    distinct     search_batch_distinct alone: the first stage of both arms

The arms take host queries in and hand host arrays out, run on the same handle and alternate round by round, so that clock and
cache state are shared; the median and the minimum of each arm's wall time per call are reported with per_group_stats.  The two
answers are compared pair by pair, ids and distance bits.  members_ms = per_group - distinct is what the member lists, the fill
and the larger copy-out add; the member lists and the fill run between the same two host synchronisations, so their split is the
kernels' own time from a kernel trace (--kernel-stats takes the trace's stats file and copies the per_group kernels' lines).
A record, not a bar: no pass / fail time is attached.

    python tools/per_group_bench.py [--rows N] [--dim D] [--queries B] [--k K] [--g G] [--rounds R] [--out profiles/per_group_bench.json]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402

MAX_MASKS = 1024


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--g", type=int, default=3)
    ap.add_argument("--per-doc", type=int, default=16)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-stats", default="", help="a kernel trace's stats csv: the per_group kernels' lines are copied into the record")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k, g = a.rows, a.dim, a.queries, a.k, a.g
    n_docs = n // a.per_doc
    n = n_docs * a.per_doc
    gen = torch.Generator(device=dev).manual_seed(41)
    centres = torch.rand((n_docs, d), device=dev, generator=gen, dtype=torch.float32)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, a.metric), keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        r = torch.arange(r0, min(r0 + chunk, n), device=dev)
        rows = torch.rand((r.numel(), d), device=dev, generator=gen, dtype=torch.float32)
        first = r < n_docs                                                      # chunk 0 of every document: at its centre
        rows[first] = centres[r[first]] + 0.05 * torch.randn((int(first.sum()), d), device=dev, generator=gen, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    codes = (np.arange(n) % n_docs).astype(np.int32)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, codes)
    at = torch.from_numpy(np.random.default_rng(42).choice(n_docs, B, replace=False)).to(dev)
    q = (centres[at] + 0.05 * torch.randn((B, d), device=dev, generator=gen, dtype=torch.float32)).cpu().numpy()
    del centres
    words = (n + 63) // 64
    member_ids = np.arange(a.per_doc, dtype=np.int64) * n_docs                  # the ids of document c: c + these

    def per_group():
        t0 = time.perf_counter()
        res = ix.search_batch_per_group(q, k, g, table, 0)
        return (time.perf_counter() - t0) * 1e3, res

    def distinct():
        t0 = time.perf_counter()
        ix.search_batch_distinct(q, k, table, 0)
        return (time.perf_counter() - t0) * 1e3

    def composed():
        t0 = time.perf_counter()
        ids, dists, gcodes, counts = ix.search_batch_distinct(q, k, table, 0)
        t1 = time.perf_counter()
        pairs = [(b, j) for b in range(B) for j in range(int(counts[b]))]
        oi = np.zeros((B, k, g), dtype=np.uint64)
        od = np.zeros((B, k, g), dtype=np.float32)
        osz = np.zeros((B, k), dtype=np.uint32)
        t_masks = t_search = 0.0
        calls = 0
        p0 = 0
        while p0 < len(pairs):
            tm = time.perf_counter()
            place, batch = {}, []
            while p0 < len(pairs):
                b, j = pairs[p0]
                c = int(gcodes[b, j])
                if c not in place:
                    if len(place) == MAX_MASKS:
                        break
                    place[c] = len(place)
                batch.append((b, j, place[c]))
                p0 += 1
            masks = np.zeros((len(place), words), dtype=np.uint64)
            for c, m in place.items():
                mid = c + member_ids
                np.bitwise_or.at(masks[m], mid >> 6, np.uint64(1) << (mid & 63).astype(np.uint64))
            qs = q[[b for b, _, _ in batch]]
            group_of = np.array([m for _, _, m in batch], dtype=np.uint32)
            ts = time.perf_counter()
            gi, gd, gc = ix.search_batch_grouped(qs, g, group_of, id_masks=masks, mask_bits=n)
            te = time.perf_counter()
            for i, (b, j, _) in enumerate(batch):
                c = int(gc[i])
                oi[b, j, :c], od[b, j, :c], osz[b, j] = gi[i, :c], gd[i, :c], c
            t_masks += ts - tm
            t_search += te - ts
            calls += 1
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (oi, od, gcodes, osz, counts), ((t1 - t0) * 1e3, t_masks * 1e3, t_search * 1e3, calls)

    for _ in range(a.warmup):
        per_group()
        composed()
        distinct()
    ta, tb, tc, parts = [], [], [], []
    for _ in range(a.rounds):
        t, ra = per_group()
        ta.append(t)
        stats = ix.per_group_stats()
        t, rb, p = composed()
        tb.append(t)
        parts.append(p)
        tc.append(distinct())
    # identical answers: every group, every member, ids and distance bits
    assert np.array_equal(ra[4], rb[4]) and np.array_equal(ra[2], rb[2])
    for b in range(B):
        for j in range(int(ra[4][b])):
            m = int(ra[3][b, j])
            assert m == int(rb[3][b, j]) and np.array_equal(ra[0][b, j, :m], rb[0][b, j, :m]), (b, j)
            assert np.array_equal(ra[1][b, j, :m].view(np.uint32), rb[1][b, j, :m].view(np.uint32)), (b, j)
    doc = {"tool": "tools/per_group_bench.py", "rows": n, "dim": d, "queries": B, "k": k, "g": g, "rows_per_document": a.per_doc,
           "metric": a.metric.lower(), "rounds": a.rounds,
           "per_group_ms": round(med(ta), 4), "per_group_ms_min": round(min(ta), 4),
           "composed_ms": round(med(tb), 4), "composed_ms_min": round(min(tb), 4),
           "composed_parts_ms": {"distinct": round(med([p[0] for p in parts]), 4), "host_masks": round(med([p[1] for p in parts]), 4),
                                 "grouped_searches": round(med([p[2] for p in parts]), 4), "grouped_calls": parts[-1][3]},
           "distinct_ms": round(med(tc), 4), "distinct_ms_min": round(min(tc), 4),
           "members_ms": round(med(ta) - med(tc), 4),
           "composed_over_per_group": round(med(tb) / med(ta), 2),
           "per_group_stats": stats, "answers_identical": True}
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            doc["kernel_stats"] = [row for row in csv.DictReader(f) if "per_group" in row.get("Name", "") or "distinct" in row.get("Name", "")]
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
