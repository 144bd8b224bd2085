#!/usr/bin/env python3
"""The exact range search (vdb_flat_range_search_batch_device) at the headline shape: 1M x 768 Cosine, B = 256,
uniform rows and queries as bench.py's config c2 draws them, device-resident calls, one process, one GPU, one JSON document.

The radii are each query's own 10th and 100th neighbour distance (taken from a k = 100 search on the same handle), so the range
search returns what a top-10 / top-100 search returns, plus ties.  Per depth:

    range_ms     median ms per batch of vdb_flat_range_search_batch_device (max_results = 128)
    topk_ms      median ms per batch of vdb_flat_search_batch_device with k = 10 / 100 on the same handle, interleaved
    range_stats  the route counters of the last range search (vdb_flat_range_stats)
    totals       min / median / max rows within the radius

and the range results are compared with the top-k results (ids and distance bits of the common prefix).  No pass / fail time
is attached.

    python tools/range_bench.py [--rows N] [--dim D] [--batch B] [--steps S] [--out profiles/range_bench.json]"""
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, mr = a.rows, a.dim, a.batch, 128
    g = torch.Generator(device=dev).manual_seed(21)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, a.metric), keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    q = torch.rand((B, d), device=dev, generator=g, dtype=torch.float32)

    def outputs(k):
        return (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
                torch.empty((B,), dtype=torch.int32, device=dev))

    top = {k: outputs(k) for k in (10, 100)}

    def topk(k):
        o = top[k]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.search_batch_device(q.data_ptr(), B, d, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    topk(100)
    topk(10)
    rng_out = outputs(mr)
    totals = torch.empty((B,), dtype=torch.int64, device=dev)
    doc = {"tool": "tools/range_bench.py", "rows": n, "dim": d, "batch": B, "metric": a.metric.lower(), "max_results": mr,
           "steps": a.steps, "depths": []}
    for depth in (10, 100):
        radii = top[100][1][:, depth - 1].contiguous()

        def rng_step():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.range_search_batch_device(q.data_ptr(), B, d, radii.data_ptr(), mr, rng_out[0].data_ptr(), rng_out[1].data_ptr(),
                                         rng_out[2].data_ptr(), out_totals_ptr=totals.data_ptr())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(a.warmup):
            rng_step()
            topk(depth)
        tr, tk = [], []
        for _ in range(a.steps):
            tr.append(rng_step())
            tk.append(topk(depth))
        stats = ix.range_stats()
        tot = totals.cpu().numpy()
        cnt = rng_out[2].cpu().numpy()
        ri, rd_ = rng_out[0].cpu().numpy(), rng_out[1].cpu().numpy()
        ti, td = top[depth][0].cpu().numpy(), top[depth][1].cpu().numpy()
        for b in range(B):
            c = min(int(cnt[b]), depth)
            assert int(tot[b]) >= depth and int(cnt[b]) == min(int(tot[b]), mr), (depth, b, int(tot[b]), int(cnt[b]))
            assert np.array_equal(ri[b, :c], ti[b, :c]) and np.array_equal(rd_[b, :c].view(np.uint32), td[b, :c].view(np.uint32)), (depth, b)
        doc["depths"].append({"radius_at_neighbour": depth, "range_ms": round(med(tr), 4), "range_ms_min": round(min(tr), 4),
                              "topk_ms": round(med(tk), 4), "topk_ms_min": round(min(tk), 4), "range_over_topk": round(med(tr) / med(tk), 3),
                              "range_stats": stats, "totals": [int(tot.min()), int(np.median(tot)), int(tot.max())]})
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
