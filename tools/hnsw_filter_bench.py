#!/usr/bin/env python3
"""Pre-filtered HNSW search (vdb_hnsw_search_batch_masked) at several selectivities: random id masks, one batch per
selectivity.  Per selectivity: queries/s of the filtered walk, queries answered on the device vs re-run by the host traversal,
recall@k against the exact filtered answer (GpuFlatIndex with the same mask), and the count and recall of the reference's
post-filter on the same queries (storage.rs:249-290: 3k results at ef = 50, the eligible ones kept).

    python tools/hnsw_filter_bench.py [--rows N] [--dim D] [--batch B] [--k K] [--ef EF] [--sel 1,0.5,0.1,0.02,0.01]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=200)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--metric", type=int, default=0)
    ap.add_argument("--sel", default="1,0.5,0.1,0.02,0.01")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    rng = np.random.default_rng(1)
    rows = rng.random((a.rows, a.dim), dtype=np.float32)
    queries = rng.random((a.batch, a.dim), dtype=np.float32)
    ids = np.arange(a.rows, dtype=np.uint64)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric(a.metric), vdb.HnswParams.new(a.m, a.efc, 50), seed=1)
    t0 = time.perf_counter()
    for c0 in range(0, a.rows, 20000):
        g.build_batch((ids[c0:c0 + 20000], rows[c0:c0 + 20000]))
    print(f"build: {a.rows} x {a.dim}, m={a.m} ef_construction={a.efc}: {time.perf_counter() - t0:.1f} s", flush=True)
    flat = vdb.GpuFlatIndex(vdb.DistanceMetric(a.metric), keep_host_copy=False)
    flat.add_bulk(rows)
    g.search_batch_arrays(queries, a.k, a.ef)                             # warm-up
    t0 = time.perf_counter()
    for _ in range(a.reps):
        g.search_batch_arrays(queries, a.k, a.ef)
    qps_plain = a.batch * a.reps / (time.perf_counter() - t0)
    print(f"unfiltered: batch {a.batch}, k={a.k}, ef={a.ef}: {qps_plain:.0f} queries/s", flush=True)
    print("| selectivity | queries/s | device walks | host re-runs | recall@%d | post-filter count | post-filter recall@%d |" % (a.k, a.k))
    print("|---|---|---|---|---|---|---|")
    for sel in [float(s) for s in a.sel.split(",")]:
        elig = rng.random(a.rows) < sel
        words = (a.rows + 63) // 64
        packed = np.zeros(words * 8, dtype=np.uint8)
        pb = np.packbits(elig, bitorder="little")
        packed[:pb.size] = pb
        mask = packed.view(np.uint64)
        g.search_batch_arrays(queries, a.k, a.ef, id_mask=mask, mask_bits=a.rows)           # warm-up
        s0 = g.stats()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            hi, hd, hc = g.search_batch_arrays(queries, a.k, a.ef, id_mask=mask, mask_bits=a.rows)
        dt = (time.perf_counter() - t0) / a.reps
        s1 = g.stats()
        dev = (s1["device_queries"] - s0["device_queries"]) // a.reps
        redo = (s1["host_redone"] - s0["host_redone"]) // a.reps
        ti, _, tc = flat.search_batch_arrays(queries, a.k, id_mask=mask, mask_bits=a.rows)
        assert all(elig[int(i)] for b in range(a.batch) for i in hi[b, :hc[b]])
        rec = np.mean([len(set(ti[b, :tc[b]].tolist()) & set(hi[b, :hc[b]].tolist())) / max(int(tc[b]), 1) for b in range(a.batch)])
        pi, _, pc = g.search_batch_arrays(queries, 3 * a.k, 50)
        post = [[int(i) for i in pi[b, :pc[b]] if elig[int(i)]][:a.k] for b in range(a.batch)]
        rec_post = np.mean([len(set(ti[b, :tc[b]].tolist()) & set(post[b])) / max(int(tc[b]), 1) for b in range(a.batch)])
        print(f"| {sel:g} | {a.batch / dt:.0f} | {dev} | {redo} | {rec:.4f} | {np.mean([len(p) for p in post]):.2f} | {rec_post:.4f} |", flush=True)


if __name__ == "__main__":
    main()
