#!/usr/bin/env python3
"""The screening tier's large-k range at 1M x 768 (rows and queries resident in HBM, B = 256): ms per batch for k in
{100, 112, 113, 300, 1000} under Cosine and Dot, with vdb_flat_set_large_k on and off ALTERNATED in one process, plus the
exact-scan query count and the candidate depth (kprime) of the last batch of each arm.  At k = 300 and k = 1000 two more arms
alternate in the same loop: every query through the re-threshold pass (VDB_TIERS_FORCE_RETHRESHOLD) and every query through the
exact scan (VDB_TIERS_FORCE_EXACT).  Prints one JSON line.

    python tools/large_k_bench.py [--rows N] [--reps R]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="100,112,113,300,1000")
    ap.add_argument("--arms", default="1,0", help="large_k settings to alternate (1,0: on and off; 1: on only, for a profile)")
    a = ap.parse_args()
    base_arms = [int(x) for x in a.arms.split(",")]
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    rows = torch.randn((a.rows, a.dim), device=dev, generator=g, dtype=torch.float32)
    q = torch.randn((a.batch, a.dim), device=dev, generator=g, dtype=torch.float32)
    kmax = max(int(x) for x in a.ks.split(","))
    oi = torch.empty((a.batch, kmax), dtype=torch.int64, device=dev)
    od = torch.empty((a.batch, kmax), dtype=torch.float32, device=dev)
    oc = torch.empty((a.batch,), dtype=torch.int32, device=dev)
    out = {"rows": a.rows, "dim": a.dim, "batch": a.batch, "reps": a.reps, "results": []}
    for metric, name in ((1, "cosine"), (2, "dot")):
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
        ix.add_bulk_device(rows.data_ptr(), a.rows, a.dim)
        torch.cuda.synchronize()
        for k in (int(x) for x in a.ks.split(",")):
            def step():
                ix.search_batch_device(q.data_ptr(), a.batch, a.dim, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
            arms = base_arms + (["rethreshold", "exact"] if k in (300, 1000) and 1 in base_arms else [])

            def select(arm):                                     # an arm: large_k on / off, or large_k on under a forced route
                ix.set_large_k(arm if arm in (0, 1) else 1)
                ix.set_tiers({"rethreshold": ix.TIERS_FORCE_RETHRESHOLD, "exact": ix.TIERS_FORCE_EXACT}.get(arm, 0))
            times = {on: [] for on in arms}
            stats = {}
            for on in arms:                                      # warm-up of every arm
                select(on)
                step()
            for _ in range(a.reps):
                for on in arms:
                    select(on)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step()
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t0) * 1e3)
                    st = ix.last_stats()
                    stats[on] = {"exact_queries": st["exact_queries"], "kprime": st["kprime"], "bf16_screen": st["bf16_screen"],
                                 "rethreshold_queries": st["rethreshold_queries"]}
            select(1)
            for on in arms:
                t = sorted(times[on])
                out["results"].append({"metric": name, "k": k, "large_k": on, "ms_median": round(t[len(t) // 2], 3),
                                       "ms_min": round(t[0], 3), **stats[on]})
        del ix
    print(json.dumps(out))


if __name__ == "__main__":
    main()
