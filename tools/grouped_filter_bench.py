#!/usr/bin/env python3
"""One batch, a filter per query: the grouped call (vdb_flat_search_batch_grouped) against what exists without
it, a loop of one masked search per filter.  1M x 768 Cosine, B = 256 queries, k = 10; the masks are G disjoint tenants with
G in {4, 32, 256} -- selectivity 1 / G, B / G queries per tenant, the tenants interleaved through the batch.  Same process, same
handle, host-pointer calls (queries and masks uploaded by every call; the compiled arm uploads the queries only), back-to-back
rounds: grouped, grouped under compiled masks, loop with the sparse-filter route forced, loop in the default mode,
grouped, ...; medians.

    ms_grouped        one search_batch_grouped call
    ms_grouped_compiled   the same call under masks compiled on the device beforehand (MetaTable.compile): nothing but the queries
                      goes up
    ms_loop_sparse    G search_batch_arrays calls with set_sparse_filter(1)
    ms_loop_default   G search_batch_arrays calls with set_sparse_filter(0)
    grouped_stats     of the grouped call

The answers of all arms are compared (ids, distance bits, counts).

    python tools/grouped_filter_bench.py [--rows N] [--dim D] [--groups 4,32,256] [--rounds 30] [--out profiles/r13_grouped_filter_bench.json]"""
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
    ap.add_argument("--groups", default="4,32,256")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k = a.rows, a.dim, a.batch, 10
    g = torch.Generator(device=dev).manual_seed(21)
    rows = torch.randn((n, d), device=dev, generator=g, dtype=torch.float32)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
    ix.add_bulk_device(rows.data_ptr(), n, d)
    ix.flush()
    del rows
    torch.cuda.empty_cache()
    rng = np.random.default_rng(7)
    q = rng.standard_normal((B, d)).astype(np.float32)
    words = (n + 63) // 64
    points = []
    table = vdb.MetaTable(0)
    table.set_present(0, n, True)
    for G in [int(x) for x in a.groups.split(",") if x]:
        tenant = rng.integers(0, G, size=n)
        masks = np.zeros((G, words), dtype=np.uint64)
        ids = np.arange(n, dtype=np.uint64)
        for t in range(G):
            sel = ids[tenant == t]
            np.bitwise_or.at(masks[t], (sel >> np.uint64(6)).astype(np.int64), np.uint64(1) << (sel & np.uint64(63)))
        group_of = (np.arange(B) % G).astype(np.uint32)             # the tenants interleaved through the batch
        members = [np.nonzero(group_of == t)[0] for t in range(G)]
        members = [(t, m) for t, m in enumerate(members) if m.size]
        blocks = [np.ascontiguousarray(q[m]) for _, m in members]

        def grouped():
            return ix.search_batch_grouped(q, k, group_of, id_masks=masks, mask_bits=n)

        def loop(mode):
            ix.set_sparse_filter(mode)
            oi = np.zeros((B, k), dtype=np.uint64)
            od = np.zeros((B, k), dtype=np.float32)
            oc = np.zeros(B, dtype=np.uintp)
            for (t, m), qb in zip(members, blocks):
                i, dd, c = ix.search_batch_arrays(qb, k, id_mask=masks[t], mask_bits=n)
                oi[m], od[m], oc[m] = i, dd, c
            ix.set_sparse_filter(0)
            return oi, od, oc

        table.set_codes(0, 0, tenant.astype(np.int32))
        cms = [table.compile([(vdb.MetaTable.EQ, 0, t)], n) for t in range(G)]

        def grouped_compiled():
            return ix.search_batch_grouped(q, k, group_of, compiled_masks=cms)

        variants = [("grouped", grouped), ("grouped_compiled", grouped_compiled), ("loop_sparse", lambda: loop(1)), ("loop_default", lambda: loop(0))]
        res = {}
        for name, f in variants:                                    # warm-up: buffers sized, answers kept
            f()
            res[name] = f()
        stats = None
        for name in ("grouped_compiled", "loop_sparse", "loop_default"):
            for x, y in zip(res["grouped"], res[name]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (G, name)
        ts = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, f in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[name].append((time.perf_counter() - t0) * 1e3)
                if name == "grouped":
                    stats = ix.grouped_stats()
        p = {"groups": G, "selectivity": round(1.0 / G, 6), "queries_per_group": B // G if G <= B else 1, "grouped_stats": stats}
        for name, _ in variants:
            p["ms_" + name] = round(med(ts[name]), 4)
        p["loop_sparse_over_grouped"] = round(p["ms_loop_sparse"] / p["ms_grouped"], 3)
        p["loop_default_over_grouped"] = round(p["ms_loop_default"] / p["ms_grouped"], 3)
        points.append(p)
        for cm in cms:
            cm.release()
    doc = {"tool": "tools/grouped_filter_bench.py", "rows": n, "dim": d, "metric": "cosine", "batch": B, "k": k, "rounds": a.rounds,
           "points": points}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
