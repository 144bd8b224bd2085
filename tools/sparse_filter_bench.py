#!/usr/bin/env python3
"""The sparse-filter route (vdb_flat_set_sparse_filter) against the tiers, same mask, same handle (one process, one GPU, one
JSON document).  Shapes: 1M x 768 Cosine, 1M x 1536 Euclid (BASELINE config 4's shape), 200k x 128 Euclid; nq in {1, 16, 256};
selectivity in {0.01, 0.1, 1, 2, 5, 10 %} of the rows (uniformly scattered); k = 10.  Per grid point, device-resident calls:

    ms_mode0   the masked search with the route off          } back-to-back rounds 0, 1, (2,) 0, 1, (2,) ...; medians
    ms_mode1   ... with the route forced                     }
    ms_mode2   ... with the automatic mode (--mode2)         }
    routed1 / routed2   whether the route answered (sparse_stats()[0]);  limit = vdb_flat_sparse_limit for the shape
    c_break_even        E nq dim / (n ld) at this point -- where ms_mode1 <= ms_mode0 the constant C may be at least this

and the answers of the modes are compared (ids, distance bits, counts).  The HNSW part (200k x 128, m = 16, ef = 200, batch 64)
records queries/s of vdb_hnsw_search_batch_masked with and without vdb_hnsw_set_filter_scan at 10, 5, 2, 1, 0.1 % selectivity.

    python tools/sparse_filter_bench.py [--mode2] [--shapes a,b,c] [--steps S] [--no-hnsw] [--out profiles/r06_sparse_filter_bench.json]"""
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

SHAPES = {"1m768": (1_000_000, 768, "Cosine"), "1m1536": (1_000_000, 1536, "Euclidean"), "200k128": (200_000, 128, "Euclidean")}
SELECTIVITY = [0.0001, 0.001, 0.01, 0.02, 0.05, 0.10]
BATCHES = [1, 16, 256]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def mask_words(ids, bits):
    m = np.zeros((bits + 63) // 64, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.uint64)
    np.bitwise_or.at(m, (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
    return m


def flat_grid(vdb, name, modes, steps, dev):
    n, d, metric = SHAPES[name]
    ld = (d + 31) // 32 * 32
    k = 10
    g = torch.Generator(device=dev).manual_seed(21)
    rows = torch.randn((n, d), device=dev, generator=g, dtype=torch.float32)
    ix = vdb.GpuFlatIndex(getattr(vdb.DistanceMetric, metric), keep_host_copy=False)
    ix.add_bulk_device(rows.data_ptr(), n, d)
    ix.flush()
    del rows
    rng = np.random.default_rng(7)
    points = []
    for nq in BATCHES:
        q = torch.randn((nq, d), device=dev, generator=g, dtype=torch.float32)
        outs = {m: (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                    torch.empty((nq,), dtype=torch.int32, device=dev)) for m in modes}
        for sel in SELECTIVITY:
            E = max(1, int(round(n * sel)))
            keep = np.sort(rng.choice(n, size=E, replace=False))
            m_t = torch.from_numpy(mask_words(keep, n).view(np.int64)).to(dev)
            routed = {}

            def step(mode):
                ix.set_sparse_filter(mode)
                o = outs[mode]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ix.search_batch_device(q.data_ptr(), nq, d, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                       mask_ptr=m_t.data_ptr(), mask_bits=n)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                routed[mode] = ix.sparse_stats()[0]
                return dt

            for _ in range(2):
                for mode in modes:
                    step(mode)
            ts = {m: [] for m in modes}
            for _ in range(steps):
                for mode in modes:
                    ts[mode].append(step(mode))
            ix.set_sparse_filter(0)
            ref = outs[0]
            cnt = ref[2].cpu().numpy()
            for mode in modes[1:]:
                o = outs[mode]
                assert torch.equal(o[2], ref[2]), (name, nq, sel, mode)
                for b in range(nq):
                    c = int(cnt[b])
                    assert torch.equal(o[0][b, :c], ref[0][b, :c]) and torch.equal(o[1][b, :c].view(torch.int32), ref[1][b, :c].view(torch.int32)), (name, nq, sel, mode, b)
            p = {"nq": nq, "selectivity": sel, "eligible": E, "limit": vdb.GpuFlatIndex.sparse_limit(n, ld, d, nq),
                 "c_break_even": round(E * nq * d / (n * ld), 6)}
            for mode in modes:
                p["ms_mode%d" % mode] = round(med(ts[mode]), 4)
                if mode:
                    p["routed%d" % mode] = routed[mode]
                    p["mode%d_over_mode0" % mode] = round(med(ts[mode]) / med(ts[0]), 3)
            points.append(p)
    del ix
    torch.cuda.empty_cache()
    return {"shape": name, "rows": n, "dim": d, "metric": metric.lower(), "k": k, "steps": steps, "points": points}


def hnsw_rates(vdb, steps):
    n, d, B, k, ef = 200_000, 128, 64, 10, 200
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(16, 200, ef), seed=1)
    g.build_batch((np.arange(n, dtype=np.uint64), rows))
    out = []
    for sel in (0.10, 0.05, 0.02, 0.01, 0.001):
        keep = np.sort(rng.choice(n, size=int(n * sel), replace=False))
        m = mask_words(keep, n)
        r = {"selectivity": sel, "eligible": int(keep.size)}
        for label, limit in (("walk_qps", 0), ("filter_scan_qps", 131072)):
            g.set_filter_scan(limit)
            g.search_batch_arrays(q, k, ef, id_mask=m, mask_bits=n)
            ts = []
            for _ in range(steps):
                t0 = time.perf_counter()
                g.search_batch_arrays(q, k, ef, id_mask=m, mask_bits=n)
                ts.append(time.perf_counter() - t0)
            r[label] = round(B / med(ts), 1)
        g.set_filter_scan(0)
        out.append(r)
    return {"rows": n, "dim": d, "m": 16, "ef": ef, "batch": B, "k": k, "rates": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode2", action="store_true", help="also time the automatic mode")
    ap.add_argument("--shapes", default="1m768,1m1536,200k128")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--no-hnsw", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    modes = [0, 1, 2] if a.mode2 else [0, 1]
    doc = {"tool": "tools/sparse_filter_bench.py", "modes": modes, "flat": [], "hnsw": None}
    for name in [s for s in a.shapes.split(",") if s]:
        doc["flat"].append(flat_grid(vdb, name, modes, a.steps, dev))
    if not a.no_hnsw:
        doc["hnsw"] = hnsw_rates(vdb, max(3, a.steps // 2))
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
