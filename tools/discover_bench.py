#!/usr/bin/env python3
"""Discovery search (vdb_flat_discover_batch) against what a caller had to do without it, at the headline shape:
1M x 768 Cosine, 256 requests of a target and 4 (positive, negative) pairs, k = 10, uniform rows as bench.py's config c2 draws them,
one process, one GPU, one handle.

    auto        ONE call: GpuFlatIndex.discover_batch(targets, pairs, k); the stage counts come from discover_stats
    scan        the same call forced to the exact scan (debug_set_discover_route(2)): one pass over the rows per request
    composed    what the parent commit offers: get_vector for the 2 P + 1 examples of a request, distances_batch for their
                distance columns over EVERY stored id (the exact reference distances, 2 P + 1 columns of `rows` floats come down),
                then the rank fold, the strike and the sort by (rank descending, ordered distance, id) in numpy.  A column costs
                about as much as a request's whole scan, so this arm runs on the first --composed-requests requests only; the file
                says how many, and composed_ms_per_request is the figure to scale.

The arms take host ids in and hand host arrays out and run on the same handle, round by round after --warmup calls; mean, median
and minimum of each arm's wall time per call are reported, and the device clocks before and after.  The answers must be identical:
ids, distance bits, ranks and counts of auto and scan for every request, and of the composed arm for its requests.  A record, not
a bar: no pass / fail time is attached.

    python tools/discover_bench.py [--rows N] [--dim D] [--requests B] [--pairs P] [--k K] [--rounds R] [--composed-requests C]
                                   [--composed-rounds M] [--out profiles/discover_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402

F32, U32, U64 = np.float32, np.uint32, np.uint64


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def summary(v):
    return {"mean": round(sum(v) / len(v), 4), "median": round(med(v), 4), "min": round(min(v), 4)}


def ordered(d):
    b = np.asarray(d, dtype=F32).view(U32)
    return np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)


def clocks():
    """the device's current shader and memory clocks as rocm-smi prints them (read only), or None"""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2] or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--composed-requests", type=int, default=4)
    ap.add_argument("--composed-rounds", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k, P = a.rows, a.dim, a.requests, a.k, a.pairs
    m = 2 * P + 1
    C = min(a.composed_requests, B)
    g = torch.Generator(device=dev).manual_seed(21)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    ex = np.random.default_rng(29).choice(n, B * m, replace=False).astype(U64).reshape(B, m)
    targets = ex[:, 0].copy()
    pairs = [r[1:].reshape(P, 2) for r in ex]
    depth = int(vdb._ffi.lib().vdb_flat_discover_depth(k, P, n, 0))
    all_ids = np.arange(n, dtype=U64)

    def device(route):
        ix.debug_set_discover_route(route)
        t0 = time.perf_counter()
        res = ix.discover_batch(targets, pairs, k)
        t = (time.perf_counter() - t0) * 1e3
        ix.debug_set_discover_route(0)
        return t, res, ix.discover_stats()

    def composed():
        oi = np.zeros((C, k), dtype=U64)
        od = np.zeros((C, k), dtype=F32)
        orank = np.zeros((C, k), dtype=U32)
        parts = [0.0, 0.0, 0.0]
        t0 = time.perf_counter()
        for b in range(C):
            ta = time.perf_counter()
            q = np.stack([np.asarray(ix.get_vector(int(e)).data, dtype=F32) for e in ex[b]])
            tb = time.perf_counter()
            cols = ix.distances_batch(q, [all_ids] * m)
            tc = time.perf_counter()
            rank = np.zeros(n, dtype=np.int64)
            for i in range(P):
                rank += cols[1 + 2 * i] < cols[2 + 2 * i]
            ok = np.ones(n, dtype=bool)
            ok[ex[b].astype(np.int64)] = False
            sel = np.nonzero(ok)[0]
            o = sel[np.lexsort((all_ids[sel], ordered(cols[0][sel]), -rank[sel]))[:k]]
            oi[b], od[b], orank[b] = all_ids[o], cols[0][o], rank[o]
            td = time.perf_counter()
            for i, v in enumerate((tb - ta, tc - tb, td - tc)):
                parts[i] += v * 1e3
        return (time.perf_counter() - t0) * 1e3, (oi, od, orank), parts

    before = clocks()
    for _ in range(a.warmup):
        device(0)
    device(2)
    ta, ts, tc, parts = [], [], [], []
    for r in range(a.rounds):
        t, ra, sa = device(0)
        ta.append(t)
        t, rs, ss = device(2)
        ts.append(t)
        if r < a.composed_rounds and C:
            t, rc, p = composed()
            tc.append(t)
            parts.append(p)
    after = clocks()
    for b in range(B):
        c = int(ra[3][b])
        assert c == int(rs[3][b]) == k, b
        assert np.array_equal(ra[0][b, :c], rs[0][b, :c]) and np.array_equal(ra[2][b, :c], rs[2][b, :c]), b
        assert np.array_equal(ra[1][b, :c].view(U32), rs[1][b, :c].view(U32)), b
        if b < C and tc:
            assert np.array_equal(ra[0][b, :c], rc[0][b]) and np.array_equal(ra[2][b, :c], rc[2][b]), b
            assert np.array_equal(ra[1][b, :c].view(U32), rc[1][b].view(U32)), b
    part = lambda i: round(med([p[i] for p in parts]), 4)
    doc = {"tool": "tools/discover_bench.py", "rows": n, "dim": d, "requests": B, "pairs": P, "k": k, "metric": "cosine",
           "rounds": a.rounds, "warmup": a.warmup, "stage0_depth": depth, "clocks_before": before, "clocks_after": after,
           "auto_ms": summary(ta), "auto_stats": sa, "scan_ms": summary(ts), "scan_stats": ss,
           "scan_over_auto": round(med(ts) / med(ta), 2), "answers_identical": True}
    if tc:
        doc.update({"composed_requests": C, "composed_rounds": len(tc), "composed_ms": summary(tc),
                    "composed_ms_per_request": round(med(tc) / C, 4),
                    "composed_parts_ms": {"get_vector": part(0), "distances_batch": part(1), "host_fold_and_sort": part(2)},
                    "composed_note": "the composed arm ran on the first %d of the %d requests only: a distance column costs about as "
                                     "much as a request's whole scan; composed_ms is for those requests, scale composed_ms_per_request" % (C, B),
                    "composed_per_request_over_auto_per_request": round((med(tc) / C) / (med(ta) / B), 1)})
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
