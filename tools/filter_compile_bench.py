#!/usr/bin/env python3
"""Filters compiled on the device (VectorStore.set_device_filter) against the numpy path, on the same store and
handle (one process, one GPU, one JSON document).  1M ids with 1 and with 4 metadata fields; a single `Eq` (25 % of the rows) and
an `And` / `Or` tree of 8 leaves.  Per grid point, medians of back-to-back rounds host, device, host, device, ...:

    pre-search: from "have a MetadataFilter" to "the search may start"
      host_compile_ms    VectorStore.compile_filter (numpy passes + packbits)
      host_upload_ms     the mask from pageable host memory into a device buffer, to completion (what the host-mask call does first)
      device_enqueue_ms  VectorStore.compile_filter_device returns: translated, validated, kernel enqueued -- a search enqueued
                         behind the mask's event may be submitted from here on
      device_complete_ms the same call + the wait for the mask's event + the 8-byte eligible count on the host
    whole call: VectorStore.search_batch_prefiltered at 1M x 768 Cosine, B = 256, k = 10
      call_host_ms / call_device_ms   the numpy compile + host-mask call (the setting off) / the setting on; the answers are compared

    python tools/filter_compile_bench.py [--rows N] [--steps S] [--out profiles/r07_filter_compile.json]"""
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

FIELDS = ["f0", "f1", "f2", "f3"]
VALUES = ["a", "b", "c", "d"]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def filters(F, n_fields):
    fs = FIELDS[:n_fields]
    leaf = [F.Eq(fs[i % n_fields], VALUES[i % 4]) if i % 3 else F.Ne(fs[i % n_fields], VALUES[(i + 1) % 4]) for i in range(8)]
    tree = F.Or([F.And([leaf[0], leaf[1], F.Or([leaf[2], leaf[3]])]), F.And([leaf[4], F.Or([leaf[5], leaf[6], leaf[7]])])])
    return {"eq": F.Eq("f0", "a"), "tree8": tree}


def grid_point(vdb, st, name, flt, queries, steps, dev):
    n = st._next_id
    d_mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    t = {k: [] for k in ("host_compile_ms", "host_upload_ms", "device_enqueue_ms", "device_complete_ms", "call_host_ms", "call_device_ms")}

    def pre_host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask, bits = st.compile_filter(flt)
        t1 = time.perf_counter()
        d_mask.copy_(torch.from_numpy(mask.view(np.int64)))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, mask

    def pre_device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cm = st.compile_filter_device(flt)
        t1 = time.perf_counter()
        count = cm.count()
        t2 = time.perf_counter()
        cm.release()
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, count

    def call(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if on:
            res = st.search_batch_prefiltered(queries, flt)
        else:                                            # the body of search_batch_prefiltered with the setting off (the table stays resident)
            for qv, _ in queries:
                st._check_dim(qv)
            mask, bits = st.compile_filter(flt)
            res = [st._map(r) for r in st._index.search_batch(list(queries), id_mask=mask, mask_bits=bits)]
        return (time.perf_counter() - t0) * 1e3, res

    st.set_device_filter(True)
    for r in range(steps + 2):                           # two warm-up rounds
        a, b, mask = pre_host()
        c, e, count = pre_device()
        if r >= 2:
            t["host_compile_ms"].append(a); t["host_upload_ms"].append(b); t["device_enqueue_ms"].append(c); t["device_complete_ms"].append(e)
    eligible = int(np.unpackbits(mask.view(np.uint8)).sum())
    assert count == eligible, (count, eligible)
    for r in range(steps + 2):
        h, res_h = call(False)
        g, res_d = call(True)
        if r >= 2:
            t["call_host_ms"].append(h); t["call_device_ms"].append(g)
    same = all([(x.id, np.float32(x.distance).view(np.uint32)) for x in a_] == [(y.id, np.float32(y.distance).view(np.uint32)) for y in b_]
               for a_, b_ in zip(res_h, res_d))
    assert same, name
    p = {"filter": name, "ops": len(st.filter_program(flt)), "eligible": eligible}
    p.update({k: round(med(v), 4) for k, v in t.items()})
    p["pre_search_host_ms"] = round(med(t["host_compile_ms"]) + med(t["host_upload_ms"]), 4)
    p["spread"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    n, d, B, k = a.rows, a.dim, a.batch, 10
    g = torch.Generator(device=dev).manual_seed(21)
    rows = torch.randn((n, d), device=dev, generator=g, dtype=torch.float32)
    q = torch.randn((B, d), device=dev, generator=g, dtype=torch.float32).cpu().numpy()
    queries = [(vdb.Vector(q[b]), k) for b in range(B)]
    rng = np.random.default_rng(7)
    doc = {"tool": "tools/filter_compile_bench.py", "rows": n, "dim": d, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "points": []}
    for n_fields in (1, 4):
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
        ix.add_bulk_device(rows.data_ptr(), n, d)
        ix.flush()
        st = vdb.VectorStore(index=ix)
        st.attach_bulk_metadata(n, {f: np.array(VALUES, dtype=object)[rng.integers(0, 4, n)] for f in FIELDS[:n_fields]})
        for name, flt in filters(vdb.MetadataFilter, n_fields).items():
            p = grid_point(vdb, st, name, flt, queries, a.steps, dev)
            p["fields"] = n_fields
            doc["points"].append(p)
        st.set_device_filter(False)
        del st, ix
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
