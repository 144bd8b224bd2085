#!/usr/bin/env python3
"""An HNSW store's pre-filtered request with the filter compiled on the device (VectorStore.set_device_filter on a
GpuHnswIndex, vdb_hnsw_search_batch_filtered) against the numpy mask on the same store and handle (one process,
one GPU, one JSON document).  200k x 128 uniform, m = 16, ef_construction = 200, B = 256, k = 10, ef = 200.

The four filter shapes of DESIGN.md 4.7 -- 1 or 4 metadata fields beside the selectivity column; a single `Eq`, or an `And` /
`Or` tree of 8 leaves -- at 50 % and 10 % of the ids eligible (the walk), and the single `Eq` at 2 % and 1 % with
set_filter_scan on (the exact scan of the eligible nodes).  The selectivity column decides who is eligible in both shapes: the
tree is And(Eq(sel), Or(six leaves over the fields, Exists(sel))), whose Or holds for every row, so both shapes leave the same
ids and differ only in what compiling them costs.

Per grid point, medians of back-to-back rounds off, on, off, on, ... after two warm-up rounds; one round is the whole request
from "have a MetadataFilter" to "the result arrays are on the host":
    off_ms   VectorStore.compile_filter (numpy) + search_batch_arrays(id_mask=...)
    on_ms    VectorStore.compile_filter_device + search_batch_arrays(compiled_mask=...) + release
The answers of the two are compared, array for array.

    python tools/hnsw_device_filter_bench.py [--rows N] [--steps S] [--out profiles/r08_hnsw_device_filter.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402

FIELDS = ["f0", "f1", "f2", "f3"]
VALUES = ["a", "b", "c", "d"]
CLASSES = [("p50", 0.50), ("p10", 0.10), ("p02", 0.02), ("p01", 0.01)]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def filters(F, n_fields, cls):
    fs = FIELDS[:n_fields]
    leaf = [F.Eq(fs[i % n_fields], VALUES[i % 4]) if i % 3 else F.Ne(fs[i % n_fields], VALUES[(i + 1) % 4]) for i in range(6)]
    always = F.Or([F.And([leaf[0], leaf[1], F.Or([leaf[2], leaf[3]])]), F.And([leaf[4], leaf[5]]), F.Exists("sel")])
    return {"eq": F.Eq("sel", cls), "tree8": F.And([F.Eq("sel", cls), always])}


def grid_point(st, ix, flt, q, k, ef, steps):
    t = {"off_ms": [], "on_ms": []}

    def off():
        t0 = time.perf_counter()
        mask, bits = st.compile_filter(flt)
        res = ix.search_batch_arrays(q, k, ef, id_mask=mask, mask_bits=bits)
        return (time.perf_counter() - t0) * 1e3, res

    def on():
        t0 = time.perf_counter()
        cm = st.compile_filter_device(flt)
        try:
            res = ix.search_batch_arrays(q, k, ef, compiled_mask=cm)
        finally:
            cm.release()
        return (time.perf_counter() - t0) * 1e3, res

    before = ix.stats()
    for r in range(steps + 2):                           # two warm-up rounds
        a, res_off = off()
        b, res_on = on()
        if r >= 2:
            t["off_ms"].append(a); t["on_ms"].append(b)
    after = ix.stats()
    for x, y in zip(res_off, res_on):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    mask, _ = st.compile_filter(flt)
    p = {"ops": len(st.filter_program(flt)), "eligible": int(np.unpackbits(mask.view(np.uint8)).sum()),
         "host_redone": after["host_redone"] - before["host_redone"], "mean_count": float(np.mean(res_on[2]))}
    p.update({key: round(med(v), 4) for key, v in t.items()})
    p["on_over_off"] = round(p["on_ms"] / p["off_ms"], 4)
    p["spread"] = {key: [round(min(v), 4), round(max(v), 4)] for key, v in t.items()}
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    n, d, B, k, ef = a.rows, a.dim, a.batch, 10, 200
    rng = np.random.default_rng(21)
    rows = rng.random((n, d), dtype=np.float32)
    q = rng.random((B, d), dtype=np.float32)
    ix = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(16, 200, 50), seed=7)
    t0 = time.perf_counter()
    ix.build_batch((np.arange(n, dtype=np.uint64), rows))
    build_s = time.perf_counter() - t0
    u = rng.random(n)
    edges = np.cumsum([0.0] + [p for _, p in CLASSES])
    sel = np.full(n, "rest", dtype=object)
    for (name, _), lo, hi in zip(CLASSES, edges[:-1], edges[1:]):
        sel[(u >= lo) & (u < hi)] = name
    doc = {"tool": "tools/hnsw_device_filter_bench.py", "rows": n, "dim": d, "metric": "euclidean", "m": 16, "ef_construction": 200,
           "batch": B, "k": k, "ef": ef, "steps": a.steps, "build_s": round(build_s, 1), "points": []}
    for n_fields in (1, 4):
        st = vdb.VectorStore.with_index(ix)
        cols = {f: np.array(VALUES, dtype=object)[rng.integers(0, 4, n)] for f in FIELDS[:n_fields]}
        cols["sel"] = sel
        st.attach_bulk_metadata(n, cols)
        st.set_device_filter(True)
        assert st.device_filter()
        for cls, scan in (("p50", 0), ("p10", 0), ("p02", 131072), ("p01", 131072)):
            ix.set_filter_scan(scan)
            for name, flt in filters(vdb.MetadataFilter, n_fields, cls).items():
                if scan and (name != "eq" or n_fields != 1):
                    continue
                p = grid_point(st, ix, flt, q, k, ef, a.steps)
                p.update({"filter": name, "fields": n_fields, "selectivity": cls, "route": "filter scan" if scan else "walk"})
                doc["points"].append(p)
        ix.set_filter_scan(0)
        st.set_device_filter(False)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
