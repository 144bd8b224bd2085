#!/usr/bin/env python3
"""Numeric range predicates (MetadataFilter.Lt / Le / Gt / Ge) compiled on the device against the numpy path, on
the same store and handle (one process, one GPU, one JSON document) -- tools/filter_compile_bench.py for the numeric leaves.
1M ids, one string field (4 values) and two numeric columns:

    low   100 distinct numbers: the LUT is 800 bytes, every gather hits a cache
    ts    one distinct number per row, codes in random order over the rows: the timestamp case, an 8 MB LUT gathered at random

and per column a single `Lt` (25 % of the rows), `And([Ge, Lt])` (a band of 50 %) and an 8-leaf tree mixing string and numeric
leaves.  Per grid point, medians (and min / max) of back-to-back rounds host, device, host, device, ... after two warm-up rounds;
the columns are those of filter_compile_bench.py:

    host_compile_ms + host_upload_ms  against  device_enqueue_ms / device_complete_ms
    call_host_ms / call_device_ms     VectorStore.search_batch_prefiltered at 1M x 768 Cosine, B = 256, k = 10; the answers are compared

    python tools/numeric_filter_bench.py [--rows N] [--steps S] [--out profiles/r14_numeric_filter_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench import load_package  # noqa: E402
from filter_compile_bench import grid_point, med  # noqa: E402,F401

VALUES = ["a", "b", "c", "d"]
TS0 = 1_700_000_000


def filters(F, col, lo, q1, mid, q3):
    """lo .. the column's smallest number, q1 / mid / q3 its quartiles"""
    tree = F.Or([F.And([F.Ge(col, q1), F.Lt(col, q3), F.Or([F.Eq("f0", "a"), F.Ne("f0", "b")])]),
                 F.And([F.Eq("f0", "c"), F.Or([F.Lt(col, q1), F.Gt(col, q3), F.Le(col, lo)])])])
    return {"lt": F.Lt(col, q1), "band": F.And([F.Ge(col, q1), F.Lt(col, q3)]), "tree8": tree}


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
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
    ix.add_bulk_device(rows.data_ptr(), n, d)
    ix.flush()
    st = vdb.VectorStore(index=ix)
    cols = {"f0": np.array(VALUES, dtype=object)[rng.integers(0, 4, n)],
            "low": rng.integers(0, 100, n).astype(str).astype(object),
            "ts": (TS0 + rng.permutation(n)).astype(str).astype(object)}
    st.attach_bulk_metadata(n, cols)
    doc = {"tool": "tools/numeric_filter_bench.py", "rows": n, "dim": d, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "points": []}
    quartiles = {"low": (0.0, 25.0, 50.0, 75.0), "ts": (float(TS0), float(TS0 + n // 4), float(TS0 + n // 2), float(TS0 + 3 * (n // 4)))}
    for col in ("low", "ts"):
        for name, flt in filters(vdb.MetadataFilter, col, *quartiles[col]).items():
            consts = st.filter_program(flt, with_consts=True)[1]
            p = grid_point(vdb, st, name, flt, queries, a.steps, dev)
            p["column"], p["distinct"], p["lut_bytes"], p["constants"] = col, len(st._cols[col].values), 8 * len(st._cols[col].values), len(consts)
            doc["points"].append(p)
    lo, hi = ({p["filter"]: p["device_complete_ms"] for p in doc["points"] if p["column"] == c} for c in ("low", "ts"))
    doc["ts_over_low_device_complete"] = {f: round(hi[f] / lo[f], 3) for f in lo}
    st.set_device_filter(False)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
