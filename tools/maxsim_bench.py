#!/usr/bin/env python3
"""Late-interaction search (vdb_flat_search_batch_maxsim) against what a caller had to do without it, at two
shapes: 1M x 128 Dot (the late-interaction shape) and 1M x 768 Cosine; documents of 16 adjacent rows, 16 queries of 32 tokens,
k = 10, uniform rows, one process, one GPU, one handle per shape.

    maxsim      ONE call: GpuFlatIndex.search_batch_maxsim(token blocks, k, table, slot, n_codes)
    composed    what the parent commit offers: distances_batch for one distance column per token over EVERY stored id (32 columns
                of `rows` floats come down per query), then the segment minimum by document (ordered-f32), the sequential f32 sum
                in token order and the sort by (ordered score, code) in numpy.  It runs on the first --composed-queries queries
                only; the file says how many, and composed_ms_per_query is the figure to compare.

The arms alternate on the same handle after --warmup calls; mean, median and minimum of each arm's wall time per call (host clock
around a call that ends in a device synchronise) are reported, and the device clocks before and after.  The answers must be
identical: codes, score bits and counts.  Per query of the maxsim arm the file also gives the bytes of rows the algorithm needs
(rows x dim x 4: the row is read once per query) over the time against the 8 TB/s peak, and the f32 vector operations it needs
(rows x tokens x dim x 2 under Dot and Cosine: one multiply and one add per element, unfused and unpacked by the bit-exactness
contract) over the time against 39.3 T operations/s (256 CUs x 64 lanes x 2.4 GHz), and says which of the two floors is higher.
A record, not a bar: no pass / fail time is attached.

--screen-out FILE runs the SCREENED route instead (vdb_flat_set_maxsim_screen, DESIGN.md 4.19 "screened route"): at both shapes
and on two kinds of data -- the uniform i.i.d. rows above, and documents that are clusters (a gaussian centre per document, its 16
rows 0.1 gaussian around it, every query's tokens around the centre of one document) -- the exact arm (switch off: the parent
commit's code, the yardstick) and the screened arm alternate on one handle; the file holds each arm's time per call, the
screened arm's stats [6] (queries screened) and [7] (documents re-scored, summed over the queries) and the documents.  The
answers must be identical.

    python tools/maxsim_bench.py [--rows N] [--queries B] [--tokens T] [--k K] [--rounds R] [--composed-queries C]
                                 [--out profiles/maxsim_bench.json] [--screen-out profiles/maxsim_screen_bench.json]"""
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

F32, U32, U64, I32 = np.float32, np.uint32, np.uint64, np.int32
HBM_PEAK, VALU_PEAK = 8.0e12, 256 * 64 * 2.4e9
PER_DOC = 16


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def summary(v):
    return {"mean": round(sum(v) / len(v), 4), "median": round(med(v), 4), "min": round(min(v), 4)}


def ordered(d):
    b = np.asarray(d, dtype=F32).view(U32)
    return np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)


def from_ordered(u):
    return np.where(u & U32(0x80000000), u & U32(0x7fffffff), ~u).astype(U32).view(F32)


def clocks():
    """the device's current shader and memory clocks as rocm-smi prints them (read only), or None"""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2] or None
    except Exception:
        return None


def shape(vdb, a, metric, name, d):
    dev = torch.device("cuda", 0)
    n, B, T, k = a.rows // PER_DOC * PER_DOC, a.queries, a.tokens, a.k
    C = min(a.composed_queries, B)
    n_docs = n // PER_DOC
    g = torch.Generator(device=dev).manual_seed(31)
    ix = vdb.GpuFlatIndex(metric, keep_host_copy=False)
    chunk = 125_000
    for r0 in range(0, n, chunk):
        rows = torch.rand((min(chunk, n - r0), d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), rows.shape[0], d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, (np.arange(n) // PER_DOC).astype(I32))
    toks = [np.ascontiguousarray(x) for x in np.random.default_rng(37).random((B, T, d), dtype=F32)]
    all_ids = np.arange(n, dtype=U64)

    def device():
        t0 = time.perf_counter()
        res = ix.search_batch_maxsim(toks, k, table, 0, n_docs)
        return (time.perf_counter() - t0) * 1e3, res, ix.maxsim_stats()

    def composed():
        oc, os_ = np.zeros((C, k), dtype=I32), np.zeros((C, k), dtype=F32)
        parts = [0.0, 0.0]
        t0 = time.perf_counter()
        for b in range(C):
            ta = time.perf_counter()
            cols = ix.distances_batch(toks[b], [all_ids] * T)
            tb = time.perf_counter()
            score = None
            for t in range(T):
                m = from_ordered(ordered(cols[t]).reshape(n_docs, PER_DOC).min(axis=1))
                score = m if score is None else (score + m).astype(F32)
            o = np.lexsort((np.arange(n_docs), ordered(score)))[:k]
            oc[b], os_[b] = o, score[o]
            parts[0] += (tb - ta) * 1e3
            parts[1] += (time.perf_counter() - tb) * 1e3
        return (time.perf_counter() - t0) * 1e3, (oc, os_), parts

    before = clocks()
    for _ in range(a.warmup):
        device()
    td, tc, parts = [], [], []
    for r in range(a.rounds):
        t, rd, st = device()
        td.append(t)
        if r < a.composed_rounds and C:
            t, rc, p = composed()
            tc.append(t)
            parts.append(p)
    after = clocks()
    assert (rd[2] == k).all()
    for b in range(C if tc else 0):
        assert np.array_equal(rd[0][b], rc[0][b]) and np.array_equal(rd[1][b].view(U32), rc[1][b].view(U32)), b
    per_q = med(td) / B * 1e-3
    row_bytes, ops = n * d * 4, n * T * d * 2
    t_hbm, t_valu = row_bytes / HBM_PEAK, ops / VALU_PEAK
    doc = {"shape": name, "rows": n, "dim": d, "metric": name.split()[-1], "queries": B, "tokens_per_query": T, "k": k, "rows_per_document": PER_DOC,
           "rounds": a.rounds, "warmup": a.warmup, "clocks_before": before, "clocks_after": after,
           "maxsim_ms": summary(td), "maxsim_stats": st, "maxsim_ms_per_query": round(per_q * 1e3, 4),
           "row_bytes_per_query": row_bytes, "row_bytes_per_s": round(row_bytes / per_q / 1e12, 4), "row_bytes_share_of_8TBps": round(t_hbm / per_q, 4),
           "f32_vector_ops_per_query": ops, "f32_vector_Tops_per_s": round(ops / per_q / 1e12, 3), "f32_vector_share_of_39.3Tops": round(t_valu / per_q, 4),
           "higher_floor": "f32 vector operations" if t_valu > t_hbm else "row bytes",
           "note": "whole-call wall time over the queries (token upload, preparation, memset, scan, fold, select, emit, copy-out): an end-to-end "
                   "rate, not the scan kernel's share of peak"}
    if tc:
        doc.update({"composed_queries": C, "composed_rounds": len(tc), "composed_ms": summary(tc), "composed_ms_per_query": round(med(tc) / C, 4),
                    "composed_parts_ms": {"distances_batch": round(med([p[0] for p in parts]), 4), "host_min_sum_sort": round(med([p[1] for p in parts]), 4)},
                    "composed_per_query_over_maxsim_per_query": round((med(tc) / C) / (med(td) / B), 1), "answers_identical": True})
    table.close()
    return doc


def screen_shape(vdb, a, metric, name, d, data):
    dev = torch.device("cuda", 0)
    n, B, T, k = a.rows // PER_DOC * PER_DOC, a.queries, a.tokens, a.k
    n_docs = n // PER_DOC
    g = torch.Generator(device=dev).manual_seed(31)
    ix = vdb.GpuFlatIndex(metric, keep_host_copy=False)
    rng = np.random.default_rng(37)
    if data == "clustered":
        centres = torch.randn((n_docs, d), device=dev, generator=g, dtype=torch.float32)
        toks = [np.ascontiguousarray(centres[int(c)].cpu().numpy() + 0.1 * rng.standard_normal((T, d)), dtype=F32) for c in rng.integers(0, n_docs, B)]
    else:
        toks = [np.ascontiguousarray(x) for x in rng.random((B, T, d), dtype=F32)]
    chunk = 125_000 // PER_DOC * PER_DOC
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        if data == "clustered":
            rows = centres[r0 // PER_DOC:(r0 + m) // PER_DOC].repeat_interleave(PER_DOC, dim=0) + 0.1 * torch.randn((m, d), device=dev, generator=g, dtype=torch.float32)
        else:
            rows = torch.rand((m, d), device=dev, generator=g, dtype=torch.float32)
        ix.add_bulk_device(rows.data_ptr(), m, d, first_id=r0)
        torch.cuda.synchronize()
    ix.flush()
    del rows
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, (np.arange(n) // PER_DOC).astype(I32))

    def call(on):
        ix.set_maxsim_screen(on)
        t0 = time.perf_counter()
        res = ix.search_batch_maxsim(toks, k, table, 0, n_docs)
        return (time.perf_counter() - t0) * 1e3, res, ix.maxsim_stats()

    before = clocks()
    for _ in range(a.warmup):
        call(False), call(True)
    te, ts = [], []
    for _ in range(a.rounds):
        t, re_, _ = call(False)
        te.append(t)
        t, rs, st = call(True)
        ts.append(t)
    for x, y in zip(re_, rs):
        assert np.array_equal(np.asarray(x).view(U32) if x.dtype == F32 else x, np.asarray(y).view(U32) if y.dtype == F32 else y)
    table.close()
    return {"shape": name, "data": data, "rows": n, "dim": d, "metric": name.split()[-1], "queries": B, "tokens_per_query": T, "k": k,
            "rows_per_document": PER_DOC, "documents": n_docs, "rounds": a.rounds, "warmup": a.warmup, "clocks_before": before, "clocks_after": clocks(),
            "exact_ms": summary(te), "screened_ms": summary(ts), "screened_over_exact": round(med(ts) / med(te), 3),
            "queries_screened": st[6], "documents_rescored": st[7], "documents_rescored_per_query": round(st[7] / max(st[6], 1), 1),
            "rows_folded_exactly": st[3], "answers_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--composed-queries", type=int, default=1)
    ap.add_argument("--composed-rounds", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--screen-out", default="")
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    if a.screen_out:
        doc = {"tool": "tools/maxsim_bench.py --screen-out",
               "shapes": [screen_shape(vdb, a, m, name, d, data) for data in ("iid", "clustered")
                          for m, name, d in ((vdb.DistanceMetric.DotProduct, "1M x 128 dot", 128), (vdb.DistanceMetric.Cosine, "1M x 768 cosine", 768))]}
        with open(a.screen_out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc))
        return
    doc = {"tool": "tools/maxsim_bench.py",
           "shapes": [shape(vdb, a, vdb.DistanceMetric.DotProduct, "1M x 128 dot", 128), shape(vdb, a, vdb.DistanceMetric.Cosine, "1M x 768 cosine", 768)]}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
