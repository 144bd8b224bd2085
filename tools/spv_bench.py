#!/usr/bin/env python3
"""Sparse-vector search (GpuSparseIndex) at a SPLADE-like shape, against the best composition available without it: a torch
CSR x dense-query product on the same GPU plus topk -- or, where this ROCm build of torch cannot do that, a numpy pass over the
CSR arrays on the host, measured on two queries and labelled per query.  Warm-up, then the two alternate; median, min and max of
each are recorded.  Writes one JSON object to --out and prints it.

--route 0 | 1 | 2 measures that route of the index (vdb_spv_set_route) as before; --route both alternates route 0, route 1 and the
baseline in one process, once per --query-min-rank R given (query indices drawn from the words of frequency rank >= R only: 0 is
the Zipf workload, 1000 one off the head of the distribution), records both routes' counted work, interpolates in log space the
ratio of the two counts at which the routes' times cross (rho) when two workloads fall on either side of it, and adds k = 1024
and a half-selective id mask on the first workload.

--segmented measures the segmented inverted walk (vdb_spv_set_segmented) at 4096, 8192 and 16384 rows per segment against the
one-workgroup walk, route 1 and the baseline, alternating, at 1, 4, 16 and 256 queries of every --query-min-rank, and the flush
times with the option off and on."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package():
    pkg = os.path.join(ROOT, "vectordb-from-scratch_amd")
    spec = importlib.util.spec_from_file_location("vectordb_from_scratch_amd", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vectordb_from_scratch_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def zipf_rows(rng, n, vocab, draws, cdf):
    """n sparse rows: `draws` Zipf-distributed indices each, repeats dropped -> (offsets, indices u32 ascending per row, values)"""
    d = np.searchsorted(cdf, rng.random((n, draws), dtype=np.float32)).astype(np.int32)
    np.minimum(d, vocab - 1, out=d)
    d.sort(axis=1)
    keep = np.ones(d.shape, dtype=bool)
    keep[:, 1:] = d[:, 1:] != d[:, :-1]
    offs = np.zeros(n + 1, dtype=np.uintp)
    np.cumsum(keep.sum(axis=1), out=offs[1:])
    idx = d[keep].astype(np.uint32)
    return offs, idx, rng.random(idx.size, dtype=np.float32) + np.float32(0.05)


def zipf_queries(rng, n, vocab, draws, min_rank):
    w = 1.0 / np.arange(1, vocab + 1, dtype=np.float64)
    w[:min_rank] = 0.0
    return zipf_rows(rng, n, vocab, draws, np.cumsum(w / w.sum()).astype(np.float32))


def both_routes(ix, queries, k, rounds, base=None, **mask):
    """route 0, route 1 (and the baseline) alternating -> {"route0": spread, "route1": spread, "baseline": spread, work counts}"""
    def run(route):
        ix.set_route(route)
        t0 = time.perf_counter()
        r = ix.search_batch_arrays(queries, k, **mask)
        return (time.perf_counter() - t0) * 1e3, r
    for route in (0, 1, 0, 1):
        run(route)
    t = {0: [], 1: [], "base": []}
    for _ in range(rounds):
        for route in (0, 1):
            ms, r = run(route)
            t[route].append(ms)
            if route == 0:
                r0, st0 = r, ix.stats()
        if base is not None:
            t["base"].append(base()[0])
    rs, st1 = ix.route_stats(), ix.stats()
    rec = {"route0": spread(t[0]), "route1": spread(t[1]), "work_inverted": rs["work_inverted"], "work_rows": rs["work_rows"],
           "passes": rs["passes"], "chunks": st1["chunks"], "entries_walked_per_query": st1["entries_walked"] / len(queries),
           "answers_and_counters_equal": bool(all(np.array_equal(a, b) for a, b in zip(r0, r)) and st0 == st1)}
    if base is not None:
        rec["baseline"] = spread(t["base"])
    return rec


SEG_ROWS, SEG_BATCHES = (4096, 8192, 16384), (1, 4, 16, 256)


def segmented_arms(vdb, a, ids, offs, idx, val, rng):
    """--segmented: the one-workgroup walk, the segmented walk at each of SEG_ROWS rows per segment (a handle each: a change of the
    setting rebuilds the file), route 1 and torch.sparse.mm + topk, alternating in one process, per query set (--query-min-rank)
    and batch size; and the flush times with the option off and on.  The arms' answers must be equal."""
    arms, rec = {}, {"shape": {"rows": a.rows, "vocab": a.vocab, "nnz": int(idx.size), "k": a.k, "rounds": a.rounds}, "flush": {}, "runs": []}
    for name, R in [("old_walk", 0)] + [("segmented_%d" % R, R) for R in SEG_ROWS]:
        ix = arms[name] = vdb.GpuSparseIndex()
        ix.set_segmented(R)
        ix.add_csr(ids, offs, idx, val)
        t0 = time.perf_counter()
        ix.flush()
        t1 = time.perf_counter()
        ix.remove(a.rows - 1)
        t2 = time.perf_counter()
        ix.flush()
        rec["flush"][name] = {"first_flush_s": t1 - t0, "flush_after_one_remove_s": time.perf_counter() - t2}
    arms["route1"] = arms["old_walk"]                    # the same handle: the route is set per call
    print(json.dumps(rec["flush"]), flush=True)
    import torch
    dev, live = torch.device("cuda:0"), a.rows - 1
    csr = torch.sparse_csr_tensor(torch.from_numpy(offs[:live + 1].astype(np.int64)), torch.from_numpy(idx[:offs[live]].astype(np.int64)),
                                  torch.from_numpy(val[:offs[live]]), size=(live, a.vocab), device=dev)

    def call(name, queries, qd):
        t0 = time.perf_counter()
        if name == "torch":
            top = torch.topk(torch.sparse.mm(csr, qd.to(dev)).t(), a.k, dim=1)
            r = (top.indices.cpu().numpy().astype(np.uint64),)
        else:
            arms[name].set_route(1 if name == "route1" else 0)
            r = arms[name].search_batch_arrays(queries, a.k)   # ends in a stream synchronise and the copy of the answers
        return (time.perf_counter() - t0) * 1e3, r

    for rank in a.query_min_rank:
        qoffs, qidx, qval = zipf_queries(rng, max(SEG_BATCHES), a.vocab, a.query_draws, rank)
        for nq in SEG_BATCHES:
            queries = [(qidx[qoffs[b]:qoffs[b + 1]], qval[qoffs[b]:qoffs[b + 1]]) for b in range(nq)]
            qd = np.zeros((a.vocab, nq), dtype=np.float32)
            for b, (qi, qv) in enumerate(queries):
                qd[qi, b] = qv
            qd = torch.from_numpy(qd)
            names = list(arms) + ["torch"]
            for _ in range(2):
                for name in names:
                    call(name, queries, qd)
            t, last = {name: [] for name in names}, {}
            for _ in range(a.rounds):
                for name in names:
                    ms, last[name] = call(name, queries, qd)
                    t[name].append(ms)
            ref = last["old_walk"]
            run = {"query_min_rank": rank, "queries": nq, "times": {name: spread(t[name]) for name in names},
                   "answers_equal": bool(all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for name in arms for x, y in zip(ref, last[name]))),
                   "torch_mean_shared_ids_of_k": float(np.mean([np.isin(last["torch"][0][b], ref[0][b]).sum() for b in range(nq)])),
                   "segments": {name: arms[name].segment_stats() for name in arms if name.startswith("segmented")}}
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
    return rec


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--row-draws", type=int, default=150)
    ap.add_argument("--query-draws", type=int, default=45)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--route", default="0", choices=["0", "1", "2", "both"])
    ap.add_argument("--query-min-rank", type=int, nargs="+", default=[0])
    ap.add_argument("--segmented", action="store_true", help="the arms of vdb_spv_set_segmented (segmented_arms)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spv_bench.json"))
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    rng = np.random.default_rng(0)
    w = 1.0 / np.arange(1, a.vocab + 1, dtype=np.float64)
    cdf = np.cumsum(w / w.sum()).astype(np.float32)
    t = time.perf_counter()
    offs, idx, val = zipf_rows(rng, a.rows, a.vocab, a.row_draws, cdf)
    qoffs, qidx, qval = zipf_queries(rng, a.queries, a.vocab, a.query_draws, a.query_min_rank[0])
    print(f"data: {idx.size} non-zeros in {a.rows} rows, {qidx.size} in {a.queries} queries, {time.perf_counter() - t:.1f} s", flush=True)
    queries = [(qidx[qoffs[b]:qoffs[b + 1]], qval[qoffs[b]:qoffs[b + 1]]) for b in range(a.queries)]
    ids = np.arange(a.rows, dtype=np.uint64)
    if a.segmented:
        rec = segmented_arms(vdb, a, ids, offs, idx, val, rng)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        return
    ix = vdb.GpuSparseIndex()
    if a.route != "both":
        ix.set_route(int(a.route))
    t = time.perf_counter()
    ix.add_csr(ids, offs, idx, val)
    t_add = time.perf_counter() - t
    t = time.perf_counter()
    ix.flush()
    t_flush = time.perf_counter() - t
    ix.remove(a.rows - 1)
    t = time.perf_counter()
    ix.flush()
    t_rebuild = time.perf_counter() - t
    print(f"add {t_add:.2f} s, first flush {t_flush:.2f} s, flush after one remove {t_rebuild:.3f} s", flush=True)

    def ours():
        t0 = time.perf_counter()
        r = ix.search_batch_arrays(queries, a.k)         # ends in a stream synchronise and the copy of the answers
        return (time.perf_counter() - t0) * 1e3, r

    # the composition without the feature
    base, base_label, base_scale = None, None, 1
    try:
        import torch
        dev = torch.device("cuda:0")
        live = a.rows - 1
        csr = torch.sparse_csr_tensor(torch.from_numpy(offs[:live + 1].astype(np.int64)), torch.from_numpy(idx[:offs[live]].astype(np.int64)),
                                      torch.from_numpy(val[:offs[live]]), size=(live, a.vocab), device=dev)
        qd = np.zeros((a.vocab, a.queries), dtype=np.float32)
        for b, (qi, qv) in enumerate(queries):
            qd[qi, b] = qv
        qd_host = torch.from_numpy(qd)

        def base():
            t0 = time.perf_counter()
            s = torch.sparse.mm(csr, qd_host.to(dev))    # [rows, queries]; the dense query block is uploaded per call, like our queries
            top = torch.topk(s.t(), a.k, dim=1)
            r = (top.indices.cpu().numpy(), top.values.cpu().numpy())
            return (time.perf_counter() - t0) * 1e3, r
        base()
        base_label = "torch.sparse.mm (CSR x dense queries) + topk on the same GPU, whole batch"
    except Exception as e:                               # noqa: BLE001 -- any refusal of this torch build sends us to the host
        print("torch CSR route unavailable:", repr(e)[:200], flush=True)
        rowid = np.repeat(np.arange(a.rows, dtype=np.int64), np.diff(offs).astype(np.int64))
        base_scale = 2

        def base():
            t0 = time.perf_counter()
            out = []
            for qi, qv in queries[:base_scale]:
                lut = np.zeros(a.vocab, dtype=np.float32)
                lut[qi] = qv
                s = np.bincount(rowid, weights=lut[idx] * val, minlength=a.rows)
                out.append(np.argsort(-s[:a.rows - 1], kind="stable")[:a.k])
            return (time.perf_counter() - t0) * 1e3 / base_scale, (np.array(out), None)
        base_label = "numpy pass over the CSR arrays on the host, PER QUERY (two queries measured)"

    if a.route == "both":
        rec = {"shape": {"rows": a.rows, "vocab": a.vocab, "nnz": int(idx.size), "queries": a.queries, "k": a.k, "rounds": a.rounds},
               "baseline_is": base_label, "workloads": []}
        for i, rank in enumerate(a.query_min_rank):
            if i:
                qoffs, qidx, qval = zipf_queries(rng, a.queries, a.vocab, a.query_draws, rank)
                queries = [(qidx[qoffs[b]:qoffs[b + 1]], qval[qoffs[b]:qoffs[b + 1]]) for b in range(a.queries)]
            w = dict(query_min_rank=rank, mean_nnz_per_query=qidx.size / a.queries,
                     **both_routes(ix, queries, a.k, a.rounds, base if i == 0 and base_scale == 1 else None))
            w["log_work_ratio"] = float(np.log(w["work_inverted"] / w["work_rows"]))
            w["log_time_ratio"] = float(np.log(w["route0"]["median_ms"] / w["route1"]["median_ms"]))
            rec["workloads"].append(w)
            print(json.dumps(w), flush=True)
            if i == 0:
                first = queries
        pts = sorted((w["log_work_ratio"], w["log_time_ratio"]) for w in rec["workloads"])
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
            if y0 < 0 <= y1:                             # route 0 faster at x0, route 1 at x1: the times cross between them
                rec["rho"] = float(np.exp(x0 - y0 * (x1 - x0) / (y1 - y0)))
        rec["k_1024"] = both_routes(ix, first, 1024, 3)
        half = np.full((a.rows + 63) // 64, 0x5555555555555555, dtype=np.uint64)
        rec["masked_half"] = both_routes(ix, first, a.k, 3, id_mask=half, mask_bits=a.rows)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return
    ours()
    ours()
    base()
    t_ours, t_base = [], []
    for _ in range(a.rounds):
        ms, r_ours = ours()
        t_ours.append(ms)
        ms, r_base = base()
        t_base.append(ms)
    st = ix.stats()
    nb = r_base[0].shape[0]
    same = [len(set(r_ours[0][b].tolist()) & set(r_base[0][b].tolist())) for b in range(nb)]
    rec = {
        "route": int(a.route),
        "shape": {"rows": a.rows, "vocab": a.vocab, "nnz": int(idx.size), "mean_nnz_per_row": idx.size / a.rows, "queries": a.queries,
                  "mean_nnz_per_query": qidx.size / a.queries, "k": a.k, "index_distribution": "Zipf, exponent 1, rows and queries alike"},
        "search_batch": spread(t_ours),
        "baseline": dict(spread(t_base), what=base_label),
        "add_bulk_s": t_add, "first_flush_s": t_flush, "flush_after_one_remove_s": t_rebuild,
        "entries_walked_per_query": st["entries_walked"] / a.queries, "candidates_per_query": st["candidates"] / a.queries, "chunks": st["chunks"],
        # two walks of 8 B per entry; per entry the fold loads and stores 4 B and the emit exchanges 4 B each way
        "bytes_per_walked_entry": 32,
        "achieved_GB_per_s": 32 * st["entries_walked"] / (np.median(t_ours) * 1e-3) / 1e9,
        "answers": {"queries_compared": nb, "mean_shared_ids_of_k": float(np.mean(same)), "min_shared_ids_of_k": int(min(same)),
                    "note": "the baseline sums in another order and scores rows without overlap as 0: near-ties may swap"},
        "not_measured": "a query whose indices are all very frequent (one workgroup walks most of the store); k = 1024; filtered searches",
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
