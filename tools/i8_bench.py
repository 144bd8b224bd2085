#!/usr/bin/env python3
"""Int8 flat search (GpuInt8Index) at an embedding-model shape against the two ways a caller has without it: GpuFlatIndex over the
same values widened to f32 (after its split conversion: the 2 B/element screen), and a torch matmul over the widened rows plus
topk on the same GPU.  The three arms run in one process, alternating; every arm is warmed up; each of --rounds rounds times
--calls calls per arm, and the median, minimum and maximum of the rounds' mean call times are recorded.  The library calls end in
a stream synchronise and the copy of the answers, so they are timed by the host clock around the call; the torch arm by device
events around its kernels and a synchronise.  Before any timing the int8 and the f32 index must agree on ids and distance bits
under Dot (dim <= 1024: every sum is below 2^24).

Per int8 call, from the shapes: the bytes (rows x ld once, the partial lists written and read), the integer MACs, and the larger
of bytes / HBM peak and MACs / int8 peak.  --kernel-stats names the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of
`--only-int8` (a run of its own: tracing slows the host): the score kernel's mean time and its share of that bound are added.
Writes one JSON object to --out and prints it."""
import argparse
import csv
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12                                 # MI355X: 8 TB/s
INT8_MACS_PER_S = 2.5e15                                 # MI355X: about 5 POP/s dense int8 (public product figure), 2 ops per MAC


def load_package():
    pkg = os.path.join(ROOT, "vectordb-from-scratch_amd")
    spec = importlib.util.spec_from_file_location("vectordb_from_scratch_amd", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vectordb_from_scratch_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "rounds": len(ms)}


def int8_normal(rng, n, dim):
    """roughly normal values scaled into +-127"""
    return np.clip(np.rint(rng.standard_normal((n, dim), dtype=np.float32) * 42.0), -127, 127).astype(np.int8)


def roofline(st, nq, k, qt):
    """what one int8 call needs, from its shapes (st: GpuInt8Index.stats after the call)"""
    rows, ld, segs = st["rows"], st["ld"], st["segments"]
    tiles = -(-nq // qt)
    part = 2 * 8 * st["merge_keys"]                      # every key written once by the score kernel, read once by the merge
    macs = rows * ld * tiles * qt
    t_bytes, t_macs = (rows * ld + part) / HBM_BYTES_PER_S, macs / INT8_MACS_PER_S
    return {"row_bytes": rows * ld, "partial_list_bytes": part, "row_bytes_if_every_query_tile_missed_cache": rows * ld * tiles,
            "int8_macs": macs, "bytes_bound_ms": t_bytes * 1e3, "macs_bound_ms": t_macs * 1e3, "bound_ms": max(t_bytes, t_macs) * 1e3,
            "binds": "HBM bytes" if t_bytes >= t_macs else "int8 MACs", "workgroups": st["workgroups"], "segments": segs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--only-int8", action="store_true", help="the int8 arm alone, Dot, k = 10: the run to trace")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --only-int8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_bench.json"))
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    dev = torch.device("cuda:0")
    M = vdb.DistanceMetric
    rng = np.random.default_rng(0)
    queries = int8_normal(rng, a.queries, a.dim)
    q32 = queries.astype(np.float32)
    configs = [(M.DotProduct, 10)] if a.only_int8 else [(M.DotProduct, 10), (M.Euclidean, 10), (M.Cosine, 10), (M.DotProduct, 100)]
    metrics = list(dict.fromkeys(m for m, _ in configs))
    i8 = {m: vdb.GpuInt8Index(m) for m in metrics}
    f32 = {} if a.only_int8 else {m: vdb.GpuFlatIndex(m, device=0, keep_host_copy=False) for m in metrics}
    x32 = None if a.only_int8 else torch.empty((a.rows, a.dim), dtype=torch.float32, device=dev)
    t0 = time.perf_counter()
    for lo in range(0, a.rows, 100_000):                 # in blocks: the host never holds the widened store
        block = int8_normal(rng, min(100_000, a.rows - lo), a.dim)
        ids = np.arange(lo, lo + block.shape[0], dtype=np.uint64)
        for ix in i8.values():
            ix.add_bulk(ids, block)
        wide = block.astype(np.float32)
        for ix in f32.values():
            ix.add_bulk(wide, ids=ids)
        if x32 is not None:
            x32[lo:lo + block.shape[0]] = torch.from_numpy(wide)
    for ix in i8.values():
        ix.flush()
    for ix in f32.values():
        ix.set_split(2)                                  # the rows split into bf16 and low halves before the next screened search
        ix.flush()
    print(f"data and stores: {time.perf_counter() - t0:.1f} s", flush=True)
    rec = {"shape": {"rows": a.rows, "dim": a.dim, "queries": a.queries, "rounds": a.rounds, "calls_per_round": a.calls},
           "clock": "host clock around calls that end in a stream synchronise (arms 1, 2); device events and a synchronise (arm 3)",
           "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "int8_macs_per_s": INT8_MACS_PER_S}, "runs": []}
    if not a.only_int8:
        # torch._int_mm on this stack: said, not relied on
        try:
            qi = torch.from_numpy(queries[:32]).to(dev)
            xi = torch.from_numpy(int8_normal(rng, 1024, a.dim)).to(dev)
            r = torch._int_mm(qi, xi.t().contiguous())
            rec["torch_int_mm"] = "runs" if torch.equal(r.cpu(), (qi.cpu().int() @ xi.cpu().int().t())) else "runs, wrong result"
        except Exception as e:                           # noqa: BLE001 -- whatever this build refuses with
            rec["torch_int_mm"] = "refused: " + repr(e)[:160]
        x_n2 = (x32 * x32).sum(dim=1)
        q_dev = torch.from_numpy(q32).to(dev)

    def arm1(m, k):
        t = time.perf_counter()
        r = i8[m].search_batch_arrays(queries, k)
        return (time.perf_counter() - t) * 1e3, r

    def arm2(m, k):
        t = time.perf_counter()
        r = f32[m].search_batch_arrays(q32, k)
        return (time.perf_counter() - t) * 1e3, r

    def arm3(m, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s = q_dev @ x32.t()                              # [queries, rows]
        if m == M.Euclidean:
            s = x_n2[None, :] - 2.0 * s
        elif m == M.Cosine:
            s = -s / x_n2.sqrt()[None, :]
        else:
            s = -s
        top = torch.topk(s, k, dim=1, largest=False)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (top.indices,)

    arms = {"int8_index": arm1} if a.only_int8 else {"int8_index": arm1, "f32_index_split": arm2, "torch_f32_matmul_topk": arm3}
    for m, k in configs:
        last = {}
        for _ in range(3):                               # warm-up; the f32 index converts to the split layout in its first search
            for name, arm in arms.items():
                last[name] = arm(m, k)[1]
        run = {"metric": m.name, "k": k}
        if not a.only_int8:
            same = np.array_equal(last["int8_index"][0], last["f32_index_split"][0])
            run["int8_and_f32_index_agree_on_ids"] = bool(same)
            run["f32_index_layout"] = f32[m].layout()
            run["torch_shares_ids_of_k"] = float(np.mean([np.isin(last["torch_f32_matmul_topk"][0][b].cpu().numpy(), last["int8_index"][0][b]).sum()
                                                          for b in range(a.queries)]))
            if m == M.DotProduct:
                assert same and np.array_equal(last["int8_index"][1].view(np.uint32), last["f32_index_split"][1].view(np.uint32)), \
                    "the int8 and the f32 index disagree under Dot"
        t = {name: [] for name in arms}
        for _ in range(a.rounds):
            mine = {name: [] for name in arms}
            for _ in range(a.calls):
                for name, arm in arms.items():
                    mine[name].append(arm(m, k)[0])
            for name in arms:
                t[name].append(float(np.mean(mine[name])))
        run["times"] = {name: spread(v) for name, v in t.items()}
        st = i8[m].stats()
        run["int8_call_from_shapes"] = roofline(st, a.queries, k, st["query_tile"])
        if not a.only_int8:
            t1, t2 = run["times"]["int8_index"], run["times"]["f32_index_split"]
            run["int8_faster_than_f32_by_more_than_its_spread"] = bool(t2["median_ms"] - t1["median_ms"] > t2["max_ms"] - t2["min_ms"])
        rec["runs"].append(run)
        print(json.dumps(run), flush=True)
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "i8_score_kernel" in row["Name"]:
                    ms = float(row["AverageNs"]) * 1e-6
                    bound = rec["runs"][0]["int8_call_from_shapes"]["bound_ms"]
                    rec["score_kernel_traced"] = {"name": row["Name"][:80], "calls": int(row["Calls"]), "mean_ms": ms, "bound_ms": bound,
                                                  "share_of_bound": bound / ms, "of": "Dot, k = 10; a separate rocprofv3 --kernel-trace --stats run"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
