#!/usr/bin/env python3
"""Binary flat search (GpuBinaryIndex) under Hamming at a 1-bit-embedding shape against the two ways a caller has without it:
GpuInt8Index under Euclidean over the same bits widened to 0/1 int8 (its distance is sqrtf((float)h): ids and order must equal
the binary index's exactly, and are checked before any timing), and a torch f32 matmul over the widened bits plus topk on the same
GPU (every sum is an integer below 2^24, exact in f32: its k smallest distances must equal the binary index's, checked before any
timing too; its order among equal distances is torch's own and is not compared).  The three arms run in one process,
alternating; every arm is warmed up; each of --rounds rounds times --calls calls per arm, and the median, minimum and maximum of the rounds' mean call times are recorded.  The library calls end in a stream synchronise
and the copy of the answers, so they are timed by the host clock around the call; the torch arm by device events around its
kernels and a synchronise.

Per binary call, from the shapes: the bytes (rows x ld once, the widened queries, the partial lists written and read), the
integer MACs, and the larger of bytes / HBM peak and MACs / int8 peak.  --kernel-stats names the kernel statistics of a
`rocprofv3 --kernel-trace --stats` run of `--only-binary` (a run of its own: tracing slows the host): the score kernel's mean time
and its share of that bound are added.  Writes one JSON object to --out and prints it."""
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


def roofline(st, nq, qt):
    """what one binary call needs, from its shapes (st: GpuBinaryIndex.stats after the call)"""
    rows, ld = st["rows"], st["ld"]
    tiles = -(-nq // qt)
    part = 2 * 8 * st["merge_keys"]                      # every key written once by the score kernel, read once by the merge
    wide = 2 * nq * ld * 8                               # the widened queries: written once, staged once per segment from L2
    macs = rows * ld * 8 * tiles * qt
    t_bytes, t_macs = (rows * ld + part + wide) / HBM_BYTES_PER_S, macs / INT8_MACS_PER_S
    return {"row_bytes": rows * ld, "partial_list_bytes": part, "widened_query_bytes": wide, "int8_macs": macs,
            "bytes_bound_ms": t_bytes * 1e3, "macs_bound_ms": t_macs * 1e3, "bound_ms": max(t_bytes, t_macs) * 1e3,
            "binds": "HBM bytes" if t_bytes >= t_macs else "int8 MACs", "workgroups": st["workgroups"], "segments": st["segments"],
            "merge_keys_this_call": st["merge_keys"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024, help="bits")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--only-binary", action="store_true", help="the binary arm alone, 256 queries, k = 10: the run to trace")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --only-binary")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_bench.json"))
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    all_queries = rng.integers(0, 256, size=(256, a.dim // 8), dtype=np.uint8)
    configs = [(256, 10)] if a.only_binary else [(256, 10), (256, 100), (1, 10), (1, 100)]
    binary = vdb.GpuBinaryIndex(vdb.BinaryMetric.Hamming)
    i8 = None if a.only_binary else vdb.GpuInt8Index(vdb.DistanceMetric.Euclidean)
    x32 = None if a.only_binary else torch.empty((a.rows, a.dim), dtype=torch.float32, device=dev)
    t0 = time.perf_counter()
    for lo in range(0, a.rows, 100_000):                 # in blocks: the host never holds the widened store
        block = rng.integers(0, 256, size=(min(100_000, a.rows - lo), a.dim // 8), dtype=np.uint8)
        ids = np.arange(lo, lo + block.shape[0], dtype=np.uint64)
        binary.add_bulk(ids, block)
        if i8 is not None:
            wide = np.unpackbits(block, axis=1).astype(np.int8)
            i8.add_bulk(ids, wide)
            x32[lo:lo + block.shape[0]] = torch.from_numpy(wide).to(dev).float()
    binary.flush()
    if i8 is not None:
        i8.flush()
        x_n = x32.sum(dim=1)                             # popcounts: h = nq + nx - 2 a, nq the same for every row
    print(f"data and stores: {time.perf_counter() - t0:.1f} s", flush=True)
    rec = {"shape": {"rows": a.rows, "bits": a.dim, "metric": "Hamming", "rounds": a.rounds, "calls_per_round": a.calls},
           "clock": "host clock around calls that end in a stream synchronise (arms 1, 2); device events and a synchronise (arm 3)",
           "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "int8_macs_per_s": INT8_MACS_PER_S}, "runs": []}
    for nq, k in configs:
        queries = all_queries[:nq]
        q8 = np.unpackbits(queries, axis=1).astype(np.int8)
        q_dev = None if a.only_binary else torch.from_numpy(q8).to(dev).float()

        def arm1():
            t = time.perf_counter()
            r = binary.search_batch_arrays(queries, k)
            return (time.perf_counter() - t) * 1e3, r

        def arm2():
            t = time.perf_counter()
            r = i8.search_batch_arrays(q8, k)
            return (time.perf_counter() - t) * 1e3, r

        def arm3():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            top = torch.topk(x_n[None, :] - 2.0 * (q_dev @ x32.t()), k, dim=1, largest=False)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), (top.indices, top.values)

        arms = {"binary_index": arm1} if a.only_binary else {"binary_index": arm1, "int8_index_widened": arm2, "torch_f32_matmul_topk": arm3}
        last = {}
        for _ in range(3):                               # warm-up
            for name, arm in arms.items():
                last[name] = arm()[1]
        run = {"queries": nq, "k": k}
        if not a.only_binary:
            b, w = last["binary_index"], last["int8_index_widened"]
            assert np.array_equal(b[0], w[0]) and np.array_equal(np.sqrt(b[1]).view(np.uint32), w[1].view(np.uint32)) and \
                b[2].tolist() == w[2].tolist(), "the binary and the int8 index disagree"
            run["binary_and_int8_index_agree_on_ids_order_and_distances"] = True
            nq_bits = torch.from_numpy(q8.sum(axis=1, dtype=np.int64).astype(np.float32)).to(dev)
            t_d = torch.sort(last["torch_f32_matmul_topk"][1] + nq_bits[:, None], dim=1).values.cpu().numpy()
            assert np.array_equal(t_d, b[1]), "torch's k smallest Hamming distances differ from the binary index's"
            run["torch_k_smallest_distances_equal_the_binary_index"] = True
        t = {name: [] for name in arms}
        for _ in range(a.rounds):
            mine = {name: [] for name in arms}
            for _ in range(a.calls):
                for name, arm in arms.items():
                    mine[name].append(arm()[0])
            for name in arms:
                t[name].append(float(np.mean(mine[name])))
        run["times"] = {name: spread(v) for name, v in t.items()}
        st = binary.stats()
        run["binary_call_from_shapes"] = roofline(st, nq, st["query_tile"])
        if not a.only_binary:
            t1, t2 = run["times"]["binary_index"], run["times"]["int8_index_widened"]
            run["binary_faster_than_int8_by_more_than_its_spread"] = bool(t2["median_ms"] - t1["median_ms"] > t2["max_ms"] - t2["min_ms"])
        rec["runs"].append(run)
        print(json.dumps(run), flush=True)
    if not a.only_binary:
        by = {(r["queries"], r["k"]): r["times"] for r in rec["runs"]}
        rec["k100_over_k10"] = {f"{nq}_queries": {arm: by[(nq, 100)][arm]["median_ms"] / by[(nq, 10)][arm]["median_ms"] for arm in by[(nq, 10)]}
                                for nq in (256, 1)}
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "bin_score_kernel" in row["Name"]:
                    ms = float(row["AverageNs"]) * 1e-6
                    bound = rec["runs"][0]["binary_call_from_shapes"]["bound_ms"]
                    rec["score_kernel_traced"] = {"name": row["Name"][:80], "calls": int(row["Calls"]), "mean_ms": ms, "bound_ms": bound,
                                                  "share_of_bound": bound / ms, "of": "256 queries, k = 10; a separate rocprofv3 --kernel-trace --stats run"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
