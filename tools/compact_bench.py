#!/usr/bin/env python3
"""vdb_flat_compact at 1M x 768 Cosine, B = 256, k = 10 (one process, one GPU, one JSON line).  For dead fractions of 5 %,
25 % and 50 % (uniformly scattered removes) and 50 % as one contiguous block:

    step_ms_before   a search batch on the index with its dead rows          } alternated, medians
    step_ms_fresh    the same batch on a NEW index bulk-loaded with the survivors in the same order
    compact_ms       the vdb_flat_compact call on the host clock (device moves + renumbering the host's id -> row map)
    compact_device_ms  its device part alone (store_stats()[7]: first enqueue .. synchronise after the last move)
    d2d_copy_ms      ONE hipMemcpyAsync device-to-device of n_live * ld * 4 bytes in this process (the yardstick)
    step_ms_after    the batch on the compacted index                         } alternated with step_ms_fresh again
    bytes_moved, chunks, store_stats before / after

Every case is rebuilt --reps times (a compaction can only be timed once per index); the figures are medians over the reps.

    python tools/compact_bench.py [--rows N] [--reps R] [--steps S]"""
import argparse
import ctypes
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9)
    a = ap.parse_args()
    vdb = load_package()
    vdb.build()
    dev = torch.device("cuda", 0)
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))   # the runtime torch and the library share
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    g = torch.Generator(device=dev).manual_seed(11)
    n, d, B, k = a.rows, a.dim, a.batch, a.k
    ld = (d + 31) // 32 * 32
    rows = torch.randn((n, d), device=dev, generator=g, dtype=torch.float32)
    q = torch.randn((B, d), device=dev, generator=g, dtype=torch.float32)
    scratch = torch.empty((n, ld), device=dev, dtype=torch.float32)          # target of the yardstick copy
    oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    od = torch.empty((B, k), dtype=torch.float32, device=dev)
    oc = torch.empty((B,), dtype=torch.int32, device=dev)

    def step(ix):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.search_batch_device(q.data_ptr(), B, d, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(x, y):
        for ix in (x, y, x, y):                                              # warm-up of both arms
            step(ix)
        tx, ty = [], []
        for _ in range(a.steps):
            tx.append(step(x))
            ty.append(step(y))
        return med(tx), med(ty)

    def d2d(nbytes):
        ts = []
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = hip.hipMemcpyAsync(scratch.data_ptr(), rows.data_ptr(), nbytes, 3, None)     # 3 = hipMemcpyDeviceToDevice
            assert rc == 0, rc
            torch.cuda.synchronize()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return med(ts)

    rng = np.random.default_rng(5)
    cases = [("scattered", 0.05), ("scattered", 0.25), ("scattered", 0.50), ("block", 0.50)]
    out = {"rows": n, "dim": d, "batch": B, "k": k, "metric": "cosine", "reps": a.reps, "steps": a.steps, "cases": []}
    for kind, frac in cases:
        n_dead = int(n * frac)
        acc = {}
        for rep in range(a.reps):
            dead = rng.permutation(n)[:n_dead] if kind == "scattered" else np.arange(n // 4 + 13, n // 4 + 13 + n_dead)
            alive = np.ones(n, dtype=bool)
            alive[dead] = False
            ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
            ix.add_bulk_device(rows.data_ptr(), n, d)
            for i in dead.tolist():
                ix.remove(i)
            keep = torch.from_numpy(np.nonzero(alive)[0]).to(dev)
            surv = rows.index_select(0, keep).contiguous()
            fresh = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
            fresh.add_bulk_device(surv.data_ptr(), n - n_dead, d, ids=np.nonzero(alive)[0].astype(np.uint64))
            r = {}
            r["step_ms_before"], f1 = alternate(ix, fresh)
            r["store_stats_before"] = ix.store_stats()
            ref = (oi.clone(), od.clone(), oc.clone())                        # the fresh index's answer
            r["d2d_copy_ms"] = d2d((n - n_dead) * ld * 4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ix.compact()
            r["compact_ms"] = (time.perf_counter() - t0) * 1e3
            assert got == n_dead
            st = ix.store_stats()
            r["store_stats_after"] = st
            r["compact_device_ms"] = st[7] / 1e6
            r["chunks_direct"], r["chunks_bounce"] = st[8], st[9]
            r["step_ms_after"], f2 = alternate(ix, fresh)
            r["step_ms_fresh"] = (f1 + f2) / 2
            step(ix)
            assert torch.equal(oi, ref[0]) and torch.equal(od, ref[1]) and torch.equal(oc, ref[2]), "compacted index != fresh index"
            for key, v in r.items():
                acc.setdefault(key, []).append(v)
            del ix, fresh, surv, keep
        c = {"kind": kind, "dead_fraction": frac, "n_live": n - n_dead, "bytes_moved_min": (n - n_dead) * ld * 4}
        for key, v in acc.items():
            c[key] = v[-1] if isinstance(v[0], list) else (v[0] if key.startswith("chunks") else round(med(v), 3))
        c["compact_device_over_d2d"] = round(c["compact_device_ms"] / c["d2d_copy_ms"], 2)
        c["compact_over_d2d"] = round(c["compact_ms"] / c["d2d_copy_ms"], 2)
        c["after_over_fresh"] = round(c["step_ms_after"] / c["step_ms_fresh"], 3)
        c["before_over_after"] = round(c["step_ms_before"] / c["step_ms_after"], 3)
        out["cases"].append(c)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
