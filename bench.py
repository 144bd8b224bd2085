#!/usr/bin/env python3
"""bench.py -- headline benchmark of the FlatIndex hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c1|c2|c3|c4] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` with N > 1 and no torchrun environment (WORLD_SIZE unset) starts the N ranks ITSELF: before anything touches
the GPU the process launches `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child, relays rank 0's
JSON line and exits with the child's code.  (`--dry-launch`: every rank prints its rank / world / local rank and exits
without touching a GPU -- how the CPU test checks the launch.)

Workloads (BASELINE.json `configs`); synthetic uniform[0,1) data like the reference's benches
(benches/search_bench.rs:6-13), seeded.  One "step" = one batched search with queries and outputs resident in HBM.

  c1  FlatIndex 10k x 128 f32, Euclidean, ONE query [0.5; 128], k = 10 -- benches/search_bench.rs:18-33, the literal
      FlatIndex::search drop-in: microseconds per vdb_flat_search call (host pointers) and per device-resident call, the
      oracle's single-core time beside them.
  c2 (default, the configuration BASELINE.json's metric is quoted on)
      FlatIndex 1M x 768 f32, cosine, batch = 256, k = 10.  --gpus N shards the SAME 1M rows ("scaling": "strong").
  c3  FlatIndex 10M x 768 f32, dot, batch = 1024, k = 100, row-sharded over 8 GPUs: every rank builds ITS 1.25M-row shard
      on the device (per-GPU work fixed, "scaling": "weak"; --gpus 8 is the 10M-row job of BASELINE configs[2]).
  c4  FlatIndex 1M x 1536 f32, Euclidean, batch = 256, k = 10, metadata eq-filter (25 % of the rows) compiled by
      VectorStore.compile_filter from string metadata into the device bitmask applied before top-k.

With N > 1 the exchange (RCCL all-gather of the partial top-k + merge) runs behind the C ABI (include/vdb_shard.h);
torch.distributed only launches the ranks, broadcasts the RCCL unique id and takes the MAX of the timings.
"single_process_sharded" is the other form of the same index: ONE vdb_flat_index over all N GPUs inside rank 0's process
(vdb_flat_create_sharded -- the object the reference's single server process would hold), timed while the other ranks idle.

A plain run sets up, warms up, times the K steps and prints the headline (`value`, `ms_per_step`, `dtype`, `path_stats`);
every side measurement below is null unless `--full` is given.  `--dump-outputs DIR` writes the arrays the last timed step
returned (ids, distances, counts) as DIR/<name>.npy.

Prints ONE JSON line on rank 0 (the driver contract); with --full it also carries
  "roofline"        the dominant kernel, HIP-event timed on its launch stream, on BOTH axes of SURVEY 8(d) with the
                    binding one named; "traffic" = PMC HBM bytes per launch of the profiled run the line cites;
  "f32_exact_tier"  the same index and queries through the f32-input MFMA tier only (the contract's f32 axis), results
                    compared bit for bit with the default path;
  "shadow_rows"     the same index with the opt-in bf16 shadow of the rows (+50 % memory, half the streamed bytes), same results;
  "gauss_dataset"   the same size on unit-normalised Gaussian rows (the harder distribution of SURVEY 8(d));
  "cpu_baseline"    the CPU oracle = port of the reference algorithm, 1 core, bounded query sample.
"""
import argparse
import importlib.util
import json
import os
import socket
import subprocess
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))

CONFIGS = {
    "c1": dict(rows=10_000, dim=128, batch=1, k=10, metric=0, scaling="strong",
               workload="FlatIndex 10k x 128 f32, k=10, Euclidean, single query [0.5; 128] (BASELINE configs[0], benches/search_bench.rs:18-33)"),
    "c2": dict(rows=1_000_000, dim=768, batch=256, k=10, metric=1, scaling="strong",
               workload="FlatIndex 1M x 768 f32, cosine, batch=256 queries, k=10 (BASELINE configs[1])"),
    "c3": dict(rows_per_rank=1_250_000, dim=768, batch=1024, k=100, metric=2, scaling="weak",
               workload="FlatIndex 10M x 768 f32, dot product, batch=1024, k=100, row-sharded 1.25M rows per GPU (BASELINE configs[2]; "
                        "the 10M-row job is --gpus 8)"),
    "c4": dict(rows=1_000_000, dim=1536, batch=256, k=10, metric=0, scaling="strong",
               workload="FlatIndex 1M x 1536 f32, Euclidean, batch=256, k=10, metadata eq filter as a device bitmask before top-k "
                        "(BASELINE configs[3])"),
}
SETTLE_STEPS = 200              # headline steps back to back in front of the W warm-up steps: the device needs 15-20 ms of work
                                # to raise its clocks; 200 C2 steps are ~125 ms, about what the side legs of --full
                                # put in front of the headline
CHUNK = 125_000                 # generation granule: data is identical for every --gpus value
PEAK_F32_MFMA_TFLOPS = 157.3    # /opt/skills/guides/MI355X_MICROARCH.md, dense f32-input MFMA
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA (not the 2:1-sparsity headline)
PEAK_HBM_GBS = 8000.0
PALETTE = ["red", "green", "blue", "amber"]


def load_package():
    name = "vectordb_from_scratch_amd"
    if name in sys.modules:
        return sys.modules[name]
    pkg = os.path.join(ROOT, "vectordb-from-scratch_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


DATA = "uniform"                # "uniform": [0,1) like the reference's benches; "gauss": unit-normalised Gaussian rows


def gen_chunk(c, n, dim, device, data=None):
    g = torch.Generator(device=device)
    g.manual_seed(1000 + c)                      # db seed family (db seed 1, query seed 2)
    if (data or DATA) == "gauss":
        x = torch.randn((n, dim), generator=g, device=device, dtype=torch.float32)
        return x / x.norm(dim=1, keepdim=True)
    return torch.rand((n, dim), generator=g, device=device, dtype=torch.float32)


def gen_queries(nq, dim, device, data=None):
    g = torch.Generator(device=device)
    g.manual_seed(2)
    if (data or DATA) == "gauss":
        return torch.randn((nq, dim), generator=g, device=device, dtype=torch.float32)
    return torch.rand((nq, dim), generator=g, device=device, dtype=torch.float32)


def build_index(vdb, metric, lo, hi, n_rows, dim, device, local_rank, data=None):
    """Rows lo..hi of the global, chunk-seeded matrix, generated on the device and handed over in HBM."""
    index = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), device=local_rank, keep_host_copy=False)
    index.reserve(hi - lo, dim)
    chunk = min(CHUNK, n_rows)
    for c in range(lo // chunk, (hi + chunk - 1) // chunk):
        c0, c1 = c * chunk, min((c + 1) * chunk, n_rows)
        block = gen_chunk(c, c1 - c0, dim, device, data)
        a, b = max(lo, c0), min(hi, c1)
        part = block[a - c0:b - c0].contiguous()
        torch.cuda.synchronize()
        index.add_bulk_device(part.data_ptr(), b - a, dim, first_id=a)
        del block, part
    index.flush()
    return index


def host_rows(n_rows, dim, device, data=None):
    chunk = min(CHUNK, n_rows)
    out = np.empty((n_rows, dim), dtype=np.float32)
    for c in range((n_rows + chunk - 1) // chunk):
        c0, c1 = c * chunk, min((c + 1) * chunk, n_rows)
        out[c0:c1] = gen_chunk(c, c1 - c0, dim, device, data).cpu().numpy()
    return out


def dump_outputs(out_dir, ids, dists, counts):
    """The arrays the caller of the timed path receives, as float64 (ids, counts: exact) and float32 (distances)."""
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "ids.npy"), np.asarray(ids).astype(np.float64))
    np.save(os.path.join(out_dir, "distances.npy"), np.asarray(dists, dtype=np.float32))
    np.save(os.path.join(out_dir, "counts.npy"), np.asarray(counts).astype(np.float64))


def free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` outside torchrun: start the N ranks as a child job.  Nothing in this process has touched
    the GPU yet (importing torch does not), and it never does: it only relays the child's output and exit code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.run(cmd, env=env).returncode


def newest_pmc_tag():
    """Tag (e.g. 'r03_b') of the newest profiles/r*_pmc_fused.json: the only PMC pass bench.py may quote traffic from."""
    import glob
    import re
    tags = []
    for f in glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_fused.json")):
        m = re.match(r"(r\d+_[a-z]+)_pmc_fused\.json$", os.path.basename(f))
        if m:
            tags.append(m.group(1))
    return max(tags) if tags else None


def run_c1(args, vdb, device):
    """BASELINE configs[0] at its own shape (benches/search_bench.rs:18-33): 10,000 x 128 uniform[0,1) rows, Euclidean, k = 10,
    ONE query [0.5; 128].  This is Index::search itself -- one vdb_flat_search call per query -- so what is reported is the
    latency of a call, host pointers in and out (the literal drop-in) and device-resident, with the oracle's time beside it."""
    import ctypes
    cfg = CONFIGS["c1"]
    n, dim, k = args.rows or cfg["rows"], args.dim or cfg["dim"], args.k or cfg["k"]
    rows = np.random.default_rng(0).random((n, dim), dtype=np.float32)          # search_bench.rs:6-13, seeded
    q = np.full((dim,), 0.5, dtype=np.float32)                                 # search_bench.rs:27
    index = vdb.GpuFlatIndex(vdb.DistanceMetric(cfg["metric"]), device=device.index or 0, keep_host_copy=False)
    index.add_bulk(rows)
    index.flush()
    L, h = vdb._ffi.lib(), index._h
    fp = ctypes.POINTER(ctypes.c_float)
    out_i = np.zeros(k, dtype=np.uint64)
    out_d = np.zeros(k, dtype=np.float32)
    out_c = ctypes.c_size_t()

    def host_call():
        rc = L.vdb_flat_search(h, q.ctypes.data_as(fp), dim, k, out_i.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                               out_d.ctypes.data_as(fp), ctypes.byref(out_c))
        assert rc == 0, vdb._ffi.last_error()

    q_t = torch.from_numpy(q[None, :]).to(device)
    d_i = torch.empty((1, k), dtype=torch.int64, device=device)
    d_d = torch.empty((1, k), dtype=torch.float32, device=device)
    d_c = torch.empty((1,), dtype=torch.int32, device=device)
    torch.cuda.synchronize()

    def dev_call():
        index.search_batch_device(q_t.data_ptr(), 1, dim, k, d_i.data_ptr(), d_d.data_ptr(), d_c.data_ptr())

    def lat(fn, w, kk):
        for _ in range(w):
            fn()
        torch.cuda.synchronize()
        ts = []
        t_all = time.perf_counter()
        for _ in range(kk):
            t1 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t1)
        t_all = time.perf_counter() - t_all
        ts.sort()
        return t_all / kk, ts[len(ts) // 2], ts[int(len(ts) * 0.99)]

    steps, warm = max(args.steps, 1), max(args.warmup, 1)
    h_mean, h_med, h_p99 = lat(host_call, warm, steps)
    stats = index.last_stats()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out_i[None, :], out_d[None, :], np.array([out_c.value]))
    dev_lat, roofline, cpu, recall = None, None, None, None
    if args.full:
        d_mean, d_med, d_p99 = lat(dev_call, warm, steps)
        import oracle
        oracle.lib()
        t1 = time.perf_counter()
        n_cpu = 0
        while n_cpu < 20 or time.perf_counter() - t1 < min(args.cpu_seconds, 3.0):
            oi, od = oracle.flat_search(cfg["metric"], rows, q, k)
            n_cpu += 1
        t_cpu = (time.perf_counter() - t1) / n_cpu
        exact = bool(int(out_c.value) == len(oi) and np.array_equal(oi, out_i[:len(oi)]) and np.array_equal(od.view(np.uint32), out_d[:len(od)].view(np.uint32)))
        exact_dev = bool(np.array_equal(d_i.cpu().numpy()[0].astype(np.uint64), oi) and np.array_equal(d_d.cpu().numpy()[0].view(np.uint32), od.view(np.uint32)))
        alg_bytes = 4.0 * n * dim + 4.0 * dim
        dev_lat = {"mean": round(1e6 * d_mean, 2), "median": round(1e6 * d_med, 2), "p99": round(1e6 * d_p99, 2)}
        recall = float(oracle.recall(oi, out_i[:k]))
        roofline = {"bound": "hbm", "achieved": round(alg_bytes / d_mean / 1e9, 2), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(alg_bytes / d_mean / 1e9 / PEAK_HBM_GBS, 6), "traffic": None,
                    "note": "5.12 MB per query: the call is bound by launch and synchronisation latency (five short kernels and one "
                            "host sync), not by a roofline; the fraction is quoted on the device-resident call for completeness"}
        cpu = {"value": round(1.0 / t_cpu, 2), "unit": "queries/s", "cores": 1, "kind": "port",
               "us_per_search": round(1e6 * t_cpu, 1),
               "sample": f"{n_cpu} searches of the same query, {n_cpu * t_cpu:.2f} s; oracle/flat_oracle.c",
               "host_cpus": os.cpu_count(), "ids_and_distances_bit_identical": exact,
               "device_resident_call_bit_identical": exact_dev}
    line = {
        "metric": f"QPS of single-query FlatIndex::search, {n}x{dim} f32 euclidean k={k} (one vdb_flat_search call per query; latency in config.us_per_search)",
        "value": round(1.0 / h_mean, 1), "unit": "queries/s", "n_gpus": 1, "steps": steps, "warmup": warm,
        "ms_per_step": round(1e3 * h_mean, 5), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32 (f32-input MFMA scores of every row -- the dense path of indexes up to 16384 rows -- then the exact f32 re-rank)",
        "data": "synthetic",
        "config": {"workload": cfg["workload"], "name": "c1", "n_rows": n, "dim": dim, "batch": 1, "k": k, "distance": "euclidean",
                   "inputs": "value: host pointers in and out (vdb_flat_search, the literal Index::search drop-in); device_resident: queries and outputs in HBM",
                   "us_per_search": {"host_pointers": {"mean": round(1e6 * h_mean, 2), "median": round(1e6 * h_med, 2), "p99": round(1e6 * h_p99, 2)},
                                     "device_resident": dev_lat}},
        "recall_at_k": recall, "path_stats": stats, "roofline": roofline, "cpu_baseline": cpu,
    }
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS), help="BASELINE.json workload (default c2 = the configuration the metric is quoted on)")
    ap.add_argument("--rows", type=int, default=0, help="override the index size (parity/debug only)")
    ap.add_argument("--dim", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--metric", type=int, default=-1)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the cpu_baseline leg")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-f32-tier", action="store_true", help="skip the side measurement of the f32 MFMA tier")
    ap.add_argument("--no-gauss", action="store_true", help="skip the side measurement on unit-normalised Gaussian rows")
    ap.add_argument("--no-shadow", action="store_true", help="skip the side measurement with the opt-in bf16 shadow rows (vdb_flat_set_shadow)")
    ap.add_argument("--no-pipelined", action="store_true", help="skip the two-batches-in-flight side measurement (keeps a profile's per-kernel averages synchronous)")
    ap.add_argument("--no-single-process", action="store_true", help="skip the ONE-index-over-all-GPUs-in-one-process side measurement (vdb_flat_create_sharded)")
    ap.add_argument("--full", action="store_true",
                    help="also every side measurement (roofline and per-kernel times, f32 tier, pipelined, shadow rows, Gaussian rows, "
                         "PCIe, after-idle, single-process, repeat rounds, CPU baseline and oracle parity); the --no-* options still apply")
    ap.add_argument("--lean", action="store_true", help="with --full: the roofline only, every other side measurement off (profiling runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the ids, distances and counts the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--data", default="uniform", choices=["uniform", "gauss"], help="distribution of the HEADLINE index")
    ap.add_argument("--screen", type=int, default=1, help="1: bf16 screening tier first (default); 0: f32 MFMA tier only")
    ap.add_argument("--no-wide", action="store_true", help="batches above 256 queries: 256-query passes instead of the 512-query filter kernel (A/B)")
    ap.add_argument("--rehearse-distributed", action="store_true",
                    help="one rank, but through every step of the N > 1 code path (process group, C-ABI shard group of one rank, "
                         "group search, repeat rounds, gloo waits): what the driver's --gpus N run executes, rehearsed on one GPU")
    ap.add_argument("--rehearse-fallback", action="store_true", help="with the distributed path: behave as if the C-ABI shard group could not be created (the torch.distributed exchange)")
    ap.add_argument("--dry-launch", action="store_true", help="print this rank's RANK / WORLD_SIZE / LOCAL_RANK as a JSON line and exit (no GPU is touched)")
    args = ap.parse_args()
    if args.lean or not args.full:
        args.no_cpu = args.no_f32_tier = args.no_gauss = args.no_shadow = args.no_pipelined = args.no_single_process = True

    # ---- `--gpus N` outside torchrun: launch the N ranks (before any GPU call in this process)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    global DATA
    DATA = args.data
    cfg = dict(CONFIGS[args.config])
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_launch:
        print(json.dumps({"dry_launch": True, "rank": rank, "world": world, "local_rank": local_rank, "gpus": args.gpus,
                          "master": f'{os.environ.get("MASTER_ADDR", "")}:{os.environ.get("MASTER_PORT", "")}'}), flush=True)
        return
    if world != args.gpus and world > 1:
        args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the engine has no CPU path")
    if world > torch.cuda.device_count():
        raise SystemExit(f"bench.py --gpus {world}: only {torch.cuda.device_count()} GPU(s) visible; RCCL needs one device per rank")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    vdb = load_package()
    vdb.build()
    if args.config == "c1":
        if world > 1:
            raise SystemExit("config c1 is a single-query, single-GPU latency measurement")
        return run_c1(args, vdb, device)
    gloo = None
    distm = world > 1 or args.rehearse_distributed                # the distributed code path (N > 1, or its one-rank rehearsal)
    if distm:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            os.environ["MASTER_PORT"] = str(free_port())
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        gloo = dist.new_group(backend="gloo")                       # host-side waits that must not park a kernel on the GPUs

    from vectordb_from_scratch_amd.sharded import ShardGroup, gpu_local_search, group_search, shard_range

    dim = args.dim or cfg["dim"]
    B = args.batch or cfg["batch"]
    k = args.k or cfg["k"]
    metric = cfg["metric"] if args.metric < 0 else args.metric
    if "rows_per_rank" in cfg:                                      # weak scaling: every rank owns a full-size shard
        per = args.rows or cfg["rows_per_rank"]
        n_rows, lo, hi = per * world, per * rank, per * (rank + 1)
    else:
        n_rows = args.rows or cfg["rows"]
        lo, hi = shard_range(n_rows, rank, world)

    index = build_index(vdb, metric, lo, hi, n_rows, dim, device, local_rank)
    index.set_screen(args.screen)
    if args.no_wide:
        index.set_wide(False)
    queries = gen_queries(B, dim, device)

    # ---- c4: the metadata filter, compiled from string metadata to the device bitmask (timed: it is part of an honest C4)
    mask_t, mask_bits, filt = None, 0, None
    if args.config == "c4":
        t1 = time.perf_counter()
        colors = np.array(PALETTE, dtype=object)[np.arange(n_rows) % 4]
        store = vdb.VectorStore.with_index(index)
        store.attach_bulk_metadata(n_rows, {"color": colors})        # ids 0..n-1 <-> rows; the vectors are already in the index
        t2 = time.perf_counter()
        mask_np, mask_bits = store.compile_filter(vdb.MetadataFilter.Eq("color", PALETTE[0]))
        t3 = time.perf_counter()
        mask_t = torch.from_numpy(mask_np.view(np.int64)).to(device)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        filt = {"filter": f'eq color="{PALETTE[0]}" (string metadata, 4 values, 25 % selectivity)', "mask_bits": int(mask_bits),
                "rows_selected": int(np.unpackbits(mask_np.view(np.uint8)).sum()),
                "metadata_attach_ms": round(1e3 * (t2 - t1), 2), "compile_filter_ms": round(1e3 * (t3 - t2), 3),
                "mask_upload_ms": round(1e3 * (t4 - t3), 3)}

    # ---- the search path: N = 1 the plain device call; N > 1 the C-ABI shard group (RCCL), one process per GPU
    mptr = mask_t.data_ptr() if mask_t is not None else 0
    group, rccl_ranks, exchange_note = None, None, None
    if distm:
        # every rank must take the same path: agree on whether the C-ABI group came up everywhere
        try:
            if args.rehearse_fallback:
                raise RuntimeError("rehearsal: --rehearse-fallback")
            group = ShardGroup.from_torch_distributed(local_rank)
            ok, why = 1, ""
        except Exception as e:                                   # noqa: BLE001 -- reported, never swallowed
            group, ok, why = None, 0, f"{type(e).__name__}: {e}"
        flag = torch.tensor([ok], dtype=torch.int32, device=device)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
        if int(flag.item()) == 0:
            # the library's own RCCL group did not come up on every rank: the same exchange over torch.distributed (three
            # all-gathers + the HIP merge per batch instead of one collective), and the line says so
            from vectordb_from_scratch_amd.sharded import torch_group_search
            group = None
            exchange_note = ("torch.distributed all_gather_into_tensor x3 + vdb_merge_topk_device (fallback: the C-ABI shard group could "
                             f"not be created on every rank: {why or 'another rank failed'})")
            rccl_ranks = world
            search = torch_group_search(index, mask_ptr=mptr, mask_bits=mask_bits)
        else:
            rccl_ranks = group.world()
            search = group_search(group, index, mask_ptr=mptr, mask_bits=mask_bits)
    else:
        search = gpu_local_search(index, mask_ptr=mptr, mask_bits=mask_bits, reuse_outputs=True)

    def step(q=None):
        return search(queries if q is None else q, k)

    def barrier():
        if distm:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def timed(fn, n_warm, n_steps):
        for _ in range(n_warm):
            o = fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            o = fn()
        barrier()
        el = time.perf_counter() - t0
        if distm:
            t = torch.tensor([el], dtype=torch.float64, device=device)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            el = float(t.item())
        return el, o

    # ---- roofline of the dominant kernel, HIP events on its launch stream (vdb_flat_set_profile).
    def kernel_ms_of(ix, fn, n_iter, rows_local):
        # average duration of ONE launch of the dominant kernel (a batch above the kernel's query tile takes several
        # passes, and the counter sums their launches: stats["filter_launches"])
        for _ in range(25):                                     # the clock state of a timed region, not of the host work before this call
            fn()
        ix.set_profile(True)
        ns = []
        for _ in range(n_iter):
            fn()
            st_ = ix.last_stats()
            ns.append(st_["fused_kernel_ns"] / max(1, launches_of(st_, rows_local)))
        ix.set_profile(False)
        return float(np.mean(ns)) / 1e6

    def launches_of(st_, rows_local):
        return max(1, round(st_["rows_scanned"] / max(rows_local, 1)))

    local_rows = hi - lo
    # ---- the f32-exact tier FIRST: the same index and queries with every score on the f32-input MFMA (SURVEY 8(d)'s f32
    # axis).  It is measured before the headline so that the GPU clock has ramped when the W + K steps of the headline run
    # (a driver run with 20 steps after 5 is otherwise a cold-clock run: 0.75 instead of 0.69 ms per step).
    f32_raw = None
    if args.screen and not args.no_f32_tier:
        index.set_screen(0)
        n_f32 = max(3, min(args.steps, 10))
        k32 = kernel_ms_of(index, step, 3, local_rows)          # (the event-synchronised launches first: the leg ends on its
        el32, o32 = timed(step, 2, n_f32)                       # continuous part, ~40 ms of dense GPU work right before the headline)
        o32 = tuple(t.clone() for t in o32)
        f32_raw = (el32, n_f32, o32, k32)
        index.set_screen(1)

    # ---- two batches in flight (vdb_flat_search_batch_device_submit / _wait): what a server that keeps the GPU busy
    # sees.  Measured BEFORE the headline (its ~140 batches also hand the headline's W + K steps a GPU in a settled clock state:
    # the first 20-step round after a change of workload runs 3-10 % slow whatever the code path).
    # Every batch completes inside its timed region.  The synchronous loop is RE-measured in the same leg,
    # interleaved (pipelined, synchronous, pipelined, synchronous; each round K steps after 3 of its own kind): at the
    # driver's 20-step length a single round of either kind moves by several per cent with the clock state the previous
    # leg left behind, and only rounds taken side by side say which form is faster.
    pipelined = None
    if not distm and not args.no_pipelined:
        bufs = [(torch.empty((B, k), dtype=torch.int64, device=device), torch.empty((B, k), dtype=torch.float32, device=device),
                 torch.empty((B,), dtype=torch.int32, device=device)) for _ in range(2)]

        def submit(i):
            o = bufs[i & 1]
            return index.search_batch_device_submit(queries.data_ptr(), B, dim, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                    mask_ptr=mptr, mask_bits=mask_bits)

        def run_pipelined(n):
            t = submit(0)
            for i in range(1, n):
                t2 = submit(i)
                index.search_batch_device_wait(t)
                t = t2
            index.search_batch_device_wait(t)

        def run_sync(n):
            for _ in range(n):
                step()

        def one_round(fn):
            fn(3)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fn(args.steps)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t1) / args.steps

        run_pipelined(max(args.warmup, 4))                            # both workspaces and streams have run before anything is timed
        rp, rs = [], []
        for _ in range(3):
            rp.append(one_round(run_pipelined))
            rs.append(one_round(run_sync))
        # (nothing between the last synchronous round and the headline's W + K steps: tools/clock_series.py shows that 5 ms of an
        # idle GPU in front of a 5 + 20-step measurement already cost 7 %, 20 ms cost 12 % -- the leg's summary is built afterwards)
    repeat_rounds = None
    if distm and args.full and not args.lean:
        # N > 1 has no two-in-flight form: three rounds of the same synchronous group search, reported, in front of the headline
        repeat_rounds = [round(1e3 * timed(step, 3, args.steps)[0] / max(args.steps, 1), 4) for _ in range(3)]

    for _ in range(SETTLE_STEPS):                 # the clock state of a busy GPU, also when no side leg ran in front
        step()
    elapsed, out = timed(step, args.warmup, args.steps)
    ms_per_step = 1e3 * elapsed / max(args.steps, 1)
    qps = B * args.steps / elapsed
    stats = index.last_stats()
    out = tuple(t.clone() for t in out)          # the search reuses its output tensors; keep this step's results
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, *(t.cpu().numpy() for t in out))
    if not distm and not args.no_pipelined:
        pipe_last = bufs[(args.steps - 1) & 1]                      # the last pipelined batch's outputs (untouched since)
        mp_, ms_ = float(np.median(rp)), float(np.median(rs))
        pipelined = {"value": round(B / (mp_ * 1e-3), 2), "unit": "queries/s", "ms_per_step": round(mp_, 4), "in_flight": 2,
                     "results_identical_to_synchronous_path": bool(torch.equal(pipe_last[0], out[0]) and
                                                                   torch.equal(pipe_last[1].view(torch.int32), out[1].view(torch.int32))),
                     "rounds_ms_per_step": {"pipelined": [round(x, 4) for x in rp], "synchronous_interleaved": [round(x, 4) for x in rs]},
                     "synchronous_interleaved_ms_per_step": round(ms_, 4),
                     "note": "vdb_flat_search_batch_device_submit / _wait: batch i+1 is submitted before batch i is waited for; medians of 3 "
                             "interleaved rounds of --steps batches each (the headline `value` stays the contract's single W + K run)"}

    n_prof = max(3, min(args.steps, 10))
    kern_ms = kernel_ms_of(index, step, n_prof, local_rows) if args.full else 0.0
    n_launch = launches_of(stats, local_rows)                   # filter-pass launches of one step
    b_launch = -(-B // n_launch)                                # queries served by one launch (one fetch of the rows)
    alg_flops = 2.0 * b_launch * local_rows * dim               # 2*B*N*d per launch
    alg_bytes = 4.0 * local_rows * dim + 4.0 * b_launch * dim   #              4*N*d + 4*B*d per launch
    screened = bool(stats.get("bf16_screen"))
    # traffic: PMC bytes per launch of the profiled run profiles/traffic.json cites -- quoted ONLY when that run is the newest
    # PMC pass under profiles/ (a line must not carry an older tree's counters)
    traffic, traffic_src = None, None
    tp = os.path.join(ROOT, "profiles", "traffic.json")
    if args.full and os.path.exists(tp) and not distm and args.config == "c2" and n_rows == CONFIGS["c2"]["rows"] and dim == 768:
        try:
            tj = json.load(open(tp))
            key = "hbm_bytes_per_launch_bf16_screen" if screened else "hbm_bytes_per_launch"
            det = tj.get(key + "_detail") or {}
            if screened and det.get("tag") != newest_pmc_tag():
                traffic_src = f"not quoted: profiles/traffic.json cites {det.get('tag')}, the newest PMC pass under profiles/ is {newest_pmc_tag()}"
            else:
                traffic = tj.get(key)
                traffic_src = det.get("source") or tj.get("source")
        except Exception:
            traffic = None

    def roofline_of(kms, screened_):
        tf = alg_flops / (kms * 1e-3) / 1e12 if kms > 0 else 0.0
        gbs = alg_bytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
        axes = {
            "hbm": {"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                    "algorithmic_bytes_per_launch": alg_bytes},
            "f32_mfma": {"achieved": round(tf, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_F32_MFMA_TFLOPS, 4),
                         "algorithmic_flops_per_launch": alg_flops},
        }
        if screened_:
            axes["f32_mfma"]["note"] = ("NOT the binding axis of this kernel: its contraction runs on the bf16 matrix cores, so the algorithmic "
                                        "f32 FLOP rate exceeds the f32-MFMA peak (frac > 1); the f32-MFMA-bound path of SURVEY 8(d) is "
                                        "reported in f32_exact_tier")
            axes["bf16_mfma"] = {"achieved": round(tf, 1), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_MFMA_TFLOPS, 4)}
            b = axes["hbm"]
            wide = b_launch > 256
            r = {"bound": "hbm", "achieved": b["achieved"], "peak": b["peak"], "unit": b["unit"], "frac": b["frac"],
                 "kernel": ("fused_bf16w_kernel (8 waves, 128 rows x 512 queries per workgroup: every fetched row tile serves 512 queries; "
                            if wide else "fused_bf16p_kernel (8 waves, 256 rows x 256 queries, ") +
                           "f32 rows by LDS-DMA into a 3-image ring, one mid-stage barrier per K stage, bf16 MFMA 32x32x16 scores, threshold filter"
                           + ("; Dot / Euclid instance with per-row error margins)" if metric != 1 else ")"),
                 "queries_per_launch": b_launch, "launches_per_step": n_launch}
        else:
            b = axes["f32_mfma"]
            r = {"bound": "mfma", "achieved": b["achieved"], "peak": b["peak"], "unit": b["unit"], "frac": b["frac"],
                 "kernel": "fused_score_filter_dma3_kernel (8 waves, 128 rows x 256 queries, f32-input MFMA 32x32x2, 3-image LDS-DMA ring)"}
        r.update({"binding_axis": "hbm" if screened_ else "f32_mfma", "axes": axes, "kernel_ms": round(kms, 4)})
        return r

    roofline = None
    if args.full:
        roofline = roofline_of(kern_ms, screened)
        roofline["traffic"] = traffic
        roofline["traffic_source"] = traffic_src

    # ---- the f32-exact tier (measured before the headline, see above)
    f32_tier = None
    if screened and f32_raw is not None:
        el32, n_f32, out_f32, k32 = f32_raw
        same = bool(torch.equal(out_f32[0], out[0]) and torch.equal(out_f32[1].view(torch.int32), out[1].view(torch.int32)))
        f32_tier = {"value": round(B * n_f32 / el32, 2), "unit": "queries/s", "ms_per_step": round(1e3 * el32 / n_f32, 4),
                    "dtype": "f32 (f32-input MFMA scores, exact f32 re-rank)", "results_identical_to_default_path": same,
                    "roofline": roofline_of(k32, False)}

    # ---- opt-in bf16 shadow rows (vdb_flat_set_shadow): +50 % device memory, the filter pass streams 2 bytes per element.
    # Same index, same queries, same results; reported beside the headline (which keeps the f32 rows), never as `value`.
    shadow = None
    if not distm and screened and not args.no_shadow and dim % 64 == 0 and mask_t is None:
        index.set_shadow(True)
        els, outs = timed(step, max(3, args.warmup), args.steps)
        sst = index.last_stats()
        outs = tuple(t.clone() for t in outs)
        ks = kernel_ms_of(index, step, n_prof, local_rows)
        index.set_shadow(False)
        sh_bytes = 2.0 * local_rows * dim + 2.0 * min(B, 256) * dim
        sh_flops = 2.0 * min(B, 256) * local_rows * dim
        shadow = {"value": round(B * args.steps / els, 2), "unit": "queries/s", "ms_per_step": round(1e3 * els / args.steps, 4),
                  "used": bool(sst.get("shadow_rows")), "extra_device_memory_bytes": int(2 * local_rows * dim),
                  "results_identical_to_default_path": bool(torch.equal(outs[0], out[0]) and torch.equal(outs[1].view(torch.int32), out[1].view(torch.int32))),
                  "kernel": "fused_s16_kernel (4 waves x 512 registers, 256 rows x 256 queries, 128 x 128 per wave with hand-allocated AccVGPR "
                            "accumulators; bf16 rows 128 B per request into a 3 x 32 KB ring, queries into a 3 x 16 KB ring)",
                  "kernel_ms": round(ks, 4),
                  "axes": {"hbm": {"achieved": round(sh_bytes / (ks * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                   "frac": round(sh_bytes / (ks * 1e-3) / 1e9 / PEAK_HBM_GBS, 4), "algorithmic_bytes_per_launch": sh_bytes},
                           "bf16_mfma": {"achieved": round(sh_flops / (ks * 1e-3) / 1e12, 1), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                                         "frac": round(sh_flops / (ks * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4)}},
                  "note": "neither axis binds alone: DMA only 0.26 ms, MFMA + fragment reads only 0.27 ms (the clock the chip holds under "
                          "a dense bf16 MFMA loop), the per-tile epilogue ~0.08 ms with one wave per SIMD (DESIGN.md 4.3)"}

    # ---- the harder distribution of SURVEY 8(d): unit-normalised Gaussian rows, Gaussian queries, same size.  Three rounds,
    # each followed by a round on the UNIFORM index in the same clock state (control): the comparison the line makes is
    # between those pairs, not with the headline taken a minute earlier.
    gauss = None
    if not distm and DATA == "uniform" and args.config == "c2" and not args.no_gauss:
        gidx = build_index(vdb, metric, 0, n_rows, n_rows, dim, device, local_rank, data="gauss")
        gq = gen_queries(B, dim, device, data="gauss")
        gsearch = gpu_local_search(gidx, reuse_outputs=True)
        gel, gout = timed(lambda: gsearch(gq, k), max(args.warmup, 5), args.steps)
        rg, ru = [1e3 * gel / args.steps], []
        for r_ in range(3):
            if r_:
                rg.append(1e3 * timed(lambda: gsearch(gq, k), 3, args.steps)[0] / args.steps)
            ru.append(1e3 * timed(step, 3, args.steps)[0] / args.steps)
        gout = gsearch(gq, k)
        gst = gidx.last_stats()
        gk = kernel_ms_of(gidx, lambda: gsearch(gq, k), n_prof, n_rows)
        uk = kernel_ms_of(index, step, n_prof, local_rows)
        mg_ = float(np.median(rg))
        gauss = {"value": round(B / (mg_ * 1e-3), 2), "unit": "queries/s", "ms_per_step": round(mg_, 4),
                 "kernel_ms": round(gk, 4), "hbm_frac": round(alg_bytes / (gk * 1e-3) / 1e9 / PEAK_HBM_GBS, 4) if gk > 0 else None,
                 "rounds_ms_per_step": {"gauss": [round(x, 4) for x in rg], "uniform_interleaved": [round(x, 4) for x in ru]},
                 "uniform_interleaved_ms_per_step": round(float(np.median(ru)), 4), "uniform_interleaved_kernel_ms": round(uk, 4),
                 "path_stats": {x: gst[x] for x in ("uncertified", "rethreshold_queries", "f32_tier_queries", "exact_queries", "pool_overflows")},
                 "data": "unit-normalised Gaussian rows, Gaussian queries (seeded)"}
        if not args.no_cpu:
            import oracle
            grows = host_rows(n_rows, dim, device, data="gauss")
            gi, gd = gout[0].cpu().numpy().astype(np.uint64), gout[1].cpu().numpy()
            ok = True
            for b in (0, B - 1):
                oi, od = oracle.flat_search(metric, grows, gq[b].cpu().numpy(), k)
                ok &= bool(np.array_equal(oi, gi[b, :len(oi)]) and np.array_equal(od.view(np.uint32), gd[b, :len(od)].view(np.uint32)))
            gauss["ids_and_distances_bit_identical_to_oracle"] = ok
            gauss["queries_checked"] = 2
            del grows
        del gidx, gsearch, gout

    # ---- the host-pointer entry point (vdb_flat_search_batch): queries cross PCIe in, results out, per batch.
    # Reported beside the headline, never as `value`.
    host_io = None
    if not distm and not args.no_cpu and mask_t is None:
        q_pin = queries.cpu().numpy()
        for _ in range(3):
            index.search_batch_arrays(q_pin, k)
        t1 = time.perf_counter()
        n_io = 10
        for _ in range(n_io):
            index.search_batch_arrays(q_pin, k)
        el = time.perf_counter() - t1
        host_io = {"value": round(B * n_io / el, 2), "unit": "queries/s", "ms_per_step": round(1e3 * el / n_io, 4),
                   "note": "host numpy arrays in and out (H2D of the queries, D2H of ids/distances/counts inside the step)"}

    # ---- the same W + K measurement on a GPU that was idle for 20 ms: what a caller sees whose batches do not arrive back to back
    # (the device drops its clocks within milliseconds of idling and takes longer than W steps to bring them back)
    after_idle = None
    if not distm and args.full and not args.lean:
        torch.cuda.synchronize()
        time.sleep(0.02)
        el_i, _ = timed(step, args.warmup, args.steps)
        after_idle = {"idle_ms": 20, "ms_per_step": round(1e3 * el_i / max(args.steps, 1), 4), "value": round(B * args.steps / el_i, 2), "unit": "queries/s",
                      "note": "the headline's W + K steps again, after 20 ms of an idle GPU (the headline itself runs right behind other work); "
                              "profiles/r03_clock_series.log has the time series"}

    # ---- ONE index over all N GPUs inside ONE process (vdb_flat_create_sharded): the object the reference's single server
    # process would hold behind `impl Index`.  Rank 0 builds it over devices 0..N-1 and times the same batch while the other
    # ranks idle on a host-side (gloo) wait -- no kernel of theirs sits on the GPUs.  Bounded: a watchdog thread gives up
    # after --single-process-timeout seconds, the line says so, and the headline above is unaffected either way.
    single, leg_hung = None, False
    if not args.no_single_process and args.config in ("c2", "c4") and mask_t is None:
        if distm:
            torch.distributed.barrier(group=gloo)
        if rank == 0:
            box = {}

            def leg():
                try:
                    box["r"] = single_process_leg(vdb, metric, n_rows, dim, B, k, world, args, out)
                except Exception as e:                               # noqa: BLE001 -- reported in the line
                    box["r"] = {"error": f"{type(e).__name__}: {e}"}

            th = threading.Thread(target=leg, daemon=True)
            th.start()
            th.join(240.0)
            single = box.get("r") or {"error": "timed out after 240 s (the leg was abandoned; the headline is unaffected)"}
            leg_hung = th.is_alive()
        if distm:
            flag = torch.tensor([1 if leg_hung else 0], dtype=torch.int32)
            torch.distributed.broadcast(flag, src=0, group=gloo)
            leg_hung = bool(flag.item())

    # ---- cpu_baseline (rank 0, N=1 only): the oracle restatement of the reference, 1 core, bounded sample
    cpu, recall, parity_n = None, None, None
    if rank == 0 and not args.no_cpu and n_rows * dim <= 2_000_000_000:
        import oracle
        ids_g = out[0].cpu().numpy().astype(np.uint64)
        dist_g = out[1].cpu().numpy()
        rows_host = host_rows(n_rows, dim, device)
        q_host = queries.cpu().numpy()
        live_host = None
        if mask_t is not None:
            live_host = np.unpackbits(mask_t.cpu().numpy().view(np.uint8), bitorder="little")[:n_rows].astype(np.uint8)
        oracle.lib()
        # N = 1: the timed CPU baseline (about cpu-seconds of whole queries); N > 1: two queries, parity only
        budget = args.cpu_seconds if not distm else 0.0
        done, t_cpu, recs, exact = 0, 0.0, [], True
        while done < B and (done < 2 or t_cpu < budget):
            t1 = time.perf_counter()
            oi, od = oracle.flat_search(metric, rows_host, q_host[done], k, live=live_host)
            t_cpu += time.perf_counter() - t1
            recs.append(oracle.recall(oi, ids_g[done, :k]))
            exact &= bool(np.array_equal(oi, ids_g[done, :len(oi)]) and np.array_equal(od, dist_g[done, :len(od)]))
            done += 1
        recall = float(np.mean(recs))
        if not distm:
            cpu = {"value": round(done / t_cpu, 4), "unit": "queries/s", "cores": 1, "kind": "port",
                   "sample": f"{done} of {B} queries against all {n_rows} rows, {t_cpu:.1f} s; oracle/flat_oracle.c "
                             f"(C restatement of the reference's single-threaded FlatIndex::search; the Rust reference "
                             f"cannot be built in this image)",
                   "host_cpus": os.cpu_count(), "ids_and_distances_bit_identical": exact}
            # second, clearly separate row: the same port on several cores, one whole query
            # per thread (the reference itself is single-threaded on this path; ctypes releases the GIL)
            import concurrent.futures
            nthr = int(min(16, os.cpu_count() or 1, B))
            t1 = time.perf_counter()
            with concurrent.futures.ThreadPoolExecutor(nthr) as ex:
                list(ex.map(lambda b: oracle.flat_search(metric, rows_host, q_host[b], k, live=live_host), range(nthr)))
            t_mt = time.perf_counter() - t1
            cpu["all_cores_row"] = {"value": round(nthr / t_mt, 3), "unit": "queries/s", "cores": nthr,
                                    "sample": f"{nthr} queries, one per thread, {t_mt:.1f} s"}
        else:
            parity_n = {"queries_checked_against_oracle": done, "ids_and_distances_bit_identical": exact}

    if rank == 0:
        mname = ["euclidean", "cosine", "dot"][metric]
        line = {
            "metric": f"QPS, FlatIndex brute-force kNN {n_rows}x{dim} f32 {mname} batch={B} k={k} (recall@{k} vs reference algorithm)"
                      if args.config != "c2" or args.rows else
                      "QPS, FlatIndex brute-force kNN 1Mx768 f32 cosine batch=256 k=10 (recall@10 vs reference algorithm)",
            "value": round(qps, 2), "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": cfg["scaling"], "vs_baseline": None,
            "dtype": ("f32 results (exact f32 re-rank in the reference's operation order); candidates RANKED by bf16-MFMA screening under a tested error bound"
                      if screened else "f32 (f32-input MFMA scores, exact f32 re-rank)"),
            "data": "synthetic" if DATA == "uniform" else "synthetic (unit-normalised Gaussian rows)",
            "config": {"workload": cfg["workload"], "name": args.config,
                       "n_rows": n_rows, "rows_per_gpu": local_rows, "dim": dim, "batch": B, "k": k, "distance": mname,
                       "sharding": f"rows/{world}, one process per GPU, exchange = RCCL all-gather + merge behind the C ABI (vdb_flat_search_batch_sharded)"
                                   if group is not None else (f"rows/{world}, one process per GPU, exchange = torch.distributed all-gathers + HIP merge (fallback)" if distm else "single GPU"),
                       "inputs": "queries and outputs resident in HBM",
                       "arithmetic": ("rows, queries and every reported distance are f32 (exact re-rank in the reference's operation "
                                      "order, bit-identical to the f32 oracle); candidates are RANKED by bf16-MFMA scores under an error "
                                      "bound that tests/test_gpu_certificate.py checks pair by pair on adversarial data; uncertified "
                                      "queries go to a re-threshold pass, the f32-MFMA tier, then an exact scan") if screened else
                                     "f32 throughout (f32-input MFMA scores, exact f32 re-rank)",
                       "filter": filt},
            "rccl_ranks": rccl_ranks,
            "recall_at_k": recall,
            "path_stats": stats,
            "roofline": roofline,
            "pipelined_two_in_flight": pipelined,
            "shadow_rows": shadow,
            "f32_exact_tier": f32_tier,
            "gauss_dataset": gauss,
            "pcie_inclusive": host_io, "after_idle": after_idle, "synchronous_rounds_before_headline_ms_per_step": repeat_rounds, "exchange": exchange_note,
            "single_process_sharded": single,
            "cpu_baseline": cpu,
        }
        if args.config == "c2":
            line["recall_at_10"] = recall
        if parity_n is not None:
            line["parity"] = parity_n
        print(json.dumps(line), flush=True)
    if distm:
        torch.distributed.barrier(group=gloo)
    if leg_hung:
        # an abandoned single-process leg still holds a thread inside the library: no teardown, no interpreter shutdown -- the
        # line is out and the ranks are in step, so every rank leaves at once
        sys.stdout.flush()
        os._exit(0)
    if distm:
        del group
        torch.distributed.destroy_process_group()


def single_process_leg(vdb, metric, n_rows, dim, B, k, n_dev, args, ref_out):
    """ONE GpuFlatIndex(devices=[0..n_dev-1]) in this process: build, W + K timed steps, results against the headline's."""
    dev0 = torch.device("cuda", 0)
    t_b = time.perf_counter()
    idx = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), devices=list(range(n_dev)), keep_host_copy=False)
    idx.reserve(n_rows, dim)
    chunk = min(CHUNK, n_rows)
    with torch.cuda.device(dev0):
        for c in range((n_rows + chunk - 1) // chunk):
            c0, c1 = c * chunk, min((c + 1) * chunk, n_rows)
            block = gen_chunk(c, c1 - c0, dim, dev0)
            torch.cuda.synchronize(dev0)
            idx.add_bulk_device(block.data_ptr(), c1 - c0, dim, first_id=c0)
            del block
        idx.flush()
        build_s = time.perf_counter() - t_b
        q = gen_queries(B, dim, dev0)
        o_i = torch.empty((B, k), dtype=torch.int64, device=dev0)
        o_d = torch.empty((B, k), dtype=torch.float32, device=dev0)
        o_c = torch.empty((B,), dtype=torch.int32, device=dev0)
        torch.cuda.synchronize(dev0)

        def one():
            idx.search_batch_device(q.data_ptr(), B, dim, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())

        res = {"shards": idx.shards(), "rows_per_shard": [idx.shard_len(g) for g in range(idx.shards())], "build_s": round(build_s, 2)}
        modes = [("rccl", vdb.GpuFlatIndex.EXCHANGE_RCCL), ("peer", vdb.GpuFlatIndex.EXCHANGE_PEER)]
        for name, mode in modes:
            idx.set_exchange(mode)
            for _ in range(max(args.warmup, 3)):
                one()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                one()
            el = time.perf_counter() - t1
            st = idx.shard_stats()
            same = bool(torch.equal(o_i.cpu(), ref_out[0].cpu()) and torch.equal(o_d.cpu().view(torch.int32), ref_out[1].cpu().view(torch.int32)))
            res[name] = {"value": round(B * args.steps / el, 2), "unit": "queries/s", "ms_per_step": round(1e3 * el / args.steps, 4),
                         "exchanges_per_step": st["exchanges"], "rccl_ranks": st["rccl_ranks"],
                         "host_enqueue_us": round(st["host_enqueued_ns"] / 1e3, 1),
                         "results_identical_to_headline": same}
        res["note"] = ("vdb_flat_create_sharded: ONE vdb_flat_index whose rows are dealt to the listed GPUs inside this process (a worker thread "
                       "and a stream per shard); 'rccl' = grouped ncclAllGather over in-process communicators (the default), 'peer' = "
                       "hipMemcpyPeerAsync of every shard's packed block into device 0; synchronous steps, queries and outputs on device 0")
    del idx
    return res


if __name__ == "__main__":
    main()
