#!/usr/bin/env python3
"""Long-run companion of tools/fuzz_parity.py for the STATE an index carries between calls: fresh lifecycle schedules
(tests/lifecycle.py: interleaved adds, upserts, removes, compactions, setting changes and every kind of read) instead of the
pinned ones of tests/test_gpu_lifecycle.py, every read compared bit for bit with the model.  A mismatch prints the failing
trace, shrinks it (ops are dropped greedily while the failure persists) and prints the shrunk trace as a literal that
lifecycle.run() replays; the exit status is then non-zero.

    python tools/fuzz_lifecycle.py [--cases N] [--seed S] [--store] [--sharded] [--large] [--twelve]

--store drives VectorStore with store-level schedules, --sharded one sharded handle over three shards on device 0, --large draws the
short 75 000-row schedules that reach the bf16 screening tier and the screened range route.  --twelve draws the schedules of the
MMR, per-group and recommend-by-best reads instead: the profiles "twelve" and "twelve-auto" (all twelve read kinds, the two debug
switches), with --store the store schedules that hold search_mmr, search_groups and recommend_best_batch (and the numeric fields),
with --large the 75 000-row twelve-kind schedule.  Without --twelve a seed names the case it always named.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import load_package  # noqa: E402
import lifecycle as lc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--store", action="store_true")
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--twelve", action="store_true")
    args = ap.parse_args()
    vdb = load_package()
    vdb.build()
    profiles = ["twelve", "twelve-auto"] if args.twelve else sorted(p for p in lc.PROFILES if not p.startswith("twelve"))
    t0, reads = time.time(), 0
    for case in range(args.cases):
        seed, metric = args.seed + case, case % 3
        if args.store:
            trace = lc.store_schedule(seed, metric, table_at=("mid", "start")[case % 2], auto=(0.0, 0.4)[(case // 2) % 2],
                                      numeric=args.twelve, twelve=args.twelve)
            make = lambda: lc.GpuStoreAdapter(vdb, metric, auto_compact=trace["auto"])   # noqa: E731
        else:
            if args.large:
                trace = lc.large_twelve_schedule(seed, metric).trace if args.twelve else lc.large_schedule(seed, metric)
            else:
                trace = lc.schedule(seed, profiles[(case // 3) % len(profiles)], metric)
            make = lambda: lc.GpuIndexAdapter(vdb, metric, devices=[0, 0, 0] if args.sharded else None)   # noqa: E731
        made = []

        def fresh():
            made.append(make())
            return made[-1]
        try:
            lc.run(trace, fresh())
        except lc.Mismatch as e:
            print(f"case {case}: MISMATCH\n{e}\nshrinking ...", flush=True)
            small = lc.shrink(trace, fresh, log=print)
            if small is None:
                print("the failure did not happen again on a fresh adapter: the trace above is all there is")
            else:
                print(f"shrunk to {len(small['ops'])} ops:\nTRACE = {small!r}")
            return 1
        finally:
            for ad in made:
                ad.close()
        reads += sum(1 for op in trace["ops"] if lc.is_read(op))
        print(f"case {case}: seed {seed} profile {trace['profile']} metric {metric}: {len(trace['ops'])} ops ok", flush=True)
    print(f"{args.cases} schedules, {reads} reads, no mismatch ({time.time() - t0:.0f} s)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
