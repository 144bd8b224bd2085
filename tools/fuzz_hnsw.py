#!/usr/bin/env python3
"""Randomised differential test of the HNSW index: random sizes, dimensions, metrics, m / ef_construction / ef, data with
duplicates, interleaved removals and re-inserts -- a share of the single adds and of a second bulk use ids that are present
or were removed (graph.rs:260-261 replaces the node and counts it again), some with a forced level, and the second bulk may
name an id twice; the product's graph must equal the CPU restatement's (same seed) and every search result must be identical
(ids, order, distance bits) -- through the device-resident search.

    python tools/fuzz_hnsw.py [--cases N] [--seed S]

--lifecycle runs random schedules of tests/hnsw_lifecycle.py instead (mutations and reads interleaved, every walk on the device
and on the host route, vdb_hnsw_mirror_stats against the model after every read) and shrinks a failing one to a literal trace:

    python tools/fuzz_hnsw.py --lifecycle [--cases N] [--seed S]
    python tools/fuzz_hnsw.py --lifecycle --mutants        (no GPU: which pinned schedule catches which mutant, at which step)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_package  # noqa: E402
import oracle  # noqa: E402


def lifecycle(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hnsw_lifecycle as hl
    if a.mutants:
        for name in hl.PINNED:
            trace, caught = hl.pinned(name), []
            hl.run(trace, hl.MirrorRef(trace), expected=hl.slots(name))
            for mutant in hl.MUTANTS:
                try:
                    hl.run(trace, mutant(trace), expected=hl.slots(name), counters=False)
                except hl.Mismatch as e:
                    step = int(str(e).split("step ")[1].split(" ")[0])
                    caught.append(f"{mutant.__name__} (step {step}, {trace['ops'][step][0]})")
            print(f"[{name}] {len(trace['ops'])} ops: " + (", ".join(caught) or "none"), flush=True)
        return
    vdb = load_package()
    vdb.build()
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    for case in range(a.cases):
        seed, metric = int(rng.integers(1, 1 << 30)), int(rng.integers(0, 3))
        d, m, base = int(rng.choice([8, 16, 33])), int(rng.choice([4, 6, 16])), int(rng.integers(300, 1501))
        trace = hl.schedule(seed, metric, d, m, base)
        try:
            model, stats, walked = hl.run_gpu(vdb, trace)
        except hl.Mismatch as e:
            print(f"FAIL case {case}: {str(e).splitlines()[0]}", flush=True)
            small = hl.shrink_gpu(vdb, trace, log=print)
            print(f"shrunk: TRACE = {small!r}", flush=True)
            sys.exit(1)
        print(f"ok   case {case}: seed={seed} metric={metric} d={d} m={m} base={base} ops={len(trace['ops'])} device walks {walked} "
              f"mirror_stats {stats}", flush=True)
    print(f"ALL {a.cases} HNSW LIFECYCLE CASES OK in {time.time() - t0:.0f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lifecycle", action="store_true", help="random lifecycle schedules (tests/hnsw_lifecycle.py) instead")
    ap.add_argument("--mutants", action="store_true", help="with --lifecycle, on the CPU: the pinned schedules against the mutants")
    a = ap.parse_args()
    if a.lifecycle:
        return lifecycle(a)
    vdb = load_package()
    vdb.build()
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    dev_q = host_q = 0
    for case in range(a.cases):
        n = int(rng.integers(50, 4000))
        d = int(rng.choice([1, 2, 7, 16, 33, 64, 128, 300]))
        metric = int(rng.integers(0, 3))
        m = int(rng.choice([2, 4, 8, 16, 19, 24]))
        efc = int(rng.choice([8, 32, 100, 200, 520]))            # 520: the insert walks' result heap beyond the wave pop (514)
        kind = str(rng.choice(["uniform", "gauss", "dups"]))
        if kind == "uniform":
            rows = rng.random((n, d), dtype=np.float32)
        elif kind == "gauss":
            rows = rng.standard_normal((n, d)).astype(np.float32)
        else:
            base = rng.random((max(n // 8, 1), d), dtype=np.float32)
            rows = base[rng.integers(0, base.shape[0], n)]
        if metric == 1:
            rows[np.linalg.norm(rows, axis=1) == 0] += 1.0
        seed = int(rng.integers(1, 1 << 30))
        g = vdb.GpuHnswIndex(vdb.DistanceMetric(metric), vdb.HnswParams.new(m, efc, 50), seed=seed)
        o = oracle.HnswOracle(metric, m=m, ef_construction=efc, ef_search=50, seed=seed)
        perm = rng.permutation(n * 2)
        ids, spare = perm[:n], perm[n:]
        half = n // 2
        g.build_batch((ids[:half].astype(np.uint64), rows[:half]))
        for i in range(half):
            o.insert(int(ids[i]), rows[i])
        removed = set()
        for v in rng.choice(ids[:half], size=min(half, int(rng.integers(0, 40))), replace=False):
            g.remove(int(v)); o.remove(int(v)); removed.add(int(v))
        present, readds = set(int(x) for x in ids[:half]) - removed, 0

        def seen_id():                                             # an id the graph has held before: removed (if any is left) or present
            nonlocal readds
            pool = sorted(removed) if removed and rng.random() < 0.5 else sorted(present)
            readds += 1
            return int(pool[int(rng.integers(0, len(pool)))])

        def took(i):
            removed.discard(i); present.add(i)

        for i in range(half, n):                                   # single adds after the removals; one in ten re-uses an id
            again = rng.random() < 0.1
            nid = seen_id() if again else int(ids[i])
            level = int(rng.integers(0, 4)) if again and rng.random() < 0.5 else -1
            g.add(nid, vdb.Vector(rows[i]), level=level)
            o.insert(nid, rows[i], level)
            took(nid)
        # a second bulk: fresh ids, ids seen before, now and then the same id twice; other vectors of the same data
        nb = int(min(max(n // 4, 1), 96))
        bulk_ids = []
        for t in range(nb):
            r = rng.random()
            bulk_ids.append(seen_id() if r < 0.15 else (bulk_ids[int(rng.integers(0, t))] if r < 0.2 and t else int(spare[t])))
        bulk_rows = rows[rng.integers(0, n, nb)] if kind == "dups" else rng.permutation(rows)[:nb] * np.float32(0.9)
        bulk_rows = np.ascontiguousarray(bulk_rows, dtype=np.float32)
        g.build_batch((np.array(bulk_ids, dtype=np.uint64), bulk_rows))
        for nid, v in zip(bulk_ids, bulk_rows):
            o.insert(nid, v)
            took(nid)
        desc = f"case {case}: n={n} d={d} metric={metric} m={m} efc={efc} data={kind} removed={len(removed)} re-adds={readds}"
        ok = g.len() == len(o) and g.entry_point() == o.entry_point()
        for i in list(ids) + [int(x) for x in spare[:nb]]:
            lv = o.level(int(i))
            ok &= g.level(int(i)) == lv
            for l in range(max(lv, -1) + 1):
                ok &= g.neighbors(int(i), l) == o.neighbors(int(i), l)
        nq = int(rng.choice([1, 5, 64]))
        q = rng.standard_normal((nq, d)).astype(np.float32) if kind == "gauss" else rng.random((nq, d), dtype=np.float32)
        if metric == 1:
            q[np.linalg.norm(q, axis=1) == 0] += 1.0
        for (k, ef) in [(10, 100), (1, 16), (int(rng.integers(1, 60)), int(rng.choice([10, 50, 300, 513, 514, 1022])))]:   # 513 / 514: the last wave pop, the first single-lane pop
            gi, gd, gc = g.search_batch_arrays(q, k, ef)
            for b in range(nq):
                oi, od = o.search(q[b], k, ef)
                ok &= bool(gc[b] == len(oi) and np.array_equal(gi[b, :gc[b]], oi) and np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)))
        # pre-filtered search with a random id mask: the device walk equals the host traversal, results are eligible; an
        # all-ones mask is the unfiltered search
        bits = int(n * 2 + rng.integers(0, 100))
        sel = float(rng.choice([1.0, 0.5, 0.1, 0.02, 0.0]))
        elig = rng.random(bits) < sel
        packed = np.zeros(((bits + 63) // 64) * 8, dtype=np.uint8)
        pb = np.packbits(elig, bitorder="little")
        packed[:pb.size] = pb
        mask = packed.view(np.uint64)
        k, ef = int(rng.integers(1, 30)), int(rng.choice([10, 50, 200]))
        dev = g.search_batch_arrays(q, k, ef, id_mask=mask, mask_bits=bits)
        g.set_traversal(True)
        host = g.search_batch_arrays(q, k, ef, id_mask=mask, mask_bits=bits)
        g.set_traversal(False)
        for b in range(nq):
            c = int(dev[2][b])
            ok &= bool(c == host[2][b] and np.array_equal(dev[0][b, :c], host[0][b, :c]) and
                       np.array_equal(dev[1][b, :c].view(np.uint32), host[1][b, :c].view(np.uint32)))
            ok &= all(bool(elig[int(i)]) for i in dev[0][b, :c])
        if sel == 1.0:
            plain = g.search_batch_arrays(q, k, ef)
            ok &= bool(np.array_equal(plain[2], dev[2]) and all(np.array_equal(plain[0][b, :plain[2][b]], dev[0][b, :dev[2][b]]) for b in range(nq)))
        desc += f" mask sel={sel}"
        st = g.stats()
        dev_q += st["device_queries"]; host_q += st["host_redone"]
        print(("ok   " if ok else "FAIL ") + desc + f"  [device walks {st['device_queries']} host re-runs {st['host_redone']} host rounds {st['last_search_rounds']}]", flush=True)
        if not ok:
            sys.exit(1)
    print(f"ALL {a.cases} HNSW CASES OK in {time.time() - t0:.0f} s; device-resident walks {dev_q}, host re-runs {host_q}", flush=True)


if __name__ == "__main__":
    main()
