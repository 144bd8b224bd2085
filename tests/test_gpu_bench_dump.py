"""`bench.py --dump-outputs DIR`: a plain run writes what its last timed step returned (ids, distances, counts), the same arrays on
every run with the same arguments, and they are the oracle's answers; the side measurements stay behind `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROWS, STEPS = 200_000, 4


def _plain(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(ROWS), "--steps", str(STEPS),
                        "--warmup", "1", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    arrays = {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("ids", "distances", "counts")}
    return line, arrays


def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    import oracle
    import torch
    import bench

    l1, a1 = _plain(tmp_path / "a")
    l2, a2 = _plain(tmp_path / "b")
    for l in (l1, l2):
        assert l["steps"] == STEPS and l["ms_per_step"] > 0 and l["value"] > 0
        assert l["roofline"] is None and l["cpu_baseline"] is None and l["f32_exact_tier"] is None
    B, k = l1["config"]["batch"], l1["config"]["k"]
    assert a1["ids"].shape == (B, k) and a1["ids"].dtype == np.float64
    assert a1["distances"].shape == (B, k) and a1["distances"].dtype == np.float32
    assert a1["counts"].shape == (B,) and a1["counts"].dtype == np.float64 and np.all(a1["counts"] == k)
    for n in a1:
        assert np.array_equal(a1[n].view(np.uint8), a2[n].view(np.uint8)), n
    dev = torch.device("cuda", 0)
    rows = bench.host_rows(ROWS, l1["config"]["dim"], dev)
    q = bench.gen_queries(B, l1["config"]["dim"], dev).cpu().numpy()
    for b in (0, B - 1):
        oi, od = oracle.flat_search(oracle.COSINE, rows, q[b], k)
        assert np.array_equal(a1["ids"][b].astype(np.uint64), oi) and np.array_equal(a1["distances"][b].view(np.uint32), od.view(np.uint32)), b
