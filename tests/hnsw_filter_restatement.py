"""A short Python restatement of the PRE-FILTERED search_knn (include/vdb_hnsw.h vdb_hnsw_search_batch_masked), walking the graph
of any object with entry_point() / neighbors(id, layer) -- oracle.HnswOracle or GpuHnswIndex -- with oracle.distance:

  - greedy descent on layers max_level .. 1 exactly as search_knn (graph.rs:397-403), no filter;
  - layer 0: search_layer(query, [ep], max(ef, k), 0) (graph.rs:143-199) where a visited node enters `candidates` under the
    unchanged rule (dist < furthest or len(results) < ef) but enters `results` only when eligible; `furthest` comes from the
    results (f32::MAX while there are none); the entry point is always a candidate, a result only when eligible;
  - output: the results sorted by distance, truncated to k.

Python's heapq stands in for Rust's BinaryHeap: the order of EQUAL distances may differ, so callers use data without ties
(Gaussian rows).  eligible = None is the unfiltered search_knn.

`peaks` (a dict handed to search) also receives the two quantities the device walk's capacities are stated in
(kernels_hnsw.hip), exactly and over EVERY layer searched, the greedy descent included:

  "pushed"         the largest length of `candidates` immediately after a push.  The kernel fails a walk that would push with
                   CAND_CAP (CAND_CAP_F when filtered) entries in the heap, so a walk fails on that cap iff this exceeds it.
                   ("candidates", the older key, is len + 1 once per expansion at layer 0: an upper bound, not this number.)
  "layer_visited"  the final len(visited) of each layer searched, in search order (max_level first, layer 0 last).  The
                   kernel clears and recounts its visited set per layer; the plain walk fails iff one of these exceeds 3/4 of
                   VIS_CAP."""
import heapq

import numpy as np

import oracle

F32_MAX = np.float32(3.40282347e+38)


class Walker:
    def __init__(self, graph, metric, rows_by_id):
        self.g, self.metric, self.rows = graph, int(metric), rows_by_id
        self._nbrs = {}

    def neighbors(self, nid, layer):
        key = (nid, layer)
        if key not in self._nbrs:
            self._nbrs[key] = self.g.neighbors(nid, layer) or []
        return self._nbrs[key]

    def search_layer(self, query, ep, ef, layer, eligible, peaks):
        dist = lambda nid: oracle.distance(self.metric, query, self.rows[nid])     # noqa: E731
        visited = {ep}
        d0 = dist(ep)
        cand = [(d0, ep)]                                       # min-heap: closest candidate first
        peaks["pushed"] = max(peaks.get("pushed", 0), 1)
        res = []                                                # max-heap by (distance, id) as (-d, -id)
        if eligible is None or eligible(ep):
            heapq.heappush(res, (-d0, -ep))
        while cand:
            cd, cid = heapq.heappop(cand)
            furthest = -res[0][0] if res else F32_MAX
            if cd > furthest:
                break
            for nid in self.neighbors(cid, layer):
                if nid in visited:
                    continue
                visited.add(nid)
                if nid not in self.rows:                        # deleted
                    continue
                d = dist(nid)
                furthest = -res[0][0] if res else F32_MAX
                if d < furthest or len(res) < ef:
                    heapq.heappush(cand, (d, nid))
                    if len(cand) > peaks["pushed"]:
                        peaks["pushed"] = len(cand)
                    if eligible is None or eligible(nid):
                        heapq.heappush(res, (-d, -nid))
                        if len(res) > ef:
                            heapq.heappop(res)
            peaks["candidates"] = max(peaks["candidates"], len(cand) + 1)
        peaks["visited"] = max(peaks["visited"], len(visited))
        peaks.setdefault("layer_visited", []).append(len(visited))
        out = sorted(((-nd, -ni) for nd, ni in res), key=lambda t: t[0])
        return [i for _, i in out], [d for d, _ in out]

    def search(self, query, k, ef, eligible=None, peaks=None):
        """-> (ids u64 array, dists f32 array); peaks (a dict) receives the layer-0 visited count and candidate-heap peak
        ("visited", "candidates") and the exact per-walk counters "pushed" and "layer_visited" (module docstring)."""
        peaks = {"visited": 0, "candidates": 0} if peaks is None else peaks
        peaks.setdefault("visited", 0); peaks.setdefault("candidates", 0); peaks.setdefault("pushed", 0)
        peaks["layer_visited"] = []                             # of THIS search; the three peaks accumulate over a reused dict
        ep, max_level = self.g.entry_point()
        if ep is None:
            return np.zeros(0, np.uint64), np.zeros(0, np.float32)
        for layer in range(max_level, 0, -1):
            upper = {"visited": 0, "candidates": 0, "pushed": peaks["pushed"], "layer_visited": peaks["layer_visited"]}
            ids, _ = self.search_layer(query, ep, 1, layer, None, upper)
            peaks["pushed"] = upper["pushed"]
            if ids:
                ep = ids[0]
        ids, ds = self.search_layer(query, ep, max(ef, k), 0, eligible, peaks)
        return np.array(ids[:k], dtype=np.uint64), np.array(ds[:k], dtype=np.float32)


def mask_of(eligible_bool):
    """bool array over ids -> (uint64 words, bits): the layout of vdb_flat_search_batch's id_mask."""
    bits = int(eligible_bool.size)
    words = (bits + 63) // 64
    packed = np.zeros(words * 8, dtype=np.uint8)
    pb = np.packbits(eligible_bool.astype(bool), bitorder="little")
    packed[:pb.size] = pb
    return packed.view(np.uint64), bits


def eligible_fn(eligible_bool):
    return lambda nid: nid < eligible_bool.size and bool(eligible_bool[nid])
