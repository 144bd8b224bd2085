"""How a tile starts and ends in the 4-wave kernel over bf16 rows (kernels_fused_s16.hip): nothing zeroes an accumulator -- the
first k-step of a tile issues its MFMAs with C = 0 over whatever the previous tile left -- and the epilogue reads the
accumulators out sub-tile by sub-tile, the row constants of a row block held in registers across its four sub-tiles.

None of it may change a bit of a score.  The shapes are the smallest at which the paths exist: with C compute units, tiles of
256 rows are dealt round-robin to C workgroups, so 256 C + 77 rows give some workgroups two tiles (a tile that starts over the
accumulators of another) and the rest one; 3 * 256 C - 300 rows give three tiles (an epilogue between two such starts), a
ragged last tile and one workgroup with two; 2 * 256 C is the even case.  At d = 64 a tile is ONE row stage, so the half-stage
that starts a tile is also the one in front of its last."""
import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu

SPLIT = 1
SHAPES = {"one_or_two": lambda c: 256 * c + 77, "three_ragged": lambda c: 3 * 256 * c - 300, "two_even": lambda c: 2 * 256 * c}
# (d, shape): both ragged shapes at every depth, the even one where a tile is a single stage
D_SHAPES = [(d, s) for d in (64, 128, 192) for s in ("one_or_two", "three_ragged")] + [(64, "two_even")]


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


_CU = []


def cu_count():
    if not _CU:
        import torch
        _CU.append(int(torch.cuda.get_device_properties(0).multi_processor_count))
    return _CU[0]


def n_rows(shape):
    return SHAPES[shape](cu_count())


_DATA = {}


def data(d, shape):
    """rows (norms spread over 0.1 .. 4) and 256 queries, made once per (d, shape) and never changed"""
    if (d, shape) not in _DATA:
        n = n_rows(shape)
        rng = np.random.default_rng(7 * d + len(shape))
        rows = rng.standard_normal((n, d), dtype=np.float32) * rng.uniform(0.1, 4.0, (n, 1)).astype(np.float32)
        q = rng.standard_normal((256, d), dtype=np.float32)
        rows.setflags(write=False)
        q.setflags(write=False)
        _DATA[(d, shape)] = (rows, q)
    return _DATA[(d, shape)]


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


def check_oracle(metric, rows, q, k, res, qsel, live=None):
    gi, gd, gc = res
    for b in qsel:
        oi, od = oracle.flat_search(metric, rows, q[b], k, live=live)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), (b, gi[b, :gc[b]], oi)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc[b]], od)


def tiles_of_the_busiest_late_workgroup(n):
    """first rows of the tiles of the workgroup that owns the LAST tile (the ragged one where there is one), in the order it runs them"""
    c = cu_count()
    nblk = (n + 255) // 256
    w = (nblk - 1) % c
    return [256 * b for b in range(w, nblk, c)]


# ------------------------------------------------------------------ raw scores
@pytest.mark.parametrize("d,shape", D_SHAPES)
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_raw_scores_equal_the_f32_row_kernels_bit_for_bit(vdb, metric, d, shape):
    """Every (query, row) score of the production filter pass over the bf16 shadow (this kernel) carries the f32 bits the
    f32-row kernel gives -- which no tile start of this file touches: the plain scores and the lower-bound scores of Dot /
    Euclid (the MARGIN instance), 1, 19 and 256 queries, a few hundred tombstones."""
    rows, q = data(d, shape)
    n = len(rows)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
    ix.add_bulk(rows)
    # tombstones at the head, in the ragged tail and on the last row of every full tile of the workgroup that runs the last tile
    for r in sorted(set(range(3, 900, 7)) | set(range(n - 400, n, 3)) | {t + 255 for t in tiles_of_the_busiest_late_workgroup(n)[:-1]}):
        ix.remove(r)
    ix.set_shadow(True)
    ix.search_batch_arrays(q[:3], 5)
    assert ix.last_stats()["shadow_rows"] == 1                    # the kernel under test serves this index
    for nq in (1, 19, 256):
        for raw in (0, 1):
            ix.set_shadow(True)
            a = ix.debug_screen_scores(q[:nq], raw=raw)[0]
            ix.set_shadow(False)
            b = ix.debug_screen_scores(q[:nq], raw=raw)[0]
            assert a.shape == (nq, n)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (metric, d, shape, nq, raw)
            assert np.isfinite(b[:, 1000]).all() and np.isnan(b[:, 3]).all()          # a live row has a score, a tombstone none


# ------------------------------------------------------------------ both copies of the scoring code across tile boundaries
@pytest.mark.parametrize("d,shape", [(64, "one_or_two"), (64, "three_ragged"), (64, "two_even"), (192, "three_ragged")])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_both_epilogue_copies_across_tile_boundaries(vdb, metric, d, shape):
    """The epilogue exists twice -- with the NaN test per group (some norm of the launch outside [2^-40, 2^40]) and without
    it -- and a tile follows either copy.  Tame rows run the copy without, rows with huge / tiny norms, inf and NaN
    elements in the first, a middle and the last tile of ONE workgroup run the copy with it: results equal the f32 tier's
    (set_screen(0)) and the oracle's, ids and distance bits."""
    base, q256 = data(d, shape)
    q, k = q256[:24], 10
    n = len(base)
    starts = tiles_of_the_busiest_late_workgroup(n)
    picks = [starts[0], starts[len(starts) // 2], starts[-1]] if len(starts) > 2 else [starts[0], starts[-1]]
    spots = [t + min(o, n - 1 - t) for t, o in zip(picks, (5, 130, 201))]            # rows of both row halves of a tile

    def index(rows):
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
        ix.set_shadow(True)
        ix.add_bulk(rows)
        return ix

    def both_tiers(ix):
        out = []
        for screen in (1, 0):
            ix.set_screen(screen)
            try:
                out.append(ix.search_batch_arrays(q, k))
            except vdb.VectorDbError as e:
                out.append(str(e))
            st = ix.last_stats()
            assert st["bf16_screen"] == screen
            if screen:
                assert st["shadow_rows"] == 1, st
        return out

    # tame: the copy without the NaN test
    a, b = both_tiers(index(base))
    assert not isinstance(a, str) and same(a, b)
    check_oracle(metric, base, q, k, a, [0, 23])
    # huge and tiny norms: the copy with it
    rows = base.copy()
    for i, r in enumerate(spots):
        rows[r] *= np.float32(1e25) if i % 2 == 0 else np.float32(1e-22)
        rows[r - 1] *= np.float32(1e-22) if i % 2 == 0 else np.float32(1e25)
    a, b = both_tiers(index(rows))
    assert not isinstance(a, str) and same(a, b)
    check_oracle(metric, rows, q, k, a, [0, 23])
    # an inf element per tile: inf distances (Euclid, Dot: sorted without complaint) or NaN (Cosine: the NaN error) -- whatever
    # the f32 tier does, the screening tier does; then a NaN element in the last tile: the NaN error from both
    rows = base.copy()
    for r in spots:
        rows[r, 3] = np.float32("inf")
    a, b = both_tiers(index(rows))
    if metric == 1:
        assert isinstance(a, str) and "NaN" in a and a == b, (a, b)
    else:
        assert not isinstance(a, str) and same(a, b)
        check_oracle(metric, rows, q, k, a, [0, 23])
    rows = base.copy()
    rows[spots[-1], 3] = np.float32("nan")
    a, b = both_tiers(index(rows))
    assert isinstance(a, str) and "NaN" in a and a == b, (a, b)


# ------------------------------------------------------------------ the SPLIT layout (the store read in place, 4 ld bytes between rows)
@pytest.mark.parametrize("d,shape", [(64, "one_or_two"), (64, "three_ragged"), (64, "two_even"), (192, "one_or_two"), (192, "three_ragged")])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_split_rows_equal_f32_rows_and_the_oracle(vdb, metric, d, shape):
    rows, q256 = data(d, shape)
    a, b = [vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False) for _ in range(2)]
    for ix, mode in ((a, 0), (b, 2)):
        ix.set_split(mode)
        ix.add_bulk(rows)
    for k in (1, 10):
        for nq in (19, 256):
            q = q256[:nq]
            ra = a.search_batch_arrays(q, k)
            sa = a.last_stats()
            rb = b.search_batch_arrays(q, k)
            sb = b.last_stats()
            assert a.layout()[0] != SPLIT and b.layout()[0] == SPLIT
            assert sa["bf16_screen"] == 1 and sb["bf16_screen"] == 1
            assert same(ra, rb), (metric, d, shape, k, nq)        # ids, distance bits, counts
            check_oracle(metric, rows, q, k, rb, [0, nq - 1])


# ------------------------------------------------------------------ the sample instance (one tile per workgroup: C = 0 in its k-step 0)
def test_sample_pass_thresholds_with_and_without_the_compact_copy(vdb):
    """The SAMPLE instance over the compact bf16 copy against the f32 gather (set_sample_cache(False), a kernel of another
    file): the same thresholds, f32 bit for f32 bit, and the same results."""
    rows, q256 = data(128, "one_or_two")
    q, k = q256[:200], 10
    for metric in (0, 1, 2):
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
        ix.add_bulk(rows)
        for r in range(0, 5000, 11):
            ix.remove(r)
        ix.set_sample_cache(True)
        a = ix.search_batch_arrays(q, k)
        ta, sa = ix.debug_last_thresholds(len(q)), ix.last_stats()
        ix.set_sample_cache(False)
        b = ix.search_batch_arrays(q, k)
        tb, sb = ix.debug_last_thresholds(len(q)), ix.last_stats()
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), metric
        assert np.all(np.isfinite(ta))
        assert same(a, b)
        assert sa["bf16_screen"] == 1 and sa["sample_rows"] == sb["sample_rows"]
