"""The sparse-vector search's SELECT (csrc/kernels_spv.hip: the 4096-key buffer, spv_prune, the `bound` bookkeeping, the threshold)
with posting lists built to length, against the CSR reference (spv_data.search_csr): ids, order, distance bits and counts."""
import numpy as np
import pytest

import spv_data as S

pytestmark = pytest.mark.gpu
U32, F32, U64 = np.uint32, np.float32, np.uint64


def from_lists(vdb, lists, n, seed=0, weight=None, ids=None):
    """an index of n rows in which posting list d holds exactly the rows lists[d]; gaussian weights, or weight(rows, d).
    Returns (index, C, view)."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.asarray(r, dtype=np.int64) for r in lists.values()])
    dims = np.concatenate([np.full(len(r), d, dtype=U32) for d, r in lists.items()])
    vals = np.concatenate([rng.standard_normal(len(r)).astype(F32) if weight is None else np.asarray(weight(np.asarray(r), d), F32)
                           for d, r in lists.items()])
    order = np.lexsort((-dims.astype(np.int64), rows))   # by row; indices descending inside a row (the index sorts on entry)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=n))
    if ids is None:
        ids = rng.permutation(n).astype(U64) * U64(5) + U64(11)
        ids[rng.choice(n, size=min(n, 7), replace=False)] += U64(1 << 32)
    ix = vdb.GpuSparseIndex()
    ix.add_csr(ids, offsets, dims[order], vals[order])
    C = (ids, offsets, dims[order], vals[order], np.ones(n, dtype=bool))
    return ix, C, S.csc_view(offsets, dims[order])


def q_of(dims, rng=None):
    dims = np.asarray(dims, dtype=U32)
    return (dims, np.ones(dims.size, F32) if rng is None else rng.standard_normal(dims.size).astype(F32))


FOUR = {d: np.arange(1024 * d, 1024 * (d + 1)) for d in range(4)}


@pytest.mark.parametrize("k", [1, 1023, 1024])
def test_exactly_4096_keys_and_one_more(vdb, k):
    """four rounds of 1024 fill the buffer to its cap without a prune (n = P = 4096 in the final sort); a fifth list of one row
    forces one prune at bound = 4096"""
    lists = dict(FOUR)
    lists[4] = [4096]
    lists[9] = np.arange(4090, 4200)                     # rows no query below reaches by this list
    ix, C, view = from_lists(vdb, lists, 4200, seed=k)
    S.check_csr(ix, C, [q_of([0, 1, 2, 3])], k, view=view)
    assert ix.stats()["candidates"] == 4096
    S.check_csr(ix, C, [q_of([4, 3, 2, 1, 0])], k, view=view)
    assert ix.stats()["candidates"] == 4097
    S.check_csr(ix, C, [q_of([4, 0, 1, 2, 3], np.random.default_rng(k))], k, view=view)


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_round_edges(vdb, k):
    """lists of 1023, 1025, 2048 and 2049 rows: rounds of 1023, 1024 + 1, 2 x 1024, 2 x 1024 + 1"""
    lens, lists, at = (1023, 1025, 2048, 2049), {}, 0
    for d, n in enumerate(lens):
        lists[d] = np.arange(at, at + n)
        at += n
    ix, C, view = from_lists(vdb, lists, at, seed=3)
    S.check_csr(ix, C, [q_of([0, 1, 2, 3]), q_of([3, 2]), q_of([1]), q_of([0, 2])], k, view=view)
    assert ix.stats()["candidates"] == sum(lens) + (2049 + 2048) + 1025 + (1023 + 2048)


def test_bound_above_the_fill(vdb):
    """the same 1024 rows in six lists: only the first list's round pushes keys, yet `bound` counts every round and reaches the cap;
    the prune then runs with n = 1024 keys, and with k = 10 further lists come after it under the threshold it set"""
    lists = {d: np.arange(1024) for d in range(6)}
    lists[6] = np.arange(1024, 3000)
    lists[7] = np.arange(2000, 4000)
    ix, C, view = from_lists(vdb, lists, 4000, seed=6)
    rng = np.random.default_rng(6)
    S.check_csr(ix, C, [q_of(range(6)), q_of(range(6), rng)], 1024, view=view)
    assert ix.stats()["candidates"] == 2048 and ix.stats()["entries_walked"] == 2 * 6 * 1024
    S.check_csr(ix, C, [q_of(range(8)), q_of(range(8), rng), q_of([7, 6, 0, 1, 2, 3, 4])], 10, view=view)
    S.check_csr(ix, C, [q_of(range(8), rng)], 1024, view=view)


def tie_ids(n):
    rng = np.random.default_rng(63)
    ids = rng.permutation(n).astype(U64) * U64(3) + U64(2)
    ids[rng.choice(n, size=40, replace=False)] += U64(1 << 32)
    ids[17] = U64((1 << 63) + 5)
    return ids


@pytest.mark.parametrize("weights", ["one", "signed_zeros", "zero_and_denormal"])
def test_ties_across_prune_rounds(vdb, weights):
    """6000 rows in one list with equal scores: the threshold of every prune decides between equal distances by id rank alone.
    signed_zeros: every second row stores -0.0, the others +0.0; the fold starts from +0.0, so both score +0.0 and every distance is
    -0.0 -- one tie group.  zero_and_denormal: every second row scores -2^-149 (distance +2^-149, behind), the others +0.0."""
    n = 6000
    ids = tie_ids(n)
    weight = {"one": lambda r, d: np.ones(r.size, F32),
              "signed_zeros": lambda r, d: np.where(r % 2 == 0, F32(-0.0), F32(0.0)),
              "zero_and_denormal": lambda r, d: np.where(r % 2 == 0, -S.DEN, F32(0.0))}[weights]
    ix, C, view = from_lists(vdb, {0: np.arange(n)}, n, weight=weight, ids=ids)
    q = [q_of([0])]
    small = np.sort(ids)
    for k in (1, 10, 1024):
        out_ids, out_d, _ = S.check_csr(ix, C, q, k, view=view)
        if weights != "zero_and_denormal":
            assert np.array_equal(out_ids[0], small[:k])
            assert (out_d[0].view(U32) == (0xbf800000 if weights == "one" else 0x80000000)).all()
    bits = int(small[n - 60]) + 1                        # the ids at and above 2^32 are beyond any mask
    eligible = (ids > small[499]) & (ids < bits)         # the mask strikes the 500 smallest ids
    mask = S.big_mask(ids, eligible, bits)
    for k in (1, 10, 1024):
        out_ids, _, _ = S.check_csr(ix, C, q, k, eligible, mask, bits, view=view)
        if weights != "zero_and_denormal":
            assert np.array_equal(out_ids[0], small[500:500 + k])


def test_all_candidates_masked_out_or_dead(vdb):
    lists = {0: np.arange(0, 3000), 1: np.arange(2500, 5000)}
    ids = np.arange(5000, dtype=U64) * U64(2) + U64(1)
    ix, C, view = from_lists(vdb, lists, 5000, ids=ids)
    q = [q_of([0, 1]), q_of([1])]
    S.check_csr(ix, C, q, 1024, view=view)
    walked = ix.stats()["entries_walked"]
    assert walked == 2 * 2500 + 3000
    none = np.zeros(5000, dtype=bool)
    for bits in (1, 64, 10001):                          # an empty mask, of one bit and of every id's
        out_ids, out_d, counts = S.check_csr(ix, C, q, 1024, none, np.zeros((bits + 63) // 64, dtype=U64), bits, view=view)
        st = ix.stats()
        assert not counts.any() and st["candidates"] == 0 and st["entries_walked"] == walked
    for i in ids[2500:]:
        ix.remove(int(i))                                # every row of list 1 is dead
    C = C[:4] + (np.arange(5000) < 2500,)
    _, _, counts = S.check_csr(ix, C, q, 1024, view=view)
    assert counts[1] == 0 and counts[0] == 1024 and ix.stats()["candidates"] == 2500


def test_per_query_k_inside_one_batch(vdb):
    lens, lists, at = (1023, 1025, 2048, 2049), {}, 0
    for d, n in enumerate(lens):
        lists[d] = np.arange(at, at + n)
        at += n
    ix, C, view = from_lists(vdb, lists, at, seed=8)
    rng = np.random.default_rng(8)
    empty = (np.zeros(0, U32), np.zeros(0, F32))
    absent = q_of([50, 4, 1 << 20])
    queries = [q_of([0, 1, 2, 3], rng), empty, q_of([3, 2], rng), absent, q_of([0, 1, 2, 3]), q_of([1], rng), q_of([2, 0], rng),
               q_of([3]), q_of([0, 1, 2, 3], rng), empty, q_of([0], rng)]
    ks = np.array([0, 5, 1, 7, 1024, 1023, 512, 2, 1024, 0, 1024], dtype=np.uintp)
    _, _, counts = S.check_csr(ix, C, queries, ks, view=view)
    assert counts.tolist() == [0, 0, 1, 0, 1024, 1023, 512, 2, 1024, 0, 1023]
    S.check_csr(ix, C, queries[::-1], ks[::-1].copy(), view=view)


@pytest.mark.parametrize("bits", [1, 63, 64, 65, 3001])
def test_mask_edges(vdb, bits):
    """ids mask_bits - 1 (the last one a mask can admit), mask_bits, and 2^32 + mask_bits - 1, whose low 32 bits name a set bit: the
    comparison id < mask_bits must refuse it.  Every bit of every word of the mask is set, those behind mask_bits included."""
    ids = np.array(sorted({0, bits // 2, bits - 1}) + [bits, bits + 1, (1 << 32) + bits - 1, (1 << 33) + 1, (1 << 63) + bits - 1], dtype=U64)
    n = ids.size
    ix, C, view = from_lists(vdb, {0: np.arange(n), 3: np.arange(0, n, 2)}, n, seed=bits, ids=ids)
    mask = np.full((bits + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=U64)
    eligible = ids < bits
    out_ids, _, counts = S.check_csr(ix, C, [q_of([0]), q_of([3, 0])], 1024, eligible, mask, bits, view=view)
    assert counts[0] == int(eligible.sum()) and (bits - 1) in out_ids[0, :counts[0]]
    half = mask.copy()
    half[(bits - 1) >> 6] &= ~(U64(1) << U64((bits - 1) & 63))      # ... and with that one bit cleared
    S.check_csr(ix, C, [q_of([0]), q_of([3, 0])], 1024, eligible & (ids != bits - 1), half, bits, view=view)
