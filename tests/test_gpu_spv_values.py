"""The sparse-vector search at the edges of f32 (spv_data.edge_corpus): denormal products and sums, overflow to +-inf, cancellation
that only the ascending fold reproduces, and every way to a NaN -- 0 * inf, inf - inf, a stored NaN, a NaN in the query, with
several payloads, the accumulators' own "untouched" pattern 0x7fffbeef among them.  Equal to spv_data.search_csr in ids, order,
distance bits and counts; a NaN is an error exactly when its row is eligible, and leaves no accumulator dirty."""
import numpy as np
import pytest

import spv_data as S

pytestmark = pytest.mark.gpu
U32, F32, U64 = np.uint32, np.float32, np.uint64


@pytest.fixture(scope="module")
def E():
    return S.edge_corpus()


def build(vdb, E):
    ix = vdb.GpuSparseIndex()
    ix.add_csr(E["ids"], E["offsets"], E["indices"], E["values"])
    return ix


def log(E, live=None):
    n = E["ids"].size
    return (E["ids"], E["offsets"], E["indices"], E["values"], np.ones(n, dtype=bool) if live is None else live)


def nan_rows(E, q):
    touched, s, _ = S.fold_csr(E["offsets"], E["indices"], E["values"], np.ones(E["ids"].size, dtype=bool), q)
    return touched & np.isnan(s)


BITS = 1 << 12                                           # above every small id of the corpus; the ids at and above 2^32 are beyond it


def test_finite_edges_bit_for_bit(vdb, E):
    ix = build(vdb, E)
    queries = [q for _, q, _ in E["finite"]]
    out_ids, out_d, counts = S.check_csr(ix, log(E), queries, 1024)
    for b, (name, _, want) in enumerate(E["finite"]):    # the rows the corpus names carry the distances it names: -score, bit for bit
        got = {int(i): int(d) for i, d in zip(out_ids[b, :counts[b]], out_d[b, :counts[b]].view(U32))}
        for r, bits in want.items():
            d = (-np.array([bits], U32).view(F32)).view(U32)[0]
            assert got[int(E["ids"][E["row"][r]])] == d, (name, r)
    fold = out_d[0, :counts[0]]
    assert fold[0] == -np.inf and fold[-1] == np.inf     # +-inf scores are ordinary answers, first and last
    den = -np.array([2.0 ** -140, 2.0 ** -126 + 2.0 ** -130 + 2.0 ** -140], F32)
    assert np.isin(den.view(U32), fold.view(U32)).all()  # denormals are not flushed: product, intermediate sum
    S.check_csr(ix, log(E), queries, np.array([3, 1, 1024, 1], dtype=np.uintp))


def test_every_nan_raises_when_eligible_and_is_silent_when_hidden(vdb, E):
    ix = build(vdb, E)
    ids = E["ids"]
    tame = E["finite"][0][1]
    for name, q, bad in E["nan"]:
        hide = nan_rows(E, q)
        assert hide.any() and all(hide[E["row"][r]] for r in bad)
        with pytest.raises(vdb.NanDistance):
            ix.search_batch_arrays([q], 10)
        # straight after the error: the same slot, the same rows, masked out -- and a tame query -- equal the reference
        elig = ~hide & (ids < BITS)
        S.check_csr(ix, log(E), [q, tame], 10, elig, S.id_mask(ids, elig, BITS), BITS)
        with pytest.raises(vdb.NanDistance):             # in the middle of a batch
            ix.search_batch_arrays([tame, q, tame], np.array([5, 1, 5], dtype=np.uintp))
        S.check_csr(ix, log(E), [tame, tame, tame], 1024)
        if name.startswith("query_nan"):                 # the row itself is finite: the next fold over it must start from 0.0
            S.check_csr(ix, log(E), [(q[0], np.full(q[0].size, 2.0, F32))], 10)


def test_nan_rows_removed_are_silent_and_nothing_stays_dirty(vdb, E):
    ix, fresh = build(vdb, E), build(vdb, E)
    live = np.ones(E["ids"].size, dtype=bool)
    for name, q, bad in E["nan"]:
        with pytest.raises(vdb.NanDistance):
            ix.search_batch_arrays([q], 10)
        live &= ~nan_rows(E, q)
    for i in E["ids"][~live]:
        ix.remove(int(i))
        fresh.remove(int(i))
    queries = [q for _, q, _ in E["nan"]] + [q for _, q, _ in E["finite"]]
    got = S.check_csr(ix, log(E, live), queries, 1024)
    want = fresh.search_batch_arrays(queries, 1024)      # an index that never met a NaN
    assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
