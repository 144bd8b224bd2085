"""The screened route of late-interaction search (vdb_flat_set_maxsim_screen, csrc/kernels_maxsim_screen.hip):
the bf16 matrix cores rank, a certified lower bound L(q, c) <= score(c) says which documents the ranking cannot exclude, and only
those are scored exactly.  Every answer is compared, bit for bit, with the model of tests/maxsim_data.py and with the same call
under the switch off; vdb_flat_maxsim_stats [6] (queries the screened route answered) proves the route ran."""
import numpy as np
import pytest

import certificate_data as cd
import distinct_data as dd
import maxsim_data as md
from test_gpu_maxsim import make_index, make_table, setup, vdb  # noqa: F401  (vdb: the module fixture)

pytestmark = pytest.mark.gpu
F32, I32 = np.float32, np.int32


def on_off(ix, t, toks, k, n_codes, **kw):
    """the screened answer and its stats, after checking it against the plain route's bits"""
    ix.set_maxsim_screen(False)
    off = ix.search_batch_maxsim(toks, k, t, 0, n_codes, **kw)
    assert ix.maxsim_stats()[6:] == [0, 0]
    ix.set_maxsim_screen(True)
    on = ix.search_batch_maxsim(toks, k, t, 0, n_codes, **kw)
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[0], off[0]) and np.array_equal(on[1].view(np.uint32), off[1].view(np.uint32))
    return on, ix.maxsim_stats()


def run(ix, t, metric, rows, codes, n_codes, toks, k, ok=None, screened=None, chunks=1, what="", **kw):
    got, st = on_off(ix, t, toks, k, n_codes, **kw)
    md.check(got, md.expected(metric, rows, codes, toks, k, ok=ok), what)
    assert st[6] == (len(toks) if screened is None else screened) and st[2] == chunks, (what, st)
    return got, st


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("dim", [20, 64, 100])
@pytest.mark.parametrize("metric", md.METRICS)
def test_every_token_count_in_one_call_column_blocks_straddle_queries(vdb, metric, dim, n):
    rows, codes, n_codes, ix, t = setup(vdb, metric, n, dim, "mixed")
    run(ix, t, metric, rows, codes, n_codes, md.tokens(dim, tuple(range(1, 33))), 12, what=(metric, dim, n))


def bound_case(kind, metric, d):
    """(rows, token lists): a coherent worst-case family, or the mixed-scale kind cut to the norms the route serves (2^-40 .. 2^40)"""
    rng = np.random.default_rng(4190 + d)
    if kind in cd.FAMILIES:
        rows, q, _ = cd.coherent(kind, metric, d, 640, rng)
    else:
        rows, q = cd.make_case(kind, metric, rng, d)
        rn, qn = np.linalg.norm(rows.astype(np.float64), axis=1), np.linalg.norm(q.astype(np.float64), axis=1)
        rows, q = rows[(rn > 1e-11) & (rn < 1e11)][:640], q[(qn > 1e-11) & (qn < 1e11)][:16]
    return np.ascontiguousarray(rows), [np.ascontiguousarray(q[i:i + 4]) for i in range(0, len(q) - 3, 4)]


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("metric", md.METRICS)
@pytest.mark.parametrize("kind", list(cd.FAMILIES) + ["scales"])
def test_the_lower_bound_never_exceeds_the_exact_score(vdb, kind, metric, d):
    rows, toks = bound_case(kind, metric, d)
    codes = (np.arange(len(rows)) // 16).astype(I32)
    n_codes = int(codes.max()) + 1
    ix, t = make_index(vdb, metric, rows), make_table(vdb, codes)
    ix.set_maxsim_screen(True)
    ix.search_batch_maxsim(toks, 5, t, 0, n_codes)
    assert ix.maxsim_stats()[6] == len(toks) >= 1                              # (every bound below is a real one)
    L = ix.debug_maxsim_lower_bounds(len(toks), n_codes)
    for b, (wc, ws) in enumerate(md.expected(metric, rows, codes, toks, n_codes)):
        assert len(wc) == n_codes and not np.isnan(L[b]).any()
        bad = md.ordered(L[b, wc]) > md.ordered(ws)
        assert not bad.any(), (kind, metric, d, b, wc[bad], L[b, wc][bad], ws[bad])


@pytest.mark.parametrize("name", md.LAYOUTS)
def test_document_shapes_runs_across_tiles_per_query_k_and_k_above_the_documents(vdb, name):
    # (mixed: runs across the 64-row half tile at 60..69 and across the workgroup at 250..261, one document of 300 rows;
    #  1000 rows are no multiple of the 128-row tile, 33 no multiple of the K stage)
    rows, codes, n_codes, ix, t = setup(vdb, md.EUCLID, 1000, 33, name)
    run(ix, t, md.EUCLID, rows, codes, n_codes, md.tokens(33), np.array([3, 100, 1, 0, 17, 1024, 64]), what=name)


def test_masks_removed_rows_compact_and_a_mask_that_removes_a_best_row(vdb):
    n, metric = 1000, md.DOT
    rows, codes, n_codes, ix, t = setup(vdb, metric, n, 64, "mixed")
    toks = md.tokens(64, (4, 17, 32))
    ok = np.arange(n) % 3 != 1
    mask, bits = dd.id_mask(ok)
    run(ix, t, metric, rows, codes, n_codes, toks, 10, ok=ok, id_mask=mask, mask_bits=bits, what="host mask")
    t.set_codes(1, 0, (np.arange(n) % 3).astype(I32))
    with t.compile([(vdb.MetaTable.NE, 1, 1)], n) as cm:
        run(ix, t, metric, rows, codes, n_codes, toks, 10, ok=ok, compiled_mask=cm, what="compiled mask")
    (plain, _, _), _ = run(ix, t, metric, rows, codes, n_codes, toks, 10)
    members = np.nonzero(codes == int(plain[0, 0]))[0]                         # the winner's best row for token 0 goes
    ok = np.ones(n, dtype=bool)
    ok[members[np.argmin(md.distances(metric, rows, toks[0][:1], codes == plain[0, 0])[0, members])]] = False
    mask, bits = dd.id_mask(ok)
    run(ix, t, metric, rows, codes, n_codes, toks, 10, ok=ok, id_mask=mask, mask_bits=bits, what="best row masked")
    live = np.ones(n, dtype=bool)
    for i in list(range(0, n, 7)) + list(range(60, 70)) + list(range(310, 590)):
        ix.remove(i)
        live[i] = False
    run(ix, t, metric, rows, codes, n_codes, toks, 20, ok=live, what="removed")
    ix.compact()
    run(ix, t, metric, rows, codes, n_codes, toks, 20, ok=live, what="compacted")


def test_exact_duplicate_documents_tie_to_the_lower_code_at_the_kth_place(vdb):
    rows = md.rows(300, 20).copy()
    rows[208:224] = rows[96:112]                                               # document 13 is document 6 again
    rows, codes, n_codes, ix, t = setup(vdb, md.EUCLID, 300, 20, "adjacent", rows)
    (got, _, _), _ = run(ix, t, md.EUCLID, rows, codes, n_codes, [np.ascontiguousarray(rows[96:99] + F32(0.001), dtype=F32)], 1)
    assert got[0, 0] == 6                                                      # (13 has the same score and the same bound: k = 1 cuts between them)


def test_two_chunks_under_a_lowered_table_cap(vdb):
    rows, codes, n_codes, ix, t = setup(vdb, md.COSINE, 257, 33, "mixed")
    ix.debug_set_maxsim_table_cap(3 * n_codes * (32 * 4 + 8 + 1))              # (room for three queries with their bitmaps, not four)
    run(ix, t, md.COSINE, rows, codes, n_codes, md.tokens(33, (32, 1, 8, 17, 5)), 9, chunks=2, what="capped")


@pytest.mark.parametrize("metric", md.METRICS)
def test_fallbacks_a_tiny_token_an_inf_row_a_nan_row(vdb, metric):
    n, dim = 257, 20
    rows = md.rows(n, dim).copy()
    rows, codes, n_codes, ix, t = setup(vdb, metric, n, dim, "adjacent", rows)
    toks = md.tokens(dim, (3, 5, 2))
    toks[1][2] *= F32(1e-20) / np.linalg.norm(toks[1][2])                      # one token of norm 1e-20: its query alone falls back
    run(ix, t, metric, rows, codes, n_codes, toks, 6, screened=2, what="tiny token")
    rows[40, 0] = np.inf                                                       # every token meets the row: no query is screened
    ix, toks = make_index(vdb, metric, rows), md.tokens(dim, (3, 5))
    if metric == md.DOT:
        _, st = on_off(ix, t, toks, 6, n_codes)
        assert st[6] == 0 and st[7] == 0
    rows[40, 0] = np.nan
    ix = make_index(vdb, metric, rows)
    for on in (False, True):
        ix.set_maxsim_screen(on)
        with pytest.raises(vdb.VectorDbError if metric == md.COSINE else vdb.NanDistance):
            ix.search_batch_maxsim(toks, 6, t, 0, n_codes)


def test_pruning_on_clustered_documents_stays_under_a_cap_the_bound_itself_keeps(vdb):
    # 64 documents of 16 rows around far-apart centres, queries made of rows of one document each; cap: 4 k documents a query.
    # The bound in float64 (Euclid, lower-bound scores: certificate_data.cert_constants) keeps the candidates
    # {c : L(c) <= e_k} under it on its own -- a condition on the data, checked here on the CPU, not a measured number.
    rng = np.random.default_rng(419)
    d, docs, per, k = 64, 64, 16, 2
    centres = rng.standard_normal((docs, d))
    rows = (np.repeat(centres, per, axis=0) + 0.05 * rng.standard_normal((docs * per, d))).astype(F32)
    codes = (np.arange(docs * per) // per).astype(I32)
    toks = [np.ascontiguousarray(rows[per * c:per * c + 6] + F32(0.01)) for c in (3, 17, 40, 63)]
    want = md.expected(md.EUCLID, rows, codes, toks, docs)
    c = cd.cert_constants(md.EUCLID, d)
    R, nd = rows.astype(np.float64), np.linalg.norm(rows.astype(np.float64), axis=1)
    margin = np.maximum(c["m_e"] * np.linalg.norm(R - cd.bf16_rne(rows).astype(np.float64), axis=1) + c["m_n"] * nd, c["m_b"] * nd) * 1.000001
    for b, q in enumerate(toks):
        Q, Qb = q.astype(np.float64), cd.bf16_rne(q).astype(np.float64)
        qn = np.linalg.norm(Q, axis=1)[:, None]
        g = (qn * (1.00001 + c["ld"] * 1.2e-7) + c["kappa"] * np.linalg.norm(Q - Qb, axis=1)[:, None] * (1.0001 + c["ld"] * 1e-7)) * 1.00001
        s = nd ** 2 * (1 - c["eps"]) - 2 * Qb @ cd.bf16_rne(rows).astype(np.float64).T - g * margin          # [T, n] lower-bound scores
        s = s.reshape(len(q), docs, per).min(axis=2)
        lb = np.sqrt(np.maximum((s - np.abs(s) * 2.4e-7 + qn ** 2 * (1 - c["eps"])) / (1 + c["eps"]), 0)) * (1 - 1e-6)
        e_k = float(want[b][1][k - 1])
        assert int((lb.sum(axis=0) <= e_k).sum()) + k <= 4 * k, b
    ix, t = make_index(vdb, md.EUCLID, rows), make_table(vdb, codes)
    _, st = run(ix, t, md.EUCLID, rows, codes, docs, toks, k)
    assert st[7] <= len(toks) * 4 * k and st[3] < st[0] * len(rows), st
