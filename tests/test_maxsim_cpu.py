"""Late-interaction search without a GPU: the model of tests/maxsim_data.py is tied to the model of the search by group, and the
argument checks of vdb_flat_search_batch_maxsim answer in the contract's order before the handle is looked at."""
import ctypes

import numpy as np
import pytest

import distinct_data as dd
import maxsim_data as md
import range_data as rd
from conftest import load_package


@pytest.mark.parametrize("metric", md.METRICS)
def test_one_token_is_the_search_by_group_under_exists(metric):
    """T = 1 on tie-free rows: the documents and the score bits are search_distinct's groups and distance bits under EXISTS(field)"""
    n, dim, k = 1000, 33, 40
    rows = md.rows(n, dim)
    codes, _ = md.layout("mixed", n)
    toks = md.tokens(dim, (1, 1, 1))
    for b, (wc, ws) in enumerate(md.expected(metric, rows, codes, toks, k)):
        rank = rd.ranking(("maxsim cpu", b), metric, rows, toks[b][0], live=(codes >= 0).astype(np.uint8))
        _, ed, ec = dd.expected(rank, codes, k)
        assert len(wc) == k and np.array_equal(wc, ec) and np.array_equal(ws.view(np.uint32), ed.view(np.uint32))


def test_argument_checks_in_the_contracts_order_with_a_null_handle():
    vdb = load_package()
    vdb.build()
    L, bad = vdb._ffi.lib(), vdb._ffi.ERR_INVALID_ARGUMENT
    szp, fp, i32p = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)

    def call(offsets, n_codes, filtered, k=1, no_tokens=False):
        off, tok = np.asarray(offsets, dtype=np.uintp), np.zeros((64, 4), dtype=np.float32)
        oc, os_, cnt = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.uintp)
        head = (None, None if no_tokens else tok.ctypes.data_as(fp), off.ctypes.data_as(szp), off.size - 1, 4, None, k, None, 0, n_codes)
        tail = (1, oc.ctypes.data_as(i32p), os_.ctypes.data_as(fp), cnt.ctypes.data_as(szp))
        if filtered:
            rc = L.vdb_flat_search_batch_maxsim_filtered(*head, ctypes.c_void_p(16), *tail)   # (never dereferenced: the checks come first)
        else:
            rc = L.vdb_flat_search_batch_maxsim(*head, None, 0, *tail)
        return rc, vdb._ffi.last_error()[0]

    # the handle is NULL throughout: every refusal but the last names the ARGUMENT, so it came before the handle was looked at
    for filtered in (False, True):
        for args, word in ((dict(offsets=[0, 0], n_codes=0, no_tokens=True), "null argument"),       # (2) before (3) and (4)
                           (dict(offsets=[0, 1], n_codes=0, k=2), "kstride"),
                           (dict(offsets=[1, 2], n_codes=0), "offsets[0]"),
                           (dict(offsets=[0, 3, 2, 40], n_codes=0), "offsets decrease"),
                           (dict(offsets=[0, 3, 3], n_codes=0), "query 1 has 0 tokens"),               # (3) before (4)
                           (dict(offsets=[0, 32, 65], n_codes=0), "query 1 has 33 tokens"),
                           (dict(offsets=[0, 32], n_codes=0), "n_codes"),                              # (4)
                           (dict(offsets=[0, 32], n_codes=5), "null argument")):                       # ... and now the handle
            rc, msg = call(filtered=filtered, **args)
            assert rc == bad and word in msg, (args, msg)
    assert L.vdb_flat_maxsim_stats(None, (ctypes.c_uint64 * 8)()) == bad and L.vdb_flat_debug_set_maxsim_table_cap(None, 0) == bad
