"""The sparse index's lifecycle schedules without a GPU: the model against the reference adapter (two different routes to every
answer), every mutant of the reference adapter caught by a pinned schedule, and the edges the pinned set must contain."""
from collections import Counter

import pytest

import spv_lifecycle as L


@pytest.fixture(scope="module")
def models():
    return [L.run(t, L.RefIndex()) for t in L.pinned()]  # raises Mismatch where the two routes differ


def test_the_reference_adapter_passes_every_pinned_schedule(models):
    assert len(models) == len(L.pinned()) >= 12
    assert all(40 <= len(t["ops"]) <= 80 for t in L.pinned())


def test_the_pinned_schedules_contain_the_edges(models):
    cover = Counter()
    for m in models:
        cover.update(m.cover)
    for edge in ("regrow_rows", "regrow_nnz", "tail_upload", "masked_after_regrow", "masked_after_tail", "across_1024", "chunk_change",
                 "read_empty", "read_after_remove_all", "multi_chunk"):
        assert cover[edge] >= 1, (edge, dict(cover))
    assert any(m.cover["regrow_rows"] and m.first_flush[0] < L.FLOOR and m.first_flush[1] < L.FLOOR for m in models)
    assert 1 <= cover["nan_reads"] <= cover["reads"] // 10              # NaN-raising reads: at most one in ten
    kinds = Counter(op[0] for t in L.pinned() for op in t["ops"])
    assert all(kinds[k] for k in ("bulk", "empty", "nan", "remove", "flush", "remove_all", "cap", "read", "reread"))
    bulks = [op for t in L.pinned() for op in t["ops"] if op[0] == "bulk"]
    assert any(op[2][0] == "perm" and op[2][2] > 1000 for op in bulks) and any(len(set(op[2])) < len(op[2]) for op in bulks if op[2][0] != "perm")
    assert any(op[4] is not None for op in bulks)
    reads = [op for t in L.pinned() for op in t["ops"] if op[0] == "read"]
    assert {"mask", "compiled"} <= {op[4][0] for op in reads if op[4]} and any(isinstance(op[3], tuple) for op in reads)


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_every_mutant_is_caught(defect):
    caught = 0
    for t in L.pinned():
        try:
            L.run(t, L.RefIndex(defect))
        except L.Mismatch:
            caught += 1
    assert caught >= 1, defect


def test_a_trace_is_plain_data_and_replays():
    t = L.pinned()[0]
    again = eval(repr(t))                                # printable: tuples, ints, strings, None
    assert again == t
    a, b = L.run(t, L.RefIndex()), L.run(again, L.RefIndex())
    assert a.stats() == b.stats() and a.cover == b.cover
