"""The pinned HNSW lifecycle schedules (tests/hnsw_lifecycle.py) on the MI355X: GpuHnswIndex plus a MetaTable against the model.
Every walk read is made twice -- through the device-resident walk (device_queries grows by the batch, host_redone stays 0), then
through the forced host traversal -- and both must equal the model to the bit; after every read vdb_hnsw_mirror_stats must equal
the model's eight predicted counters, capacities included, so a change of the mirror's growth rule fails here instead of silently
un-aiming the edge schedules.  A failure prints the shrunk trace as a literal."""
import time

import pytest

import hnsw_lifecycle as hl
from conftest import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def run_or_shrink(vdb, name, trace=None):
    trace = trace or hl.pinned(name)
    t0 = time.perf_counter()
    try:
        model, stats, walked = hl.run_gpu(vdb, trace, expected=hl.slots(name) if name in hl.PINNED else None)
    except (hl.Mismatch, AssertionError) as e:
        small = hl.shrink_gpu(vdb, trace) if isinstance(e, hl.Mismatch) else None
        raise AssertionError(f"[{name}] {e}\nshrunk: TRACE = {small!r}") from e
    print(f"[{name}] {len(trace['ops'])} ops, {walked} queries walked on the device, {time.perf_counter() - t0:.2f} s, "
          f"mirror_stats {dict(zip(hl.STAT_NAMES, stats))}")
    return trace, model, stats, walked


@pytest.mark.parametrize("name", [n for n in hl.PINNED if n not in hl.EDGES])
def test_a_pinned_schedule_equals_the_model_on_both_routes(vdb, name):
    trace, model, stats, walked = run_or_shrink(vdb, name)
    assert stats == model.mirror_stats()
    assert walked >= 30 and {"walk", "scan", "empty"} <= set(model.routes)
    assert stats[0] > stats[1] >= 3 and stats[4] >= 3, stats        # rebuilds for a mutation and for the id capacity, and scatters


@pytest.mark.parametrize("name", hl.EDGES)
def test_an_edge_schedule_reaches_its_edge_on_the_device(vdb, name):
    trace, model, stats, walked = run_or_shrink(vdb, name)
    hl.edge_conditions(name, stats, trace)                           # the device's own counters
    assert stats == model.mirror_stats()


# add() keeps the Vector it stored on the Python side; a build_batch that names the id again must drop that copy, or get_vector
# answers with the vector the graph has replaced.
READD_IN_A_BATCH = {"seed": 7, "metric": 0, "d": 8, "m": 4, "efc": 40,
                    "ops": [("bulk", 1, 40, 0, ()), ("add", 40, 2), ("get_vector", 40), ("bulk", 3, 33, 41, ((5, 40),)),
                            ("get_vector", 40), ("search", 4, 1, 1, 8, (3, 33, 5)), ("graph",)]}


def test_get_vector_after_a_batch_replaced_an_added_id(vdb):
    trace, model, stats, walked = run_or_shrink(vdb, "re-add in a batch", READD_IN_A_BATCH)
    assert model.ver[40] == 2 and walked == 1
