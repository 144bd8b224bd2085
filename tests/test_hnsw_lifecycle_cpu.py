"""The HNSW lifecycle model against its reference adapter and the adapter's mutants (tests/hnsw_lifecycle.py): no GPU.  The
pinned schedules must pass the unmutated adapter (which also pins the restated mirror rule against itself), catch every mutant,
hold the full (mutation, read) pair table and reach the capacity edges the three edge schedules are aimed at."""
import pytest

import hnsw_lifecycle as hl

NAMES = list(hl.PINNED)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_adapter_agrees_with_the_model(name):
    trace = hl.pinned(name)
    model = hl.run(trace, hl.MirrorRef(trace), expected=hl.slots(name))
    s = model.mirror_stats()
    assert s[1] + s[2] + s[3] == s[0] and s[0] >= 1
    assert "walk" in model.routes


@pytest.mark.parametrize("mutant", hl.MUTANTS, ids=lambda c: c.__name__)
def test_a_pinned_schedule_catches_the_mutant(mutant):
    """answers only (counters=False): the defect must show in what a read returns"""
    for name in list(hl.EDGES) + NAMES[:9]:                          # (tools/fuzz_hnsw.py --lifecycle --mutants prints the whole table)
        trace = hl.pinned(name)
        try:
            hl.run(trace, mutant(trace), expected=hl.slots(name), counters=False)
        except hl.Mismatch as e:
            print(f"{mutant.__name__}: caught by [{name}] {str(e).splitlines()[0]}")
            return
    raise AssertionError(f"{mutant.__name__} passes every pinned schedule")


def test_the_pair_table_is_complete():
    pairs = set()
    for name in NAMES:
        pairs |= hl.coverage(hl.pinned(name))["pairs"]
    missing = [(a, b) for a in hl.MUTATIONS for b in hl.READS if (a, b) not in pairs]
    assert not missing, missing


def test_both_re_add_kinds_occur_at_every_level_relation():
    seen = set()
    for name in NAMES:
        seen |= hl.coverage(hl.pinned(name))["readds"]
    want = {(kind, how) for kind in ("readd_present", "readd_removed") for how in ("drawn", "same", "lower", "higher")}
    assert want <= seen, sorted(want - seen)


def test_a_refused_sync_inside_a_mutation_is_a_mismatch_not_an_error():
    """the id equal to cap_ids is still dirty when a bulk build below it starts: the bulk's first sync is where the real rule
    rebuilds for the id capacity and where the mutant sends the id to the scatter"""
    g = hl._Gen(5, hl.EUCLID, 8, 4)
    g.base(250)
    cap = g.model.book.cap_ids
    g.add(cap)
    before = g.model.mirror_stats()[2]
    g.emit(("bulk", g.next_key(), 40, 250, ()))
    assert g.model.mirror_stats()[2] == before + 1
    g.emit(("search", g.next_key(), 1, 5, 8, None))
    trace = g.trace
    hl.run(trace, hl.MirrorRef(trace))
    with pytest.raises(hl.Mismatch, match="bulk: .*DeviceError"):
        hl.run(trace, hl.IdCapacityOffByOne(trace), counters=False)


@pytest.mark.parametrize("name", NAMES[:9])
def test_a_generated_schedule_holds_the_whole_table_and_every_route(name):
    cov = hl.coverage(hl.pinned(name))
    assert not [(a, b) for a in hl.MUTATIONS for b in hl.READS if (a, b) not in cov["pairs"]]
    assert all(cov["routes"].get(r, 0) >= 3 for r in ("walk", "scan", "empty")), cov["routes"]
    s = cov["stats"]
    assert s[0] > s[1] >= 3 and s[4] >= 3, s                        # rebuilds by mutation AND by capacity (the jumps), and scatters


@pytest.mark.parametrize("name", hl.EDGES)
def test_an_edge_schedule_reaches_its_edge(name):
    trace = hl.pinned(name)
    stats = hl.coverage(trace)["stats"]
    print(name, dict(zip(hl.STAT_NAMES, stats)))
    hl.edge_conditions(name, stats, trace)


def test_the_edge_ids_schedule_adds_the_three_ids_around_the_capacity():
    trace = hl.pinned("edge ids")
    cap = hl.GROW_PAD                                                # of the first rebuild: the empty graph's, ahead of the base's bulk build
    assert hl.coverage(dict(trace, ops=trace["ops"][:2]))["stats"][6] == cap
    added = [op[1] for op in trace["ops"] if op[0] == "add"]
    assert {cap - 1, cap, cap + 1} <= set(added)
    # the model rebuilds for exactly the id `cap`: one scatter per add before it, the rebuild at it
    upto = dict(trace, ops=trace["ops"][:[i for i, op in enumerate(trace["ops"]) if op[:2] == ("add", cap)][0]])
    assert hl.coverage(upto)["stats"][2] == 0
    upto["ops"] = trace["ops"][:len(upto["ops"]) + 2]
    assert hl.coverage(upto)["stats"][2] == 1


def test_the_edge_pool_schedule_fills_the_pool_exactly_before_it_overflows():
    trace = hl.pinned("edge pool")
    m = hl.Model(trace)
    left = []
    for op in trace["ops"]:
        if hl.is_read(op):
            if op[0] != "graph":
                m.read_sync()
                left.append((m.book.cap_upper - m.book.used, m.book.c[3]))
        else:
            name, args = hl.resolve(trace, op)
            getattr(m, name)(*args)
    assert (0, 0) in left and left[left.index((0, 0)) + 1][1] == 1, left[-8:]


def test_a_pasted_trace_replays_to_the_same_ops():
    trace = hl.pinned(NAMES[0])
    pasted = eval(repr(trace))                                       # what a failure prints is a Python literal
    assert pasted == trace and pasted is not trace
    hl.run(dict(pasted, ops=pasted["ops"][:40]), hl.MirrorRef(pasted))
    assert hl.PINNED[NAMES[0]]() == trace                            # and the generator deals the same ops again


def test_the_shrinker_reduces_a_failing_trace_to_one_that_still_fails():
    trace = hl.pinned(NAMES[0])
    small = hl.shrink(trace, lambda: hl.RemoveLeavesMirror(trace), counters=False)
    assert small is not None and len(small["ops"]) < len(trace["ops"]) // 2
    with pytest.raises(hl.Mismatch):
        hl.run(small, hl.RemoveLeavesMirror(small), counters=False)
    hl.run(small, hl.MirrorRef(small))
