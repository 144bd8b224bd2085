"""The lifecycle schedules of tests/lifecycle.py can catch things -- proved without a GPU.

  * every pinned schedule passes against the reference adapter (the survivors as a fresh block, another path than the model's);
  * every mutant -- the reference adapter with ONE stale-state defect, modelled on a flag of the engine -- fails on the pinned set;
  * the pinned set covers every (mutation, first read after it) pair, both crossings of SMALL_N, capacity doublings, a shrink, a
    reset with another dimension, an auto-compaction and a compaction with staged rows;
  * the caps on the inputs: at most 15 % of the reads expect an error, no read kind is below 8 % of the reads, every answered
    read returns a row for some query.  (Counted on the traces, i.e. for a plain handle.  A sharded handle refuses every range
    read on top of that, 10-18 % of the reads, so the 15 % cap does NOT hold for the sharded runs of the same schedules.)

The grouped, recommend and numeric-filter reads (six index schedules NEW_PINNED, three store schedules NEW_STORE_PINNED) get
the same proofs further down: the 19 older traces have not moved (digests), the reference adapter passes, mutants 13-21 fall on
every new index schedule and 22 / 23 on the store schedules they apply to, every (mutation, first read) pair of the three new
read kinds with all twelve mutations, (numbers, r) for every r that can carry a numeric mask, two LUT regrows per schedule,
and the caps: the old three, at most a quarter of the grouped per-query answers empty, 80 % of the numeric masks keeping
5-95 % of the live rows, every recommend read striking or cutting an entry.  (A sharded handle refuses every grouped read too:
with the range reads that is about a fifth of the reads of these schedules.)

The MMR, per-group and recommend-by-best reads (TWELVE_PINNED, large-twelve, TWELVE_STORE_PINNED) get them once more at the end
of the file: the 19 + 9 + 3 older traces have not moved, the reference adapter passes with all three counter vectors, the
sharded reference refuses what the model says, mutants 24-34 fall on all six index schedules, a failing trace shrinks to at
most eight ops, every (mutation, first read) pair of the three kinds, and their caps with the model alone."""
from collections import Counter

import numpy as np
import pytest

import lifecycle as lc
from conftest import load_package

NAMES = [p[0] for p in lc.PINNED]
LARGE_NAMES = [p[0] for p in lc.LARGE_PINNED]
STORE_NAMES = [p[0] for p in lc.STORE_PINNED]
_TRACES = {}


def trace_of(name):
    if name not in _TRACES:
        _TRACES[name] = lc.store_pinned(name) if name in STORE_NAMES else lc.pinned(name)
    return _TRACES[name]


def caught_by(make, names):
    """the pinned schedules on which an adapter fails, with the first line of each failure"""
    out = {}
    for name in names:
        t = trace_of(name)
        try:
            lc.run(t, make(t), expected=lc.slots(name, t))
        except lc.Mismatch as e:
            out[name] = str(e).split("\n")[0]
    return out


# ------------------------------------------------------------------ the reference adapter passes; the caps on the answers
@pytest.mark.parametrize("name", NAMES + LARGE_NAMES)
def test_reference_adapter_passes(name):
    t = trace_of(name)
    empty = []

    def answered(step, op, model, args, got):
        if "error" not in got and not any(len(l[0]) for l in got["lists"]):
            empty.append((step, op))
    lc.run(t, lc.RefIndex(t["metric"]), expected=lc.slots(name, t), on_read=answered)
    assert not empty, empty                                          # every answered read returns a row for some query


@pytest.mark.parametrize("name", NAMES[:3])
def test_reference_adapter_refuses_range_when_sharded(name):
    t = trace_of(name)
    seen = Counter()
    lc.run(t, lc.RefIndex(t["metric"], sharded=True), expected=lc.slots(name, t), on_read=lambda s, op, m, a, got: seen.update([(op[0], "error" in got)]))
    assert seen[("range", True)] == sum(1 for op in t["ops"] if op[0] == "range") and not seen[("range", False)]


@pytest.mark.parametrize("name", STORE_NAMES)
def test_store_reference_passes(name):
    vdb = load_package()
    t = trace_of(name)
    empty, kinds = [], Counter()

    def answered(step, op, model, args, got):
        kinds[op[0]] += 1
        if "error" not in got and not any(len(l[0]) for l in got["lists"]):
            empty.append((step, op))
    lc.run(t, lc.StoreSim(vdb, lc.RefIndex(t["metric"])), expected=lc.slots(name, t), on_read=answered)
    assert not empty, empty
    assert set(kinds) == set(lc.STORE_READS) and min(kinds.values()) >= 0.08 * sum(kinds.values()), kinds


# ------------------------------------------------------------------ every mutant is caught
@pytest.mark.parametrize("number", sorted(lc.INDEX_MUTANTS))
def test_index_mutant_is_caught(number):
    mutant = lc.INDEX_MUTANTS[number]
    caught = caught_by(lambda t: mutant(t["metric"]), NAMES)
    print(number, mutant.__name__, len(caught), "of", len(NAMES), next(iter(caught.values()), None))
    assert caught, f"mutant {number} ({mutant.__doc__.strip()}) survives every pinned schedule"
    if number not in (7,):                                           # (7 needs the Cosine metric; every other one falls everywhere)
        assert len(caught) == len(NAMES), sorted(set(NAMES) - set(caught))
    else:
        assert set(caught) == {p[0] for p in lc.PINNED if p[3] == lc.COSINE}


@pytest.mark.parametrize("name", LARGE_NAMES)
def test_the_large_schedules_reach_the_screening_tier_and_catch_the_stale_copy(name):
    """d = 64 and more than 65 536 rows (the floor of the bf16 screen, its sample copy and the screened range route; above the
    issue's size cap, which contradicts its route list), the large-k floor 240 (113 + 192) rows passed as well; a read at n rows,
    a shrinking compaction, adds back to n rows and the same reads again: mutant 5 (a row copy keyed by the row count) falls."""
    t = trace_of(name)
    m = lc.Model(t["metric"])
    peak, collide = 0, []
    for op in t["ops"]:
        if lc.is_read(op):
            peak = max(peak, m.n_rows())
            lc.read_begins(t, op, m)
        else:
            lc.apply_mutation(t, op, m)
            if op[0] == "compact_shrink":
                collide.append(m.n_rows())
    assert t["d"] == 64 and 240 * (113 + 192) <= peak <= 80_000 and min(collide) >= lc.BF16_MIN_ROWS, (peak, collide)
    kinds = Counter(op[0] for op in t["ops"])
    assert kinds["range"] >= 8 and kinds["search"] >= 20 and len(t["ops"]) <= 100
    assert {(op[1], op[2]) for op in t["ops"] if op[0] == "set"} >= {(n, v) for n in ("shadow", "sample_cache", "screen", "large_k") for v in (0, 1)}
    caught = caught_by(lambda t: lc.SampleKeyCollision(t["metric"]), [name])
    assert caught, "the row-count collision above the floor does not catch mutant 5"


def test_store_mutant_is_caught():
    """11. the presence bit of a superseded internal id stays set: the pre-filtered search returns the old version"""
    vdb = load_package()
    caught = caught_by(lambda t: lc.StoreSim(vdb, lc.RefIndex(t["metric"]), stale_presence=True), STORE_NAMES)
    print(caught)
    assert len(caught) == len(STORE_NAMES), caught
    assert all("s_prefiltered" in v or "s_similar" in v or "s_within" in v or "s_distinct" in v for v in caught.values()), caught


# ------------------------------------------------------------------ coverage, from the traces alone
def test_coverage_of_the_pinned_set():
    covs = {name: lc.coverage(trace_of(name)) for name in NAMES}
    pairs = set().union(*(c["pairs"] for c in covs.values()))
    missing = [(m, r) for m in lc.MUTATIONS for r in lc.READS if (m, r) not in pairs]
    assert not missing, missing
    for name, c in covs.items():
        n = c["counts"]
        assert n["up"] >= 1 and n["down"] >= 1, (name, n)            # SMALL_N crossed in both directions
        assert n["doublings"] >= 3 and n["shrinks"] >= 1 and n["dim_resets"] >= 1, (name, n)
        assert n["auto_compactions"] >= 1 and n["compact_with_staged"] >= 1, (name, n)
        assert 150 <= len(trace_of(name)["ops"]) <= 250, (name, len(trace_of(name)["ops"]))


def test_sizes_stay_small():
    for name in NAMES:
        t = trace_of(name)
        m = lc.Model(t["metric"])
        peak, low, dims = 0, 10 ** 9, set()
        for op in t["ops"]:
            if lc.is_read(op):
                peak, low = max(peak, m.n_rows()), min(low, m.n_live())
                dims.add(m.d)
                m.uploaded()
            else:
                lc.apply_mutation(t, op, m)
            assert m.id_bound <= lc.ID_LIMIT
        assert lc.SMALL_N < peak <= 20_000 and low <= 1000, (name, peak, low)
        assert dims == {40, 64}, (name, dims)


def test_caps_on_the_inputs():
    for name in NAMES:
        c = lc.coverage(trace_of(name))
        reads = Counter(c["reads"])
        total = sum(reads.values())
        assert c["errors"] <= 0.15 * total, (name, c["errors"], total)
        assert set(reads) == set(lc.READS) and min(reads.values()) >= 0.08 * total, (name, reads)
        ops = trace_of(name)["ops"]
        for kind in lc.READS:                                        # every read kind draws its batch from {1, 8, 9, 40} ...
            assert {op[1] for op in ops if op[0] == kind} <= set(lc.BATCHES), (name, kind)
        assert {op[1] for op in ops if op[0] in lc.READS} == set(lc.BATCHES), name
        for kind in ("search", "masked", "sparse", "by_id", "distinct"):   # ... and k from {1, 10, 113, 300} or one k per query
            ks = [op[2] for op in ops if op[0] == kind]
            assert {k for k in ks if isinstance(k, int)} <= set(lc.KS), (name, kind)
        ks = [op[2] for op in ops if op[0] in ("search", "masked", "sparse", "by_id", "distinct")]
        assert {k for k in ks if isinstance(k, int)} == set(lc.KS) and any(isinstance(k, tuple) for k in ks), name
    for kind in lc.READS:                                            # ... all four of them over the pinned set
        assert {op[1] for n in NAMES for op in trace_of(n)["ops"] if op[0] == kind} == set(lc.BATCHES), kind
    cosine = [p[0] for p in lc.PINNED if p[3] == lc.COSINE]
    assert cosine and all(any(op[0] == "zero" for op in trace_of(n)["ops"]) for n in cosine)
    assert any(op[0] == "misfit" for n in NAMES for op in trace_of(n)["ops"])


# ------------------------------------------------------------------ grouped, recommend and numeric-filter reads (lifecycle.NEW_PINNED)
# The old schedules are dealt from one rng stream each: a digest of repr(trace), computed on the commit before the new read kinds
# came, says that none of them moved.
OLD_DIGESTS = {
    "even-euclid": "e3c25ab8794da1d6", "even-cosine": "61506c2cffa0b9a1", "even-dot": "638fe53dbd8255aa",
    "odd-euclid": "7545cbbbcc320b2c", "odd-cosine": "03901372ac228caf", "odd-dot": "3ab466341078dfe6",
    "misfit-euclid": "45c935e1dcec2e98", "misfit-cosine": "4766466f5468b25a", "misfit-dot": "89f09b990182f93a",
    "auto-euclid": "a1d30fa684078625", "auto-cosine": "db042d76e808a0e0", "auto-dot": "d6501246ae78ff2e",
    "large-euclid": "19f8ab73d25a6c64", "large-cosine": "ce8b5e3e9f7eeba7", "large-dot": "83bed28f1a60e808",
    "store-euclid-late": "74cb6a156f810aa7", "store-cosine-late": "05c2015431d3966e", "store-dot-early": "6dd6e11382a16081",
    "store-euclid-early": "65aa23185b83342d",
}
NEW_NAMES = [p[0] for p in lc.NEW_PINNED]
# the 9 + 3 schedules that came with the grouped / recommend / numeric reads and with the SPLIT layout: digests computed with the
# generator of the commit before MMR, per group and recommend by best became read kinds (lifecycle.TWELVE_PINNED)
NINE_DIGESTS = {
    "nine-euclid": "12397159a246d068", "nine-cosine": "e3c076a8a95bf529", "nine-dot": "3824bc828f55e8b1",
    "nine-auto-euclid": "8a375c4f6d468b01", "nine-auto-cosine": "83c43e4baaacb552", "nine-auto-dot": "6b687f90ba5fb2af",
    "store-numeric-early": "2fcaa6ee9548e37d", "store-numeric-late": "b073d66ac77e74be", "store-numeric-again": "a21f2b5f01728d1c",
    "split-adaptive-euclid": "b7a12e67c50c653b", "split-mode2-cosine": "a7de658198423643", "split-off-then-on-dot": "2624a8bd8d719f87",
}


def test_the_old_schedules_do_not_move():
    import hashlib
    assert sorted(OLD_DIGESTS) == sorted(NAMES + LARGE_NAMES + STORE_NAMES) and len(OLD_DIGESTS) == 19
    got = {name: hashlib.sha256(repr(trace_of(name)).encode()).hexdigest()[:16] for name in OLD_DIGESTS}
    assert got == OLD_DIGESTS, {n: d for n, d in got.items() if d != OLD_DIGESTS[n]}
    nine = {p[0]: lc.pinned(p[0]) for p in lc.NEW_PINNED}
    nine.update({p[0]: lc.store_pinned(p[0]) for p in lc.NEW_STORE_PINNED})
    nine.update({p[0]: lc.split_pinned(p[0]) for p in lc.SPLIT_PINNED})
    assert sorted(nine) == sorted(NINE_DIGESTS) and len(NINE_DIGESTS) == 12
    got = {name: hashlib.sha256(repr(t).encode()).hexdigest()[:16] for name, t in nine.items()}
    assert got == NINE_DIGESTS, {n: d for n, d in got.items() if d != NINE_DIGESTS[n]}
    assert lc.READS9 == lc.READS + ("grouped", "recommend", "numeric") and lc.MUTATIONS12 == lc.MUTATIONS + ("numbers",)
    assert lc.READS12 == lc.READS9 + ("mmr", "per_group", "best")
    assert not any(op[0] in lc.NEWER_READS + lc.NEWER_STORE_READS + ("near",) or op[:2] in (("set", "pg_cap"), ("set", "rb_route"))
                   for t in list(nine.values()) + [trace_of(n) for n in OLD_DIGESTS] for op in t["ops"])
    assert lc.READS == ("search", "masked", "sparse", "range", "by_id", "distinct") and len(lc.STORE_READS) == 6 and len(lc.STORE_FILTERS) == 6
    assert not any(op[0] in lc.NEW_READS or op[0] == "numbers" for n in NAMES + LARGE_NAMES for op in trace_of(n)["ops"])


@pytest.mark.parametrize("name", NEW_NAMES)
def test_reference_adapter_passes_the_nine_read_kinds(name):
    """the reference adapter passes, and the caps on the answers hold with the model alone: every answered read returns a row
    for some query; at most a quarter of the per-query answers of the grouped reads are empty; at least 80 % of the reads under
    a numeric mask keep between 5 % and 95 % of the live rows; every recommend read strikes an entry, or cuts one, for some request"""
    t = trace_of(name)
    empty, seen, idle = [], Counter(), []

    def answered(step, op, model, args, got):
        if "error" in got:
            return
        if not any(len(l[0]) for l in got["lists"]):
            empty.append((step, op))
        want = lc.slots(name, t)[step][2]
        if op[0] == "grouped":
            seen["grouped_answers"] += len(want["lists"])
            seen["grouped_empty"] += sum(1 for l in want["lists"] if not len(l[0]))
            for j, key in ((2, "scan"), (3, "fallback"), (4, "unfiltered")):
                seen[key] += want["gstats"][j]
        elif op[0] == "recommend" and not want["rstats"][1] and not want["cut"]:
            idle.append((step, op))
        if lc.carries_numeric(op) and op[0] != "grouped":
            ok = lc.mask_ok(args[-1], model.codes, model.present, model.numbers)
            share = int((model.alive & lc.ok_of_ids(ok, model.ids)).sum()) / model.n_live()
            seen["numeric_reads"] += 1
            seen["numeric_mid"] += 0.05 <= share <= 0.95
    lc.run(t, lc.RefIndex(t["metric"]), expected=lc.slots(name, t), on_read=answered)
    print(name, dict(seen))
    assert not empty, empty
    assert not idle, idle
    assert 4 * seen["grouped_empty"] <= seen["grouped_answers"], seen
    assert seen["numeric_reads"] >= 8 and seen["numeric_mid"] >= 0.8 * seen["numeric_reads"], seen
    assert seen["scan"] > 0 and seen["fallback"] > 0 and seen["unfiltered"] > 0, seen      # what the GPU runs must see the engine count


@pytest.mark.parametrize("name", NEW_NAMES[:2])
def test_reference_adapter_refuses_grouped_when_sharded(name):
    t = trace_of(name)
    seen = Counter()
    lc.run(t, lc.RefIndex(t["metric"], sharded=True), expected=lc.slots(name, t), on_read=lambda s, op, m, a, got: seen.update([(op[0], "error" in got)]))
    for kind in ("range", "grouped"):
        assert seen[(kind, True)] == sum(1 for op in t["ops"] if op[0] == kind) and not seen[(kind, False)]
    assert seen[("recommend", False)] > 0 and seen[("numeric", False)] > 0


# the schedules a new mutant must fall on: all six -- each holds the interleaving the mutant needs by construction (_Gen9.build)
NEW_APPLIES = {number: NEW_NAMES for number in lc.NEW_INDEX_MUTANTS}


@pytest.mark.parametrize("number", sorted(lc.NEW_INDEX_MUTANTS))
def test_new_index_mutant_is_caught(number):
    mutant = lc.NEW_INDEX_MUTANTS[number]
    caught = caught_by(lambda t: mutant(t["metric"]), NEW_NAMES)
    print(number, mutant.__name__, len(caught), "of", len(NEW_NAMES), caught)
    assert sorted(caught) == sorted(NEW_APPLIES[number]), sorted(set(NEW_APPLIES[number]) - set(caught))
    kinds = {13: ("grouped",), 14: ("grouped",), 15: ("grouped",), 16: ("recommend",), 17: ("recommend",), 18: ("recommend",)}.get(number)
    if kinds:                                                        # a grouped defect falls on a grouped read, a recommend defect on a recommend read
        assert all(any(f"('{k}'," in v for k in kinds) for v in caught.values()), caught
    else:                                                            # a LUT defect on a read under a numeric mask
        assert all("'numeric'" in v for v in caught.values()), caught


def test_coverage_of_the_nine_read_kinds():
    covs = {name: lc.coverage(trace_of(name)) for name in NEW_NAMES}
    pairs = set().union(*(c["pairs"] for c in covs.values()))
    missing = [(m, r) for m in lc.MUTATIONS12 for r in lc.NEW_READS if (m, r) not in pairs]
    assert not missing, missing
    after_numbers = set()                                            # (numbers, r) with the numeric mask IN that read
    for name in NEW_NAMES:
        ops = trace_of(name)["ops"]
        for a, b in zip(ops, ops[1:]):
            if a[0] == "numbers" and lc.is_read(b) and lc.carries_numeric(b):
                after_numbers.add(b[0])
    assert after_numbers == set(lc.NUMERIC_CARRIERS), after_numbers
    for name, c in covs.items():
        n = c["counts"]
        assert n["up"] >= 1 and n["down"] >= 1, (name, n)
        assert n["doublings"] >= 3 and n["shrinks"] >= 1 and n["dim_resets"] >= 1, (name, n)
        assert n["auto_compactions"] >= 1 and n["compact_with_staged"] >= 1 and n["regrows"] >= 2, (name, n)
        assert 150 <= len(trace_of(name)["ops"]) <= 250, (name, len(trace_of(name)["ops"]))
        assert trace_of(name)["numbers"] is True


def test_sizes_and_caps_of_the_nine_read_kinds():
    """the limits of the twelve old schedules; at most 15 % of the reads expect an error (counted on the traces, i.e. for a plain
    handle: a sharded handle refuses every range AND every grouped read on top, about a fifth of the reads), no kind below 8 %"""
    for name in NEW_NAMES:
        t = trace_of(name)
        m = lc.Model(t["metric"])
        peak, low, dims, codes_past_lut = 0, 10 ** 9, set(), 0
        for op in t["ops"]:
            if lc.is_read(op):
                peak, low = max(peak, m.n_rows()), min(low, m.n_live())
                dims.add(m.d)
                if m.numbers.size and lc.carries_numeric(op):
                    codes_past_lut += bool((m.codes[m.ids[m.alive].astype("int64")] >= m.numbers.size).any())
                m.uploaded()
            else:
                lc.apply_mutation(t, op, m)
            assert m.id_bound <= lc.ID_LIMIT
        assert lc.SMALL_N < peak <= 20_000 and low <= 1000, (name, peak, low)
        assert dims == {40, 64} and codes_past_lut >= 3, (name, dims, codes_past_lut)
        c = lc.coverage(t)
        reads = Counter(c["reads"])
        total = sum(reads.values())
        assert c["errors"] <= 0.15 * total, (name, c["errors"], total)
        assert set(reads) == set(lc.READS9) and min(reads.values()) >= 0.08 * total, (name, reads)
        ops = t["ops"]
        assert {op[1] for op in ops if op[0] in lc.NEW_READS} == set(lc.BATCHES), name
        ks = [op[2] for op in ops if op[0] in lc.NEW_READS]
        assert {k for k in ks if isinstance(k, int)} == set(lc.KS) | {lc.GROUPED_BIG_K} and any(isinstance(k, tuple) for k in ks), name
        forms = Counter(op[5] for op in ops if op[0] == "grouped")
        assert set(forms) == {"host", "compiled", "numeric"} and len({op[4] for op in ops if op[0] == "grouped"}) >= 3, (name, forms)
        assert any(op[0] == "recommend" and op[4] for op in ops), name                       # an absent example: VectorNotFound
    assert {op[4] for n in NEW_NAMES for op in trace_of(n)["ops"] if op[0] == "grouped"} == {1, 2, 3, 4, 5, 6}   # G, over the set
    cosine = [p[0] for p in lc.NEW_PINNED if p[3] == lc.COSINE]
    assert cosine and all(any(op[0] == "zero" for op in trace_of(n)["ops"]) for n in cosine)
    assert any(op[0] == "misfit" for n in NEW_NAMES for op in trace_of(n)["ops"])


def test_a_new_failure_shrinks():
    t = trace_of(NEW_NAMES[0])
    make = lambda: lc.RecommendFoldsOldRow(t["metric"])
    small = lc.shrink(t, make)
    assert small is not None and len(small["ops"]) <= 6, small and small["ops"]   # a bulk, an upsert, the recommend read (and little more)
    assert small["ops"][-1][0] == "recommend"
    with pytest.raises(lc.Mismatch):
        lc.run(small, make())
    lc.run(small, lc.RefIndex(t["metric"]))


NEW_STORE_NAMES = [p[0] for p in lc.NEW_STORE_PINNED]


def new_store_trace(name):
    if name not in _TRACES:
        _TRACES[name] = lc.store_pinned(name)
    return _TRACES[name]


@pytest.mark.parametrize("name", NEW_STORE_NAMES)
def test_store_reference_passes_with_numeric_fields(name):
    """StoreSim over RefIndex passes the store schedules of the numeric fields: s_with_filters stated as search_batch_prefiltered
    query by query, s_recommend as the host composition; every read kind keeps its 8 %, every answered read returns a row"""
    import ast
    vdb = load_package()
    t = new_store_trace(name)
    assert ast.literal_eval(repr(t)) == t and t["numeric"] is True                 # plain data, "-inf" included
    empty, kinds = [], Counter()

    def answered(step, op, model, args, got):
        kinds[op[0]] += 1
        if "error" not in got and not any(len(l[0]) for l in got["lists"]):
            empty.append((step, op))
    lc.run(t, lc.StoreSim(vdb, lc.RefIndex(t["metric"])), expected=lc.slots(name, t), on_read=answered)
    assert not empty, empty
    assert set(kinds) == set(lc.STORE_READS + lc.NEW_STORE_READS) and min(kinds.values()) >= 0.08 * sum(kinds.values()), kinds
    fields = [f for call in (c for op in t["ops"] if not lc.is_read(op) for c in lc.resolve_store(t, op)) if call[0] == "insert" for f in [call[1][2]]]
    ts = [f["ts"] for f in fields]
    assert len(set(ts)) >= 0.9 * len(ts) and set(lc.TS_SPECIAL) <= set(ts), (len(set(ts)), len(ts))   # the dictionary grows on nearly every insert
    assert 15 <= len({f["price"] for f in fields if "price" in f}) <= 20 and 0.15 < sum("price" not in f for f in fields) / len(fields) < 0.25
    used = {repr(op[4]) for op in t["ops"] if op[0] in ("s_prefiltered", "s_similar", "s_recommend", "s_distinct", "s_within")}
    assert used >= {repr(f) for f in lc.NUMERIC_STORE_FILTERS[len(lc.STORE_FILTERS):]}, used          # every numeric filter of the pool is drawn
    switches = [op[2] for op in t["ops"] if op[:2] == ("set", "device_filter")]
    assert switches == {"store-numeric-early": [1], "store-numeric-late": [1], "store-numeric-again": [1, 0, 1]}[name]


@pytest.mark.parametrize("lut,applies", [("stale_sent", ["store-numeric-again"]), ("bulk_only", NEW_STORE_NAMES)])
def test_store_lut_mutant_is_caught(lut, applies):
    """22. _lut_sent survives set_device_filter(False) / (True): the new table never receives the old numbers (applies where the
    filter goes off and on again).  23. the numbers of new dictionary values are forwarded on a bulk attach only (everywhere)."""
    vdb = load_package()
    caught = {}
    for name in NEW_STORE_NAMES:
        t = new_store_trace(name)
        try:
            lc.run(t, lc.StoreSim(vdb, lc.RefIndex(t["metric"]), lut=lut), expected=lc.slots(name, t))
        except lc.Mismatch as e:
            caught[name] = str(e).split("\n")[0]
    print(lut, caught)
    assert sorted(caught) == sorted(applies), caught
    assert all(any(w in v for w in ("'lt'", "'le'", "'gt'", "'ge'", "s_with_filters")) for v in caught.values()), caught


def test_traces_are_plain_data_and_replay():
    import ast
    t = trace_of(NAMES[0])
    again = ast.literal_eval(repr(t))
    assert again == t and lc.pinned(NAMES[0]) == t                   # printed, parsed back, generated twice: the same trace
    short = dict(t, ops=t["ops"][:30])
    lc.run(ast.literal_eval(repr(short)), lc.RefIndex(t["metric"]))


def test_a_failure_names_its_trace_and_shrinks():
    t = trace_of(NAMES[0])
    with pytest.raises(lc.Mismatch) as e:
        lc.run(t, lc.ByIdGathersOldRow(t["metric"]))
    msg = str(e.value)
    assert f"seed {t['seed']}" in msg and "step " in msg and "TRACE = {" in msg
    import ast
    literal = ast.literal_eval(msg.split("TRACE = ", 1)[1])
    with pytest.raises(lc.Mismatch):
        lc.run(literal, lc.ByIdGathersOldRow(t["metric"]))          # the printed trace fails the same way
    assert len(literal["ops"]) < len(t["ops"]) and literal["ops"] == t["ops"][:len(literal["ops"])]
    small = lc.shrink(literal, lambda: lc.ByIdGathersOldRow(t["metric"]))
    assert small is not None and len(small["ops"]) <= 4, small["ops"]   # a bulk, an upsert, the by-id read (and at most one more)
    with pytest.raises(lc.Mismatch):
        lc.run(small, lc.ByIdGathersOldRow(t["metric"]))
    lc.run(small, lc.RefIndex(t["metric"]))
    assert lc.shrink(literal, lambda: lc.RefIndex(t["metric"])) is None


# ------------------------------------------------------------------ the SPLIT row layout (lifecycle.SPLIT_PINNED)
SPLIT_NAMES = [p[0] for p in lc.SPLIT_PINNED]
_SPLIT = {}


def split_trace(name):
    if name not in _SPLIT:
        _SPLIT[name] = lc.split_pinned(name)
    return _SPLIT[name]


def test_the_split_schedules_do_not_move_the_others():
    assert lc.pinned(NAMES[0]) == trace_of(NAMES[0]) and lc.split_pinned(SPLIT_NAMES[0]) == split_trace(SPLIT_NAMES[0])


@pytest.mark.parametrize("name", SPLIT_NAMES)
def test_split_reference_passes(name):
    """the reference adapter with the layout rule inside, behind LayoutChecked: every read equals the model, the layouts agree
    after every call, and the schedule holds what the issue asks of it"""
    t = split_trace(name)
    ad = lc.LayoutChecked(lc.SplitRefIndex(t["metric"]))
    sizes = []
    m = lc.run(t, ad, expected=lc.slots(name, t), on_read=lambda step, op, model, args, got: sizes.append(model.n_rows()))
    rule = ad.tracker.rule
    assert rule.forward >= 5 and rule.back >= 5 and rule.refusals == 1 and rule.expect()[0] == lc.LAYOUT_SPLIT, vars(rule)
    kinds = Counter(op[0] for op in t["ops"])
    assert all(kinds[r] >= 3 for r in lc.READS9), kinds
    assert all(kinds[x] >= 1 for x in ("add", "upsert", "remove", "remove_many", "compact", "compact_shrink", "bulk", "inf")), kinds
    assert max(sizes) >= 240 * (113 + 192) and min(s for s in sizes[8:]) < lc.BF16_MIN_ROWS <= sizes[-1] and len(t["ops"]) <= 130
    assert ("set", "shadow", 1) not in t["ops"] and t["ops"][0][:2] == ("set", "split") and t["ops"][1] == ("set", "split_after", 2)
    assert m.counts["doublings"] >= 3 and m.counts["shrinks"] >= 1


@pytest.mark.parametrize("mutant", lc.SPLIT_MUTANTS)
def test_split_mutant_is_caught(mutant):
    """a by-id gather / a recommend fold that sees the bytes as they lie while the rows are SPLIT, an append written into SPLIT
    rows and then converted back, a refusal forgotten after a search: each falls on every one of the three schedules"""
    caught = {}
    for name in SPLIT_NAMES:
        t = split_trace(name)
        try:
            lc.run(t, lc.LayoutChecked(lc.SplitRefIndex(t["metric"], mutant=mutant)), expected=lc.slots(name, t))
        except lc.Mismatch as e:
            caught[name] = str(e).split("\n")[0]
    print(mutant, caught)
    assert set(caught) == set(SPLIT_NAMES), (mutant, caught)
    assert all(("layout after" in v) == (mutant == "refusal_forgotten") for v in caught.values()), caught


# ------------------------------------------------------------------ MMR, per-group and recommend-by-best reads (lifecycle.TWELVE_PINNED)
# The same proofs for the three composed reads: six index schedules, one short large one, two store schedules; mutants 24-34.
TWELVE_NAMES = [p[0] for p in lc.TWELVE_PINNED]
TWELVE_STORE_NAMES = [p[0] for p in lc.TWELVE_STORE_PINNED]


def twelve_trace(name):
    if name not in _TRACES:
        _TRACES[name] = lc.store_pinned(name) if name in TWELVE_STORE_NAMES else lc.pinned(name)
    return _TRACES[name]


def caught12(make, names):
    out = {}
    for name in names:
        t = twelve_trace(name)
        try:
            lc.run(t, make(t), expected=lc.slots(name, t))
        except lc.Mismatch as e:
            out[name] = str(e).split("\n")[0]
    return out


def reference_run12(name):
    """one index schedule against the reference adapter; what the caps need, counted from the MODEL's answers kept in slots()"""
    t = twelve_trace(name)
    empty, seen, sizes = [], Counter(), []
    stages, routes, caps_set = Counter(), set(), set()

    def answered(step, op, model, args, got):
        sizes.append((op[0], model.n_rows()))
        if "error" in got:
            return
        if not any(len(l[0]) for l in got["lists"]):
            empty.append((step, op))
        want = lc.slots(name, t)[step][2]
        if op[0] == "mmr":
            lam = args[3]
            seen["mmr_diverse"] += bool(np.min(lam) < 1)
            seen["mmr_moved"] += bool(np.min(lam) < 1 and want["moved"])
            seen["mmr_all_rows"] += len(args[0]) == 1 and args[2] == lc.MMR_MAX and want["mstats"][2] == lc.MMR_MAX
            seen["mmr_pairs"] += want["mstats"][3]
            assert not any(np.isnan(sc.view(np.float32)).any() for sc in want["scores"])
        elif op[0] == "per_group":
            seen["pg_reads"] += 1
            seen["pg_with_members"] += any(len(ids) > 1 for grp in want["groups"] for _, ids, _ in grp)
            seen["pg_deep"] += want["deep"] >= 1024
            seen["pg_filled"] += want["pstats"][1]
            seen["pg_giants_low_cap"] += want["pstats"][2] if model.pg_cap == lc.PG_LOW_CAP else 0
            caps_set.add(model.pg_cap)
        elif op[0] == "best":
            seen["best_requests"] += len(want["lists"])
            seen["best_empty"] += sum(1 for l in want["lists"] if not len(l[0]))
            assert any(len(p) >= 2 and len(n) >= 1 for p, n in zip(args[0], args[1])), (step, op)
            routes.add(model.rb_route)
            if model.rb_route == 0:
                stages.update(want["bstages"])
            seen["best_list_searches"] += want["bstats"][6]
    lc.run(t, lc.RefIndex(t["metric"]), expected=lc.slots(name, t), on_read=answered)
    print(name, dict(seen), dict(stages), routes, caps_set)
    assert not empty, empty                                          # every answered read returns a row
    # the caps the issue words for EVERY schedule
    assert seen["mmr_diverse"] >= 4 and 2 * seen["mmr_moved"] >= seen["mmr_diverse"] and seen["mmr_all_rows"] >= 1 and seen["mmr_pairs"] > 0, seen
    assert 5 * seen["pg_with_members"] >= 4 * seen["pg_reads"] and seen["pg_deep"] >= 1 and seen["pg_filled"] > 0, seen
    assert 4 * seen["best_empty"] <= seen["best_requests"] and seen["best_list_searches"] > 0, seen
    return t, seen, stages, routes, caps_set, sizes


@pytest.mark.parametrize("name", TWELVE_NAMES)
def test_reference_adapter_passes_the_twelve_read_kinds(name):
    """The reference adapter -- the naive greedy choice over the whole pair matrix, the host compositions of per group and of
    recommend by best -- passes: lists, score bits, group codes, sizes and members, dn bits and all three counter vectors.  The
    caps hold WITH THE MODEL ALONE (the answers kept in slots()), so that a passing GPU run cannot be vacuous: those of every
    schedule in reference_run12, here those of every INDEX schedule."""
    t, seen, stages, routes, caps_set, sizes = reference_run12(name)
    assert seen["mmr_diverse"] >= 6, seen
    assert seen["pg_giants_low_cap"] > 0 and caps_set == {0, lc.PG_LOW_CAP}, (seen, caps_set)
    assert stages[0] > 0 and stages[1] > 0 and stages[2] > 0 and routes == {0, 1, 2}, (stages, routes)


def test_the_large_twelve_schedule():
    """75 000 rows of d = 64, at most 40 ops, all three kinds before and after a compaction and a shrinking compaction refilled
    to the same row count (that the searches inside run on the bf16 screening tier is the engine's word: the GPU test), the
    MMR read at m = 1024 with B = 1, a per-group member beyond rank 1024, and the caps of every schedule with the model alone"""
    t, seen, stages, routes, caps_set, sizes = reference_run12("large-twelve")
    assert t["d"] == 64 and len(t["ops"]) <= 40 and all(n >= lc.BF16_MIN_ROWS for kind, n in sizes if kind in lc.NEWER_READS), sizes
    kinds = [op[0] for op in t["ops"]]
    for kind in lc.NEWER_READS:
        at = [i for i, op in enumerate(t["ops"]) if op[0] == kind and not (kind == "mmr" and op[4] == lc.MMR_MAX)]
        assert len(at) == 4 and at[1] < kinds.index("compact") < at[2] < kinds.index("compact_shrink") < at[3], (kind, at)
    assert [op[1:3] + op[4:5] for op in t["ops"] if op[0] == "mmr" and op[4] == lc.MMR_MAX] == [(1, 3, lc.MMR_MAX)]
    assert lc.LARGE_ROWS <= max(n for _, n in sizes) <= lc.LARGE_ROWS + 4           # (the single add and the upsert append a row each)
    c = lc.coverage(t)                                               # (of the old three: no error read at all; four read kinds, so no 8 % rule)
    assert c["errors"] == 0 and set(c["reads"]) == set(lc.NEWER_READS) | {"search"}, c


@pytest.mark.parametrize("name", TWELVE_NAMES[:2] + TWELVE_NAMES[3:4])          # (the fourth holds the misfit episode)
def test_reference_adapter_refuses_the_three_when_sharded(name):
    """the sharded reference refuses exactly the reads the model says: range, grouped and every read of the three new kinds
    (no read of these schedules meets an empty index, which MMR and per group would answer first)"""
    t = twelve_trace(name)
    seen = Counter()
    lc.run(t, lc.RefIndex(t["metric"], sharded=True), expected=lc.slots(name, t), on_read=lambda s, op, m, a, got: seen.update([(op[0], "error" in got)]))
    for kind in ("range", "grouped") + lc.NEWER_READS:
        assert seen[(kind, True)] == sum(1 for op in t["ops"] if op[0] == kind) > 0 and not seen[(kind, False)], (kind, seen)
    assert all(seen[(kind, False)] > 0 for kind in ("search", "masked", "by_id", "distinct", "recommend", "numeric")), seen


def test_the_order_of_the_checks_on_an_empty_or_sharded_index():
    """MMR and per group answer an EMPTY index with empty lists before they refuse a sharded handle; recommend by best refuses
    the sharded handle first (and names an absent example before the dimension mismatch and the zero-norm row on a plain one)"""
    q = np.ones((2, 8), dtype=np.float32)
    for cls in (lc.Model, lc.RefIndex):
        sharded = cls(lc.COSINE, sharded=True)
        assert [len(l[0]) for l in sharded.mmr(q, 3, 8, 0.5)["lists"]] == [0, 0] and sharded.per_group(q, 3, 2)["groups"] == [[], []]
        assert lc.capture(lambda: sharded.best([[5]], [[]], 3)) == {"error": ("Refused", None)}
        sharded.add_bulk(np.ones((4, 8), dtype=np.float32), np.arange(4))
        for call in (lambda: sharded.mmr(q, 3, 8, 0.5), lambda: sharded.per_group(q, 3, 2), lambda: sharded.best([[1]], [[]], 3)):
            assert lc.capture(call) == {"error": ("Refused", None)}
        plain = cls(lc.COSINE)
        assert lc.capture(lambda: plain.best([[5]], [[]], 3)) == {"error": ("VectorNotFound", 5)}
        plain.add_bulk(np.ones((4, 8), dtype=np.float32), np.arange(4))
        plain.add(9, np.zeros(8, dtype=np.float32))
        plain.add(10, np.ones(5, dtype=np.float32))
        assert lc.capture(lambda: plain.best([[1, 7]], [[6]], 3)) == {"error": ("VectorNotFound", 7)}
        assert lc.capture(lambda: plain.best([[1]], [[]], 3)) == {"error": ("DimensionMismatch", None)}
        plain.remove([10])
        for call in (lambda: plain.mmr(q, 3, 8, 0.5), lambda: plain.per_group(q, 3, 2), lambda: plain.best([[1]], [[]], 3)):
            assert lc.capture(call) == {"error": ("InvalidVector", None)}


MUTANT_KIND = {24: "best", 25: "best", 26: "best", 27: "best", 28: "best", 29: "mmr", 30: "mmr", 31: "per_group", 32: "per_group", 33: "per_group"}


@pytest.mark.parametrize("number", sorted(lc.TWELVE_INDEX_MUTANTS))
def test_twelve_index_mutant_is_caught(number):
    """every mutant falls on EVERY one of the six schedules, on a read of the kind whose state it spoils (34, the switches that
    revert at a re-allocation, on the counters of a per-group or a best read)"""
    mutant = lc.TWELVE_INDEX_MUTANTS[number]
    caught = caught12(lambda t: mutant(t["metric"]), TWELVE_NAMES)
    print(number, mutant.__name__, len(caught), "of", len(TWELVE_NAMES), caught)
    assert sorted(caught) == sorted(TWELVE_NAMES), sorted(set(TWELVE_NAMES) - set(caught))
    if number in MUTANT_KIND:
        assert all(f"('{MUTANT_KIND[number]}'," in v for v in caught.values()), caught
    else:
        assert all(("pstats" in v or "bstats" in v) for v in caught.values()), caught
    assert len(lc.TWELVE_INDEX_MUTANTS) >= 9 and min(lc.TWELVE_INDEX_MUTANTS) == 24
    assert all(sum(1 for k in MUTANT_KIND.values() if k == kind) >= 2 for kind in lc.NEWER_READS)


@pytest.mark.parametrize("number", [25, 30, 31])
def test_a_twelve_failure_shrinks(number):
    """a failing trace of a new mutant (one per kind) shrinks to at most eight ops that still fail it and pass the reference"""
    t = twelve_trace(TWELVE_NAMES[0])
    make = lambda: lc.TWELVE_INDEX_MUTANTS[number](t["metric"])
    small = lc.shrink(t, make)
    assert small is not None and len(small["ops"]) <= 8, small and small["ops"]
    assert small["ops"][-1][0] == MUTANT_KIND[number]
    with pytest.raises(lc.Mismatch):
        lc.run(small, make())
    lc.run(small, lc.RefIndex(t["metric"]))


def test_coverage_sizes_and_caps_of_the_twelve_read_kinds():
    covs = {name: lc.coverage(twelve_trace(name)) for name in TWELVE_NAMES}
    pairs = set().union(*(c["pairs"] for c in covs.values()))
    missing = [(m, r) for m in lc.MUTATIONS12 for r in lc.NEWER_READS if (m, r) not in pairs]
    assert not missing, missing
    for name, c in covs.items():
        t = twelve_trace(name)
        n, ops = c["counts"], t["ops"]
        assert n["up"] >= 1 and n["down"] >= 1, (name, n)
        assert n["doublings"] >= 3 and n["shrinks"] >= 1 and n["dim_resets"] >= 1, (name, n)
        assert n["auto_compactions"] >= 1 and n["compact_with_staged"] >= 1, (name, n)
        assert 150 <= len(ops) <= 300 and t["twelve"] is True, (name, len(ops))
        assert {op[0] for op in ops if not lc.is_read(op)} >= set(lc.MUTATIONS12) - {"remove_absent"} | {"near"}, name
        reads = Counter(c["reads"])
        total = sum(reads.values())
        assert c["errors"] <= 0.15 * total, (name, c["errors"], total)
        assert set(reads) == set(lc.READS12) and min(reads.values()) >= 0.08 * total, (name, reads)   # (the older cap, as it stands)
        m = lc.Model(t["metric"])
        peak, low, dims = 0, 10 ** 9, set()
        since = {}                                                   # switch -> counted mutations since it was set
        used = set()
        for op in ops:
            if lc.is_read(op):
                peak, low = max(peak, m.n_rows()), min(low, m.n_live())
                dims.add(m.d)
                for sw, kind in (("pg_cap", "per_group"), ("rb_route", "best")):
                    if op[0] == kind and sw in since and since[sw][1] >= 2:
                        used.add((sw, since[sw][0]))
                m.uploaded()
            else:
                lc.apply_mutation(t, op, m)
                if op[0] == "set" and op[1] in ("pg_cap", "rb_route"):
                    since[op[1]] = [op[2], 0]
                elif op[0] in lc.MUTATIONS12 or op[0] == "remove_many":
                    for v in since.values():
                        v[1] += 1
        assert lc.SMALL_N < peak <= 20_000 and low <= 1300, (name, peak, low)
        assert dims == {40, 64}, (name, dims)
        # both values of pg_cap and all three of rb_route, each read two mutations or more after it was set
        assert used == {("pg_cap", 0), ("pg_cap", lc.PG_LOW_CAP), ("rb_route", 0), ("rb_route", 1), ("rb_route", 2)}, (name, used)
        assert any(op[0] == "best" and op[4] for op in ops), name                               # an absent example: VectorNotFound
        codes = [i for i, op in enumerate(ops) if op[0] == "codes"]
        grouped_reads = [i for i, op in enumerate(ops) if op[0] in ("distinct", "per_group")]
        assert any(a < c_ < b for a in grouped_reads for b in grouped_reads for c_ in codes if c_ > 100), name   # set_codes late, between two such reads
    cosine = [p[0] for p in lc.TWELVE_PINNED if p[3] == lc.COSINE]
    assert cosine and all(any(op[0] == "zero" for op in twelve_trace(n)["ops"]) for n in cosine)
    assert any(op[0] == "misfit" for n in TWELVE_NAMES for op in twelve_trace(n)["ops"])
    assert {p[2] for p in lc.TWELVE_PINNED} == {"twelve", "twelve-auto"} and {lc.PROFILES[p]["d"] for p in ("twelve", "twelve-auto")} == {40, 64}


@pytest.mark.parametrize("name", TWELVE_STORE_NAMES)
def test_store_reference_passes_with_the_three_reads(name):
    """StoreSim over RefIndex passes the two store schedules of s_mmr, s_groups and s_recommend_best (with upserts, the filter
    pool, the device filter from the start and switched on mid-life, auto-compaction in one): every kind keeps its share,
    every answered read returns a row; a group header carries the field value and the size"""
    import ast
    vdb = load_package()
    t = twelve_trace(name)
    assert ast.literal_eval(repr(t)) == t and t["twelve"] is True and t["numeric"] is True
    empty, kinds, groups = [], Counter(), Counter()

    def answered(step, op, model, args, got):
        kinds[op[0]] += 1
        if "error" in got:
            return
        if not any(len(l[0]) for l in got["lists"]):
            empty.append((step, op))
        want = lc.slots(name, t)[step][2]                            # the MODEL's answer: the caps are conditions on it alone
        if op[0] == "s_groups":
            sizes = [b for s, b in want if str(s).startswith("#")]
            groups["reads"] += 1
            groups["reads_with_members"] += any(x > 1 for x in sizes)
            groups["none"] += sum(1 for s, _ in want if s == "#None")
        elif op[0] == "s_mmr":
            groups["mmr_diverse"] += args[2] < 1
            groups["mmr_moved"] += bool(args[2] < 1 and want["moved"])
        elif op[0] == "s_recommend_best":
            groups["best_requests"] += len(want)
            groups["best_empty"] += sum(1 for l in want if not l)
            assert any(len(p) >= 2 and len(n) >= 1 for p, n in args[0]), (step, op)
    lc.run(t, lc.StoreSim(vdb, lc.RefIndex(t["metric"])), expected=lc.slots(name, t), on_read=answered)
    print(name, dict(kinds), dict(groups))
    assert not empty, empty
    assert set(kinds) == set(lc.STORE_READS + lc.NEW_STORE_READS + lc.NEWER_STORE_READS) and min(kinds.values()) >= 0.08 * sum(kinds.values()), kinds
    assert 5 * groups["reads_with_members"] >= 4 * groups["reads"] and groups["none"] > 0, groups
    assert groups["mmr_diverse"] >= 6 and 2 * groups["mmr_moved"] >= groups["mmr_diverse"], groups
    assert 4 * groups["best_empty"] <= groups["best_requests"], groups
    switches = [op[2] for op in t["ops"] if op[:2] == ("set", "device_filter")]
    assert switches == [1] and (t["ops"][0][:2] == ("set", "device_filter")) == (name == "store-twelve-early")
    assert (t["auto"] > 0) == (name == "store-twelve-late") and sum(1 for op in t["ops"] if op[0] == "s_insert") >= 40


def test_store_mutant_is_caught_by_the_three_reads():
    """11 (the presence bit of a superseded internal id stays set) falls on both new store schedules"""
    vdb = load_package()
    caught = caught12(lambda t: lc.StoreSim(vdb, lc.RefIndex(t["metric"]), stale_presence=True), TWELVE_STORE_NAMES)
    print(caught)
    assert sorted(caught) == sorted(TWELVE_STORE_NAMES), caught


def test_twelve_traces_are_plain_data_and_replay():
    import ast
    name = TWELVE_NAMES[3]
    t = twelve_trace(name)
    again = ast.literal_eval(repr(t))
    assert again == t and lc.pinned(name) == t                      # printed, parsed back, generated twice: the same trace
    kept = lc.slots(name, t)
    fresh = [None] * len(t["ops"])
    lc.run(again, lc.RefIndex(t["metric"]), expected=fresh)          # the WHOLE printed trace, without the answers the generator kept
    compared = 0
    for step, (a, b) in enumerate(zip(kept, fresh)):                 # what the generator kept is what a replay materialises and computes:
        if a is not None and b is not None:                          # auto-compaction inside a redrawn read included (on from about op 60)
            assert a[0] == b[0] and repr(a[1]) == repr(b[1]) and lc.diff(a[2], b[2]) is None and lc.diff(b[2], a[2]) is None, step
            compared += 1
    assert compared >= 30 and t["profile"] == "twelve-auto", compared
