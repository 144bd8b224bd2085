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
with the range reads that is about a fifth of the reads of these schedules.)"""
from collections import Counter

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


def test_the_old_schedules_do_not_move():
    import hashlib
    assert sorted(OLD_DIGESTS) == sorted(NAMES + LARGE_NAMES + STORE_NAMES) and len(OLD_DIGESTS) == 19
    got = {name: hashlib.sha256(repr(trace_of(name)).encode()).hexdigest()[:16] for name in OLD_DIGESTS}
    assert got == OLD_DIGESTS, {n: d for n, d in got.items() if d != OLD_DIGESTS[n]}
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
