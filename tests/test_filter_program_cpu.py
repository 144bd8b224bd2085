"""The postfix filter program (VectorStore.filter_program -> vdb_meta_compile) without a GPU: a numpy interpreter
of the program (tests/filter_programs.py), applied to the translator's output, must equal `_eval_filter` for every id and the
reference's per-row `MetadataFilter::matches` (src/storage.rs:60-71) for every live row."""
import numpy as np

import filter_programs as fp
from conftest import load_package


def _store(vdb):
    return fp.host_store(vdb)


def _filled_store(vdb, steps=1500):
    rng = np.random.default_rng(11)
    st = _store(vdb)
    for step in range(steps):
        st.insert_with_metadata(f"v{rng.integers(0, 500)}", vdb.Vector([float(step)]), vdb.Metadata(fp.random_metadata(rng)))   # collisions: upserts
        if rng.random() < 0.1:
            ids = st.list_ids()
            st.delete(ids[int(rng.integers(0, len(ids)))])
    return st


def _check(st, flt):
    prog = st.filter_program(flt)
    assert prog is not None
    want_mask, bits = st.compile_filter(flt)
    mask, count = fp.interpret(prog, fp.store_columns(st), st._present, bits)
    assert np.array_equal(mask, want_mask)
    # _eval_filter for every id, deleted ones included (the program before the presence AND)
    raw, _ = fp.interpret(prog, fp.store_columns(st), np.ones(bits, dtype=bool), bits)
    ev = st._eval_filter(flt, bits)
    assert np.array_equal(np.unpackbits(raw.view(np.uint8), bitorder="little")[:bits].astype(bool), ev)
    # per-row matches (storage.rs:60-71) over the live rows
    want_ids = sorted(i for i, md in st._metadata.items() if flt.matches(md))
    got_ids = np.flatnonzero(np.unpackbits(mask.view(np.uint8), bitorder="little")[:bits]).tolist()
    assert got_ids == want_ids and count == len(want_ids)


def test_random_trees_equal_eval_filter_and_per_row_matches():
    vdb = load_package()
    st = _filled_store(vdb)
    trees = fp.random_trees(vdb.MetadataFilter)
    assert len(trees) == 300
    ops = set()
    for t in trees:
        _check(st, t)
        ops |= {op for op, _, _ in st.filter_program(t)}
    assert ops == {fp.EQ, fp.NE, fp.EXISTS, fp.CONST, fp.AND, fp.OR}          # the trees reach every op
    F = vdb.MetadataFilter
    for t in (F.And([]), F.Or([]), F.Eq(fp.ABSENT_FIELD, "x"), F.Ne(fp.ABSENT_FIELD, "x"), F.Exists(fp.ABSENT_FIELD),
              F.Eq("color", fp.ABSENT_VALUE), F.Ne("color", fp.ABSENT_VALUE), F.And([F.Exists("size")]), F.Or([F.Or([])])):
        _check(st, t)
    assert st.filter_program(F.And([])) == [(fp.CONST, 0, 1)] and st.filter_program(F.Or([])) == [(fp.CONST, 0, 0)]
    assert st.filter_program(F.Ne(fp.ABSENT_FIELD, "x")) == [(fp.CONST, 0, 1)] and st.filter_program(F.Eq("color", fp.ABSENT_VALUE)) == [(fp.CONST, 0, 0)]
    a, b, c = F.Exists("color"), F.Exists("size"), F.Exists("shape")
    sa, sb, sc = (st._slots[k] for k in ("color", "size", "shape"))
    assert st.filter_program(F.And([a, b, c])) == [(fp.EXISTS, sa, 0), (fp.EXISTS, sb, 0), (fp.AND, 0, 0), (fp.EXISTS, sc, 0), (fp.AND, 0, 0)]   # a left fold


def test_reference_fixtures(known_answers):
    vdb = load_package()
    F = vdb.MetadataFilter
    for case in known_answers["filter"] + known_answers["batch_filter"]:
        st = _store(vdb)
        for sid, row in case["rows"].items():
            st.insert_with_metadata(sid, vdb.Vector(row), vdb.Metadata(case["meta"].get(sid, {})))
        f = case["filter"]
        assert f["op"] == "eq"
        flt = F.Eq(f["field"], f["value"])
        _check(st, flt)
        mask, _ = fp.interpret(st.filter_program(flt), fp.store_columns(st), st._present, max(st._next_id, 1))
        got = {st._internal_to_id[i] for i in range(st._next_id) if (int(mask[i >> 6]) >> (i & 63)) & 1}
        if "expect_id_set" in case:
            assert got == set(case["expect_id_set"]), case["src"]
        else:
            assert got == {i for ids in case["expect_ids"] for i in ids}, case["src"]


def test_program_limits():
    vdb = load_package()
    F, T = vdb.MetadataFilter, vdb.MetaTable
    st = _filled_store(vdb, 50)
    leaf = F.Exists("color")
    # n leaves in one Or: 2n - 1 ops
    assert len(st.filter_program(F.Or([leaf] * 512))) == 1023
    assert st.filter_program(F.Or([leaf] * 513)) is None                        # 1025 ops
    # nesting in the SECOND operand deepens the stack by one per level; in the first it does not

    def right_nested(levels):
        f = leaf
        for _ in range(levels):
            f = F.And([leaf, f])
        return f

    def left_nested(levels):
        f = leaf
        for _ in range(levels):
            f = F.And([f, leaf])
        return f

    def depth_of(prog):
        d = peak = 0
        for op, _, _ in prog:
            d += 1 if op < T.AND else -1
            peak = max(peak, d)
        assert d == 1
        return peak

    assert depth_of(st.filter_program(right_nested(31))) == 32
    assert st.filter_program(right_nested(32)) is None                          # depth 33
    assert depth_of(st.filter_program(left_nested(200))) == 2
    _check(st, right_nested(31))
    _check(st, left_nested(200))
    assert (T.MAX_OPS, T.MAX_DEPTH) == (1024, 32)


def test_compile_filter_is_unchanged():
    """compile_filter keeps its signature and its result: (uint64 words, bits) with bits = max(next id, 1), built from
    _eval_filter, the presence bitmap and packbits -- restated here independently."""
    vdb = load_package()
    F = vdb.MetadataFilter
    st = _filled_store(vdb, 700)
    for flt in (F.Eq("color", "red"), F.Ne("size", "m"), F.And([F.Exists("shape"), F.Or([F.Eq("color", "blue"), F.Ne("color", "nope")])])):
        mask, bits = st.compile_filter(flt)
        assert mask.dtype == np.uint64 and bits == st._next_id and mask.size == (bits + 63) // 64
        want = np.zeros(mask.size * 64, dtype=bool)
        for i, md in st._metadata.items():
            want[i] = flt.matches(md)
        assert np.array_equal(np.unpackbits(mask.view(np.uint8), bitorder="little").astype(bool), want)
    empty = _store(vdb)
    mask, bits = empty.compile_filter(F.And([]))
    assert bits == 1 and mask.tolist() == [0]
    assert not empty.device_filter()                                            # off by default
    empty.set_device_filter(True)                                               # not a GpuFlatIndex: a no-op
    assert not empty.device_filter()
