"""Shared by test_numeric_filter_cpu.py and test_gpu_numeric_filter.py: filter_programs.py's metadata plus two numeric fields,
seeded random MetadataFilter trees over all seven leaf kinds, and a numpy interpreter of the postfix program with constants that
VectorStore.filter_program(flt, with_consts=True) emits (the restatement the device kernel of csrc/kernels_filter.hip is compared
with).  Not a test module."""
import os
import struct

import numpy as np

import filter_programs as fp
from filter_programs import AND, CONST, EQ, EXISTS, NE, OR  # noqa: F401

LT, LE, GT, GE = 16, 17, 18, 19
NUMERIC = (LT, LE, GT, GE)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "numeric_strings.tsv")

TINY = 5e-324                                                                 # the smallest subnormal
# score: floats with duplicates, +-0, subnormals and neighbours one ulp apart, as the strings repr() gives (they round-trip)
SCORE_VALUES = [0.0, -0.0, TINY, -TINY, 2.5e-310, 0.1, float(np.nextafter(0.1, 1.0)), float(np.nextafter(0.1, 0.0)), 1.0, float(np.nextafter(1.0, 2.0)),
                -1.0, 0.5, 0.5, 0.75, -2.25, 1e300, -1e300, 3.0, 9007199254740992.0]
SCORE_STRINGS = [repr(v) for v in SCORE_VALUES] + ["9007199254740993", "1e3", "+.5", "5."]
NON_NUMERIC = ["n/a", "", "1_0", "inf", "nan", "0x10", " 1"]


def fixture():
    """[(string, expected f64 bit pattern or None)] of tests/golden/numeric_strings.tsv"""
    out = []
    with open(FIXTURE, encoding="utf-8", newline="\n") as f:
        for line in f.read().split("\n"):
            if not line:
                continue
            s, want = line.rsplit("\t", 1)
            out.append((s, None if want == "-" else int(want, 16)))
    return out


def bits_of(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def random_price(rng):
    """integers 0..99 as decimal strings; 20 % missing (None), 5 % non-numeric"""
    r = rng.random()
    if r < 0.20:
        return None
    if r < 0.25:
        return NON_NUMERIC[int(rng.integers(0, len(NON_NUMERIC)))]
    return str(int(rng.integers(0, 100)))


def random_score(rng):
    r = rng.random()
    if r < 0.3:
        return None
    if r < 0.35:
        return NON_NUMERIC[int(rng.integers(0, len(NON_NUMERIC)))]
    return SCORE_STRINGS[int(rng.integers(0, len(SCORE_STRINGS)))]


def random_metadata(rng):
    md = fp.random_metadata(rng)
    for f, gen in (("price", random_price), ("score", random_score)):
        v = gen(rng)
        if v is not None:
            md[f] = v
    return md


def random_columns(rng, n):
    cols = fp.random_columns(rng, n)
    cols["price"] = np.array([random_price(rng) for _ in range(n)], dtype=object)
    cols["score"] = np.array([random_score(rng) for _ in range(n)], dtype=object)
    return cols


def random_constant(rng, field):
    r = rng.random()
    if r < 0.08:
        return [float("inf"), float("-inf"), 0.0, -0.0][int(rng.integers(0, 4))]
    if field == "price":
        return float(rng.integers(-2, 103)) + (0.5 if rng.random() < 0.2 else 0.0)
    v = SCORE_VALUES[int(rng.integers(0, len(SCORE_VALUES)))]
    if rng.random() < 0.3:
        v = float(np.nextafter(v, [np.inf, -np.inf][int(rng.integers(0, 2))]))
    return v


def random_leaf(F, rng):
    if rng.random() < 0.5:
        return fp.random_leaf(F, rng)
    r = rng.random()
    field = fp.ABSENT_FIELD if r < 0.08 else ("color" if r < 0.14 else ("price" if r < 0.6 else "score"))   # (color: a column without a number in it)
    make = [F.Lt, F.Le, F.Gt, F.Ge][int(rng.integers(0, 4))]
    return make(field, random_constant(rng, field if field in ("price", "score") else "price"))


def random_tree(F, rng, depth=4, budget=None):
    """filter_programs.random_tree over the seven leaf kinds: depth <= 4, at most 12 leaves, And / Or with 0..4 children"""
    budget = budget if budget is not None else [12]
    if depth == 0 or budget[0] <= 1 or rng.random() < 0.25:
        budget[0] -= 1
        return random_leaf(F, rng)
    kids = []
    for _ in range(int(rng.integers(0, 5))):
        if budget[0] <= 0:
            break
        kids.append(random_tree(F, rng, depth - 1, budget))
    return F.And(kids) if rng.random() < 0.5 else F.Or(kids)


def is_leaf(f):
    return f.op not in ("and", "or")


def has_numeric(f):
    return f.op in ("lt", "le", "gt", "ge") if is_leaf(f) else any(has_numeric(g) for g in f.filters)


def random_trees(F, seed=11, count=300):
    rng = np.random.default_rng(seed)
    trees = [random_tree(F, rng) for _ in range(count)]
    kinds = set()

    def walk(f):
        if is_leaf(f):
            kinds.add(f.op)
        for g in f.filters:
            walk(g)
    for t in trees:
        walk(t)
    assert kinds == {"eq", "ne", "exists", "lt", "le", "gt", "ge"}
    return trees


def interpret(program, consts, columns, luts, present, bits):
    """The program over ids 0 .. bits-1 -> (mask words u64, popcount).  columns: {slot: int32 codes, ANY length}; an id at or above
    a column's length reads -1.  luts: {slot: f64 by code, ANY length, maybe absent}; a negative code and a code at or above the
    LUT's length read NaN, which fails all four comparisons.  Otherwise filter_programs.interpret."""
    consts = np.asarray(consts if consts is not None else [], dtype=np.float64)
    assert not np.isnan(consts).any() and consts.size <= 1024
    stack = []
    for op, slot, code in program:
        if op in (EQ, NE, EXISTS) or op in NUMERIC:
            col = np.full(bits, -1, dtype=np.int32)
            src = np.asarray(columns[slot], dtype=np.int32)[:bits]
            col[:src.size] = src
            if op in NUMERIC:
                assert 0 <= code < consts.size
                lut = np.asarray(luts.get(slot, []), dtype=np.float64)
                ok = (col >= 0) & (col.astype(np.int64) < lut.size)
                v = np.full(bits, np.nan)
                v[ok] = lut[col[ok]]
                c = consts[code]
                stack.append(v < c if op == LT else (v <= c if op == LE else (v > c if op == GT else v >= c)))
            else:
                stack.append(col == code if op == EQ else (col != code if op == NE else col >= 0))
        elif op == CONST:
            assert code in (0, 1)
            stack.append(np.full(bits, bool(code), dtype=bool))
        else:
            assert op in (AND, OR) and len(stack) >= 2
            a, b = stack.pop(), stack.pop()
            stack.append((a & b) if op == AND else (a | b))
        assert len(stack) <= 32
    assert len(stack) == 1
    pres = np.zeros(bits, dtype=bool)
    p = np.asarray(present, dtype=bool)[:bits]
    pres[:p.size] = p
    m = stack[0] & pres
    packed = np.zeros((bits + 63) // 64 * 8, dtype=np.uint8)
    pb = np.packbits(m, bitorder="little")
    packed[:pb.size] = pb
    return packed.view(np.uint64), int(m.sum())


def store_luts(st):
    """{slot: nums} of a VectorStore, for interpret()"""
    return {st._slots[k]: c.nums for k, c in st._cols.items()}


def build_store(vdb, st, rng, n_single=700, n_bulk=4300, add_rows=None):
    """n_single + n_bulk internal ids made by inserts, upserts, deletes and ONE bulk attach.  add_rows(first_id, n): puts the bulk
    range's vectors into the index behind st (None: the index needs none, a host store)."""
    M, V = vdb.Metadata, vdb.Vector
    made = 0
    names = []
    while made < n_single:
        if names and rng.random() < 0.15:                                     # an upsert: a new internal id, the old one goes
            name = names[int(rng.integers(0, len(names)))]
        else:
            name = f"v{len(names)}"
            names.append(name)
        st.insert_with_metadata(name, V([float(made), 1.0]), M(random_metadata(rng)))
        made += 1
        if made == n_single // 2:                                             # the bulk range in the middle of the single rows
            if add_rows is not None:
                add_rows(st._next_id, n_bulk)
            st.attach_bulk_metadata(n_bulk, random_columns(rng, n_bulk))
    for name in rng.choice(names, size=60, replace=False):
        st.delete(str(name))
    start = st._bulk[0][0]
    for i in rng.choice(n_bulk, size=300, replace=False):
        st.delete(str(start + int(i)))
    assert st._next_id == n_single + n_bulk
    return st
