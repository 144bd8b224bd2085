"""Shared by test_filter_program_cpu.py and test_gpu_device_filter.py: seeded random MetadataFilter trees, the metadata they run
over, and a numpy interpreter of the postfix program VectorStore.filter_program emits (the restatement the device kernel of
csrc/kernels_filter.hip is compared with).  Not a test module."""
import numpy as np

FIELDS = ["color", "size", "shape"]
VALUES = {"color": ["red", "green", "blue"], "size": ["s", "m", "l", "xl"], "shape": ["round", "square"]}
ABSENT_FIELD, ABSENT_VALUE = "weight", "nope"                     # a field no row has, a value no row has
EQ, NE, EXISTS, CONST, AND, OR = range(6)


def random_metadata(rng):
    """a row's fields: each of FIELDS present with its own probability, so every column has holes"""
    md = {}
    for f, p in zip(FIELDS, (0.8, 0.5, 0.3)):
        if rng.random() < p:
            md[f] = VALUES[f][int(rng.integers(0, len(VALUES[f])))]
    return md


def random_columns(rng, n):
    """{field: object array of n values / None} for attach_bulk_metadata, same distribution as random_metadata"""
    cols = {}
    for f, p in zip(FIELDS, (0.8, 0.5, 0.3)):
        v = np.array(VALUES[f], dtype=object)[rng.integers(0, len(VALUES[f]), n)]
        v[rng.random(n) >= p] = None
        cols[f] = v
    return cols


def random_leaf(F, rng):
    r = rng.random()
    field = ABSENT_FIELD if r < 0.1 else FIELDS[int(rng.integers(0, 3))]
    kind = int(rng.integers(0, 3))
    if kind == 2:
        return F.Exists(field)
    vals = VALUES.get(field, ["x"])
    value = ABSENT_VALUE if rng.random() < 0.15 else vals[int(rng.integers(0, len(vals)))]
    return F.Eq(field, value) if kind == 0 else F.Ne(field, value)


def random_tree(F, rng, depth=4, budget=None):
    """depth <= 4, at most 12 leaves; And / Or with 0..4 children (so empty ones occur)"""
    budget = budget if budget is not None else [12]
    if depth == 0 or budget[0] <= 1 or rng.random() < 0.25:
        budget[0] -= 1
        return random_leaf(F, rng)
    n = int(rng.integers(0, 5))
    kids = []
    for _ in range(n):
        if budget[0] <= 0:
            break
        kids.append(random_tree(F, rng, depth - 1, budget))
    return F.And(kids) if rng.random() < 0.5 else F.Or(kids)


def count_leaves(f):
    return 1 if f.op in ("eq", "ne", "exists") else sum(count_leaves(g) for g in f.filters)


def tree_depth(f):
    return 0 if f.op in ("eq", "ne", "exists") else 1 + max([tree_depth(g) for g in f.filters], default=0)


def random_trees(F, seed=7, count=300):
    rng = np.random.default_rng(seed)
    trees = [random_tree(F, rng) for _ in range(count)]
    assert all(count_leaves(t) <= 12 and tree_depth(t) <= 4 for t in trees)
    return trees


def interpret(program, columns, present, bits):
    """The program over ids 0 .. bits-1 -> (mask words u64, popcount).  columns: {slot: int32 codes, ANY length}; an id at or
    above a column's length reads -1.  present: bool array of any length (missing = absent).  Mirrors the kernel: a stack of
    verdicts, leaves push, AND / OR fold the two topmost; the result is ANDed with presence and packed LSB-first."""
    stack = []
    for op, slot, code in program:
        if op in (EQ, NE, EXISTS):
            col = np.full(bits, -1, dtype=np.int32)
            src = np.asarray(columns[slot], dtype=np.int32)[:bits]
            col[:src.size] = src
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


def store_columns(st):
    """{slot: codes} of a VectorStore, for interpret()"""
    return {st._slots[k]: c.codes for k, c in st._cols.items()}


def host_store(vdb):
    """a VectorStore over the Index trait with no device behind it: everything but the searches works"""
    class FakeIndex(vdb.Index):
        def __init__(self):
            self.rows = {}

        def add(self, id, vector):
            self.rows[id] = vector

        def remove(self, id):
            self.rows.pop(id, None)

        def search(self, query, k):
            return []

        def get_vector(self, id):
            return self.rows.get(id)

        def metric(self):
            return vdb.DistanceMetric.Euclidean

        def len(self):
            return len(self.rows)

    return vdb.VectorStore.with_index(FakeIndex())
