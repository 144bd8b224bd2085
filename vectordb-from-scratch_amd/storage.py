"""Host-side mirror of the reference's VectorStore (src/storage.rs:83-348): String id <-> internal
id maps, metadata, dimension enforcement, the metadata filter, and the batch drivers that call the
index.  Same names, argument meaning and error behaviour as the reference; `search_batch` hands the
whole batch to the index in one call (the hook SURVEY.md 8(b) describes)."""
import math
import re
import struct
from dataclasses import dataclass, field

import numpy as np

from .error import DimensionMismatch, VectorNotFound
from .hnsw import GpuHnswIndex
from .index import GROUP_NONE, GpuFlatIndex, Index, MetaTable
from .vector import DistanceMetric, Vector


@dataclass
class SearchResult:                                  # storage.rs:13-16
    id: str
    distance: float


class Metadata:                                      # storage.rs:19-42
    def __init__(self, fields=None):
        self._fields = dict(fields or {})

    def insert(self, key, value):
        self._fields[key] = value

    def get(self, key):
        return self._fields.get(key)

    def fields(self):
        return self._fields


_NUMERIC = re.compile(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")
NUMERIC_OPS = ("lt", "le", "gt", "ge")


def num(s):
    """The number of a metadata string, or None.  Metadata values stay strings (storage.rs:19-22); `s` is numeric iff ALL of it
    matches the ASCII grammar [+-]?([0-9]+(\\.[0-9]*)?|\\.[0-9]+)([eE][+-]?[0-9]+)? -- no whitespace, `_`, inf / nan, hex or
    non-ASCII digits -- and its correctly rounded binary64 value is finite; that value is its number.  So "1e400" has none,
    "1E-400" is 0.0, "-0" is -0.0, and an integer above 2^53 has the number it rounds to."""
    if not isinstance(s, str) or _NUMERIC.fullmatch(s) is None:
        return None
    v = float(s)                                     # (correctly rounded; the grammar is a subset of what float() takes)
    return v if math.isfinite(v) else None


def _bits(value):
    """the bit pattern of a binary64: what tells -0.0 from 0.0"""
    return struct.unpack("<Q", struct.pack("<d", value))[0]


class MetadataFilter:                                # storage.rs:45-71
    def __init__(self, op, field=None, value=None, filters=None):
        self.op, self.field, self.value, self.filters = op, field, value, filters or []

    # ---- numeric comparisons (no reference counterpart): the row has the field, its string is numeric (num), and
    # num(string) OP value holds as an IEEE comparison (-0.0 equals 0.0; value may be +-inf).  A row without the field or with
    # a non-numeric string matches none of the four.
    @staticmethod
    def _numeric(op, field, value):
        if isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{op}: the value must be a number, not a bool")
        try:
            value = float(value)
        except (TypeError, OverflowError) as e:
            raise ValueError(f"{op}: the value must be a number ({e})") from None
        if value != value:
            raise ValueError(f"{op}: the value must not be NaN")
        return MetadataFilter(op, field, value)

    @staticmethod
    def Lt(field, value):
        return MetadataFilter._numeric("lt", field, value)

    @staticmethod
    def Le(field, value):
        return MetadataFilter._numeric("le", field, value)

    @staticmethod
    def Gt(field, value):
        return MetadataFilter._numeric("gt", field, value)

    @staticmethod
    def Ge(field, value):
        return MetadataFilter._numeric("ge", field, value)

    @staticmethod
    def Eq(field, value):
        return MetadataFilter("eq", field, value)

    @staticmethod
    def Ne(field, value):
        return MetadataFilter("ne", field, value)

    @staticmethod
    def Exists(field):
        return MetadataFilter("exists", field)

    @staticmethod
    def And(filters):
        return MetadataFilter("and", filters=filters)

    @staticmethod
    def Or(filters):
        return MetadataFilter("or", filters=filters)

    def matches(self, metadata):                     # storage.rs:62-70
        if self.op == "eq":
            return metadata.get(self.field) == self.value and metadata.get(self.field) is not None
        if self.op == "ne":
            return metadata.get(self.field) != self.value
        if self.op == "exists":
            return metadata.get(self.field) is not None
        if self.op in NUMERIC_OPS:
            s = metadata.get(self.field)
            v = num(str(s)) if s is not None else None   # (str: the one encoding of _Column.code)
            if v is None:
                return False
            return {"lt": v < self.value, "le": v <= self.value, "gt": v > self.value, "ge": v >= self.value}[self.op]
        if self.op == "and":
            return all(f.matches(metadata) for f in self.filters)
        if self.op == "or":
            return any(f.matches(metadata) for f in self.filters)
        raise ValueError(self.op)


@dataclass
class BatchInsertItem:                               # storage.rs:74-79
    id: str
    vector: Vector
    metadata: Metadata = field(default_factory=Metadata)


class _Column:
    """One metadata field as a dictionary-encoded column over internal ids: codes[internal] = index into `values`
    (-1: the row has no such field).  What `HashMap<usize, Metadata>` (storage.rs:90) holds per row, transposed so that a
    filter over a million rows is a few numpy passes instead of a million dict lookups."""

    def __init__(self):
        self.codes = np.full(1024, -1, dtype=np.int32)
        self.values, self.code_of = [], {}
        self._nums = np.full(64, np.nan)                 # num(values[c]) by code, NaN = none; always at least one NaN behind the last code

    @property
    def nums(self):
        """f64, parallel to `values`: the number of each dictionary value (num), NaN where it has none"""
        return self._nums[:len(self.values)]

    def numbers_of(self, n):
        """num() of the field for internal ids below n: NaN for a row without the field or with a non-numeric string"""
        return self._nums[:len(self.values) + 1][self.view(n)]      # (code -1 indexes the NaN behind the last code)

    def _grow(self, n):
        if n > self.codes.size:
            new = np.full(max(n, 2 * self.codes.size), -1, dtype=np.int32)
            new[:self.codes.size] = self.codes
            self.codes = new

    def code(self, value, create=False):
        value = str(value)                               # Metadata is HashMap<String, String> (storage.rs:19-22): one encoding for set and set_range
        c = self.code_of.get(value)
        if c is None and create:
            c = self.code_of[value] = len(self.values)
            self.values.append(value)
            if c + 2 > self._nums.size:
                new = np.full(2 * self._nums.size, np.nan)
                new[:c] = self._nums[:c]
                self._nums = new
            v = num(value)
            self._nums[c] = np.nan if v is None else v
        return c

    def set(self, internal, value):
        self._grow(internal + 1)
        self.codes[internal] = self.code(value, create=True)

    def set_range(self, start, values):
        """values: a sequence of n strings (or None for 'no such field') for internal ids start .. start+n-1."""
        vals = np.asarray(values, dtype=object)
        self._grow(start + vals.size)
        uniq, inv = np.unique(np.where(vals == None, "", vals).astype(str), return_inverse=True)   # noqa: E711
        lut = np.array([self.code(u, create=True) for u in uniq], dtype=np.int32)
        codes = lut[inv]
        if (vals == None).any():                                                                  # noqa: E711
            codes = np.where(vals == None, -1, codes)                                             # noqa: E711
        self.codes[start:start + vals.size] = codes

    def view(self, n):
        self._grow(n)
        return self.codes[:n]


class VectorStore:
    """VectorStore<I: Index>  (storage.rs:83-95).  `VectorStore(metric)` builds the GPU flat index
    where the reference's `VectorStore::new` builds a FlatIndex (storage.rs:99-101)."""

    def __init__(self, metric=None, index=None, device=0, auto_compact=0.0):
        """auto_compact: dead-row fraction above which the GPU flat index reclaims removed rows by itself
        (GpuFlatIndex.set_auto_compact; 0 = never, compact() by hand)."""
        if index is None:
            index = GpuFlatIndex(DistanceMetric(metric), device=device)
        assert isinstance(index, Index)
        self._index = index
        if auto_compact:
            index.set_auto_compact(auto_compact)         # (an index without it raises AttributeError: nothing to pass it to)
        self._id_to_internal = {}
        self._internal_to_id = {}
        self._metadata = {}
        self._next_id = 0
        self._dimension = None
        # filter compilation: the metadata as dictionary-encoded columns + a presence bitmap, kept in
        # step with every insert / upsert / delete
        self._cols = {}
        self._present = np.zeros(1024, dtype=bool)
        self._bulk = []                                  # attach_bulk_metadata ranges: (first internal id, n, ids or None)
        # set_device_filter: the same columns resident on the index's GPU (a slot per field, in order of first appearance) and
        # filters compiled there; None = off, the default
        self._slots = {}
        self._table = None
        self._lut_sent = {}                              # field -> dictionary codes whose numbers the table has (MetaTable.set_numbers)

    @classmethod
    def with_index(cls, index):                      # storage.rs:118-127
        return cls(index=index)

    # ---- mutation
    def insert(self, id, vector):                    # storage.rs:130-132
        self.insert_with_metadata(id, vector, Metadata())

    def insert_with_metadata(self, id, vector, metadata):   # storage.rs:135-172
        id = str(id)
        dim = vector.dimension()
        if self._dimension is not None:
            if dim != self._dimension:
                raise DimensionMismatch(self._dimension, dim)
        else:
            self._dimension = dim
        old = self._id_to_internal.get(id)
        if old is None:
            old = self._bulk_internal(id)                # an id that names a bulk-attached row: the insert replaces that row
        if old is not None:
            self._index.remove(old)
            self._metadata.pop(old, None)
            self._internal_to_id.pop(old, None)
        internal = self._next_id
        self._next_id += 1
        self._index.add(internal, vector)
        self._id_to_internal[id] = internal
        self._internal_to_id[internal] = id
        self._metadata[internal] = metadata
        self._mark_present(internal, True)
        for key, value in metadata.fields().items():
            col = self._column(key)
            col.set(internal, value)
            if self._table is not None:
                self._table.set_codes(self._slots[key], internal, col.codes[internal:internal + 1])
                self._forward_numbers(key, col)
        if old is not None:
            self._mark_present(old, False)

    def insert_batch(self, items):                   # storage.rs:293-298
        for it in items:
            self.insert_with_metadata(it.id, it.vector, it.metadata)

    def delete(self, id):                            # storage.rs:175-192
        internal = self._id_to_internal.pop(id, None)
        if internal is None:
            internal = self._bulk_internal(id)
        if internal is None:
            raise VectorNotFound(id)
        v = self._index.get_vector(internal)
        if v is None:
            v = Vector([])
        self._internal_to_id.pop(internal, None)
        self._metadata.pop(internal, None)
        self._index.remove(internal)
        self._mark_present(internal, False)
        return v

    def compact(self):
        """Reclaim the index rows that upserts and deletes left behind (every upsert above is remove(old) + add(new), so a
        flat index on the GPU keeps one dead device row per upsert until this runs).  Internal ids do not change, so no map
        of the store does.  Returns the number of rows given back; 0 for an index that frees rows as it removes them.
        No reference counterpart (a HashMap-backed FlatIndex has nothing to reclaim); a write, like insert / delete."""
        compact = getattr(self._index, "compact", None)
        return int(compact()) if compact is not None else 0

    def set_sparse_filter(self, mode):
        """How pre-filtered searches (search_batch_prefiltered, the server's "prefilter": true) treat a selective filter.
        Flat index: 0 (default) every row is streamed, 1 only the eligible rows are scanned, 2 automatic
        (GpuFlatIndex.set_sparse_filter).  HNSW index: mode != 0 answers filters that leave at most 131072 nodes with an exact scan
        of those nodes instead of the walk (GpuHnswIndex.set_filter_scan).  An index without either setting ignores it."""
        mode = int(mode)
        if mode not in (0, 1, 2):
            raise ValueError(f"sparse filter mode must be 0, 1 or 2, not {mode}")
        flat = getattr(self._index, "set_sparse_filter", None)
        scan = getattr(self._index, "set_filter_scan", None)
        if flat is not None:
            flat(mode)
        elif scan is not None:
            scan(131072 if mode else 0)

    # ---- reads
    def _internal_of(self, id):
        """String id -> internal id, for inserted rows and for bulk-attached rows alike (None: unknown)."""
        internal = self._id_to_internal.get(id)
        return internal if internal is not None else self._bulk_internal(id)

    def _metadata_of(self, internal):
        """The row's Metadata (storage.rs:90): the stored object of an inserted row, or the columns of a bulk-attached row
        materialised on demand."""
        meta = self._metadata.get(internal)
        if meta is None and self._bulk_id(internal) is not None:
            meta = Metadata({k: c.values[c.codes[internal]] for k, c in self._cols.items()
                             if internal < c.codes.size and c.codes[internal] >= 0})
        return meta

    def get(self, id):                               # storage.rs:195-198
        internal = self._internal_of(id)
        return None if internal is None else self._index.get_vector(internal)

    def get_metadata(self, id):                      # storage.rs:201-204
        internal = self._internal_of(id)
        return None if internal is None else self._metadata_of(internal)

    def len(self):
        return self._index.len()

    def __len__(self):
        return self.len()

    def is_empty(self):
        return self._index.is_empty()

    def metric(self):
        return self._index.metric()

    def dimension(self):
        return self._dimension

    def index(self):
        return self._index

    def list_ids(self):
        out = list(self._id_to_internal)
        for start, n, ids, _ in self._bulk:
            live = np.nonzero(self._present[start:start + n])[0]
            out.extend(str(start + int(j)) if ids is None else ids[int(j)] for j in live)
        return out

    def _mark_present(self, internal, on):
        if internal >= self._present.size:
            new = np.zeros(max(internal + 1, 2 * self._present.size), dtype=bool)
            new[:self._present.size] = self._present
            self._present = new
        self._present[internal] = on
        if self._table is not None:
            self._table.set_present(internal, 1, on)

    def _column(self, key):
        """The column of field `key`, created (with the next slot) when the field appears for the first time."""
        col = self._cols.get(key)
        if col is None:
            col = self._cols[key] = _Column()
            self._slots[key] = len(self._slots)
        return col

    def _forward_numbers(self, key, col):
        """The numbers of the dictionary codes the device table has not seen yet (the LUT numeric leaves read), when the
        column's dictionary grew."""
        sent = self._lut_sent.get(key, 0)
        if len(col.values) > sent:
            self._table.set_numbers(self._slots[key], sent, col.nums[sent:])
            self._lut_sent[key] = len(col.values)

    def attach_bulk_metadata(self, n, columns, ids=None):
        """Register n rows that are ALREADY in the index under the next n internal ids (a bulk device load, a mapped
        vector file: persistence/mmap.rs has no id or metadata column) together with their metadata columns
        {field: sequence of n strings / None}.  String ids default to the decimal internal id.  The per-row
        `Metadata` objects of the reference (storage.rs:90) are materialised only when asked for (get_metadata)."""
        n = int(n)
        start = self._next_id
        if ids is not None and len(ids) != n:
            raise ValueError("ids must have n entries")
        # one id, one row: a bulk id that names a row already in the store would make upsert / delete act on the wrong one
        new_ids = [str(i) for i in ids] if ids is not None else None
        if new_ids is not None:
            if len(set(new_ids)) != n:
                raise ValueError("bulk ids must be distinct")
            clash = next((i for i in new_ids if self._internal_of(i) is not None), None)
        else:
            clash = next((i for i in self._id_to_internal if i.isdigit() and str(int(i)) == i and start <= int(i) < start + n), None)
            if clash is None:
                clash = next((i for s0, m, other, _ in self._bulk if other is not None
                              for i in other if i.isdigit() and str(int(i)) == i and start <= int(i) < start + n), None)
        if clash is not None:
            raise ValueError(f"bulk id {clash!r} is already in use")
        for key, values in columns.items():
            if len(values) != n:
                raise ValueError(f"column {key!r} must have n entries")
            col = self._column(key)
            col.set_range(start, values)
            if self._table is not None:
                self._table.set_codes(self._slots[key], start, col.codes[start:start + n])
                self._forward_numbers(key, col)
        self._mark_present(start + n - 1, False)                 # grow once
        self._present[start:start + n] = True
        if self._table is not None and n:
            self._table.set_present(start, n, True)
        self._bulk.append((start, n, new_ids, None if new_ids is None else {sid: start + j for j, sid in enumerate(new_ids)}))
        self._next_id += n
        if self._dimension is None and hasattr(self._index, "dim"):
            self._dimension = self._index.dim() or None
        return start

    def _bulk_id(self, internal):
        for start, n, ids, _ in self._bulk:
            if start <= internal < start + n:
                if not self._present[internal]:
                    return None
                return str(internal) if ids is None else ids[internal - start]
        return None

    def _bulk_internal(self, id):
        """Internal id of a LIVE bulk-attached row named `id` (None: no such row)."""
        id = str(id)
        for start, n, ids, lut in self._bulk:
            if ids is None:
                if id.isdigit() and str(int(id)) == id and start <= int(id) < start + n and self._present[int(id)]:
                    return int(id)
            else:
                internal = lut.get(id)
                if internal is not None and self._present[internal]:
                    return internal
        return None

    def _check_dim(self, query):
        if self._dimension is not None and query.dimension() != self._dimension:
            raise DimensionMismatch(self._dimension, query.dimension())

    def _map(self, index_results):
        out = []
        for internal, dist in index_results:         # storage.rs:234-242
            sid = self._internal_to_id.get(internal)
            if sid is None and self._bulk:
                sid = self._bulk_id(internal)
            if sid is not None:
                out.append(SearchResult(sid, float(dist)))
        return out

    # ---- search
    def search(self, query, k):                      # storage.rs:217-245
        if self.is_empty():
            return []
        self._check_dim(query)
        return self._map(self._index.search(query, k))

    def _post_filter(self, index_results, k, flt):   # storage.rs:272-287
        out = []
        for internal, dist in index_results:
            sid = self._internal_to_id.get(internal)
            if sid is None and self._bulk:
                sid = self._bulk_id(internal)             # rows registered by attach_bulk_metadata live in the columns only
            meta = self._metadata_of(internal) if sid is not None else None
            if sid is None or meta is None:
                continue
            if flt.matches(meta):
                out.append(SearchResult(sid, float(dist)))
                if len(out) == k:
                    break
        return out

    def search_with_filter(self, query, k, flt):     # storage.rs:249-290  (post-filter, 3x over-fetch)
        if self.is_empty():
            return []
        self._check_dim(query)
        fetch_k = min(max(k * 3, k), self.len())
        return self._post_filter(self._index.search(query, fetch_k), k, flt)

    def search_batch(self, queries):                 # storage.rs:302-310, one index call
        if self.is_empty():
            return [[] for _ in queries]
        for q, _ in queries:
            self._check_dim(q)
        return [self._map(r) for r in self._index.search_batch(list(queries))]

    def search_batch_with_filter(self, queries, flt):   # storage.rs:313-322
        if self.is_empty():
            return [[] for _ in queries]
        for q, _ in queries:
            self._check_dim(q)
        n = self.len()
        fetch = [(q, min(max(k * 3, k), n)) for q, k in queries]
        res = self._index.search_batch(fetch)
        return [self._post_filter(r, k, flt) for r, (_, k) in zip(res, queries)]

    # ---- BASELINE config 4: the filter compiled to a device bitmask applied BEFORE top-k.
    # The reference's post-filter result is always a prefix of this one.
    def _eval_filter(self, flt, n):
        """MetadataFilter::matches (storage.rs:60-71) for ALL internal ids below n at once: a bool array."""
        if flt.op in ("eq", "ne", "exists"):
            col = self._cols.get(flt.field)
            if col is None:                                       # nobody has the field: Eq / Exists never match, Ne always does
                return np.full(n, flt.op == "ne", dtype=bool)
            codes = col.view(n)
            if flt.op == "exists":
                return codes >= 0
            c = col.code(flt.value) if flt.value is not None else None
            if flt.op == "eq":
                return (codes == c) if c is not None else np.zeros(n, dtype=bool)
            return (codes != c) if c is not None else np.ones(n, dtype=bool)      # Ne: a missing field matches (storage.rs:65)
        if flt.op in NUMERIC_OPS:
            col = self._cols.get(flt.field)
            if col is None:                                       # nobody has the field
                return np.zeros(n, dtype=bool)
            v = col.numbers_of(n)                                 # NaN (no field, no number) fails all four comparisons
            return {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal}[flt.op](v, flt.value)
        if flt.op in ("and", "or"):
            acc = np.full(n, flt.op == "and", dtype=bool)          # all([]) is true, any([]) is false, like Rust's iterators
            for f in flt.filters:
                m = self._eval_filter(f, n)
                acc = (acc & m) if flt.op == "and" else (acc | m)
            return acc
        raise ValueError(flt.op)

    def compile_filter(self, flt):
        """The filter as the id bitmask the device applies before top-k (bit i of word i>>6 = internal id i eligible).
        Vectorised over the dictionary-encoded metadata columns: eq / ne / exists are one comparison of an int32 column,
        and / or combine bool arrays, the presence bitmap removes deleted and superseded ids, np.packbits packs."""
        bits = max(self._next_id, 1)
        m = self._eval_filter(flt, bits)
        pres = self._present[:bits] if self._present.size >= bits else np.concatenate([self._present, np.zeros(bits - self._present.size, dtype=bool)])
        m = m & pres
        words = (bits + 63) // 64
        packed = np.zeros(words * 8, dtype=np.uint8)
        pb = np.packbits(m, bitorder="little")
        packed[:pb.size] = pb
        return packed.view(np.uint64), bits

    # ---- the same mask compiled on the device from resident columns (include/vdb_flat.h vdb_meta_table)
    def set_device_filter(self, on=True):
        """on: keep the metadata columns and the presence bitmap resident on the index's GPU, forward every later insert /
        upsert / delete / bulk attach to them, and let search_batch_prefiltered compile its filter there (one kernel launch,
        nothing uploaded but the filter expression) instead of in numpy.  off (the default): free them.  Results are identical
        either way.  A GpuFlatIndex searches under the compiled mask where it is; a GpuHnswIndex ANDs it with the graph's presence
        on the device and walks (or, with set_sparse_filter, scans) under that (vdb_hnsw_search_batch_filtered).  A store over any
        other index ignores the setting."""
        if not isinstance(self._index, (GpuFlatIndex, GpuHnswIndex)):
            return
        if not on:
            table, self._table = self._table, None
            self._lut_sent = {}
            if table is not None:
                table.close()
            return
        if self._table is not None:
            return
        table = MetaTable(self._index._device)
        n = self._next_id
        for key, col in self._cols.items():
            table.set_codes(self._slots[key], 0, col.codes[:min(n, col.codes.size)])
            table.set_numbers(self._slots[key], 0, col.nums)
            self._lut_sent[key] = len(col.values)
        pres = self._present[:n]
        edges = np.flatnonzero(np.diff(np.concatenate(([False], pres, [False])).astype(np.int8)))   # the runs of present ids
        for a, b in zip(edges[0::2], edges[1::2]):
            table.set_present(int(a), int(b - a), True)
        self._table = table

    def device_filter(self):
        return self._table is not None

    def filter_program(self, flt, with_consts=False):
        """The filter as the postfix program vdb_meta_compile takes: a list of (op, slot, code), or None when it needs more
        than MetaTable.MAX_OPS ops or an evaluation stack deeper than MetaTable.MAX_DEPTH.  Everything that needs the
        dictionary is resolved here, exactly as _eval_filter does: a field nobody has and a value no row has become CONST
        (Eq / Exists 0, Ne 1), And([]) is CONST 1, Or([]) CONST 0, n-ary And / Or are left folds of the binary op.
        with_consts=True: (program, consts), what vdb_meta_compile_num takes -- a numeric leaf is (LT | LE | GT | GE, slot,
        index into consts), equal constants (by bit pattern) share an index, a field nobody has is CONST 0, and more than
        MetaTable.MAX_CONSTS distinct constants give None.  Without it the constants are dropped: a program with numeric leaves
        is then good for counting its ops only."""
        T = MetaTable
        prog = []
        consts, const_of = [], {}
        depth = peak = 0
        # iterative post-order walk (a filter may nest deeper than Python's recursion limit likes): ("visit", f) | ("emit", op)
        todo = [("visit", flt)]
        while todo:
            what, f = todo.pop()
            if what == "emit":
                prog.append((f, 0, 0))
                depth -= 1
            elif f.op in ("eq", "ne", "exists"):
                col = self._cols.get(f.field)
                c = None
                if col is not None and f.op != "exists":
                    c = col.code(f.value) if f.value is not None else None
                if col is None or (f.op != "exists" and c is None):
                    prog.append((T.CONST, 0, 1 if f.op == "ne" else 0))
                elif f.op == "exists":
                    prog.append((T.EXISTS, self._slots[f.field], 0))
                else:
                    prog.append((T.EQ if f.op == "eq" else T.NE, self._slots[f.field], c))
                depth += 1
            elif f.op in ("and", "or"):
                if not f.filters:
                    prog.append((T.CONST, 0, 1 if f.op == "and" else 0))
                    depth += 1
                else:
                    op = T.AND if f.op == "and" else T.OR
                    steps = [("visit", f.filters[0])]
                    for g in f.filters[1:]:
                        steps += [("visit", g), ("emit", op)]
                    todo.extend(reversed(steps))
            elif f.op in NUMERIC_OPS:                               # (behind the reference's five: they walk the code they always did)
                if f.field not in self._cols:
                    prog.append((T.CONST, 0, 0))
                else:
                    j = const_of.setdefault(_bits(f.value), len(consts))
                    if j == len(consts):
                        consts.append(f.value)
                        if len(consts) > T.MAX_CONSTS:
                            return None
                    prog.append(({"lt": T.LT, "le": T.LE, "gt": T.GT, "ge": T.GE}[f.op], self._slots[f.field], j))
                depth += 1
            else:
                raise ValueError(f.op)
            peak = max(peak, depth)
            if len(prog) > T.MAX_OPS or peak > T.MAX_DEPTH:
                return None
        return (prog, consts) if with_consts else prog

    def compile_filter_device(self, flt):
        """compile_filter on the device: a CompiledMask over max(next internal id, 1) bits, equal to compile_filter's word for
        word.  The call does not wait for the device; release() the mask after the last search that uses it.  None when the
        filter does not fit the program limits (filter_program)."""
        if self._table is None:
            raise ValueError("the device filter is off: set_device_filter(True) first")
        prog = self.filter_program(flt, with_consts=True)
        if prog is None:
            return None
        prog, consts = prog
        return self._table.compile(prog, max(self._next_id, 1), consts if consts else None)

    # ---- exact range search (GpuFlatIndex.range_search_batch; no reference counterpart)
    def search_within(self, query, radius, limit, flt=None):
        """Every stored vector whose distance d to `query` satisfies d <= radius, nearest first (ties by internal id), at most
        `limit` (1..2048) of them.  With flt the filter is applied BEFORE the radius, under the mask of compile_filter, like
        search_batch_prefiltered."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("search_within needs a GpuFlatIndex")
        if self.is_empty():
            return []
        self._check_dim(query)
        mask, bits = self.compile_filter(flt) if flt is not None else (None, 0)
        ids, dists, counts, _ = self._index.range_search_batch(query.data[None, :], float(radius), int(limit), id_mask=mask, mask_bits=bits)
        return self._map([(int(ids[0, i]), dists[0, i]) for i in range(int(counts[0]))])

    # ---- "what is near item X?" (GpuFlatIndex.search_batch_by_id; no reference counterpart)
    def search_similar(self, id, k, flt=None):
        """The k stored vectors nearest to the stored vector `id`, that vector itself left out, nearest first."""
        return self.search_similar_batch([id], k, flt)[0]

    def search_similar_batch(self, ids, k, flt=None):
        """search_similar for several ids in one device call; the vectors never leave the GPU.  An unknown id raises
        VectorNotFound.  flt is a PRE-filter (the mask of compile_filter, or the device filter when set_device_filter is on),
        as in search_batch_prefiltered: a filtered-out id may still be asked about, it is simply in nobody's answer."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("search_similar needs a GpuFlatIndex")
        internal = []
        for id in ids:
            i = self._internal_of(id)
            if i is None:
                raise VectorNotFound(id)
            internal.append(i)
        if not internal:
            return []
        q = np.asarray(internal, dtype=np.uint64)
        cm = self.compile_filter_device(flt) if flt is not None and self._table is not None else None
        if cm is not None:
            try:
                out_ids, dists, counts = self._index.search_batch_by_id(q, int(k), compiled_mask=cm)
            finally:
                cm.release()
        else:
            mask, bits = self.compile_filter(flt) if flt is not None else (None, 0)
            out_ids, dists, counts = self._index.search_batch_by_id(q, int(k), id_mask=mask, mask_bits=bits)
        return [self._map([(int(out_ids[b, i]), dists[b, i]) for i in range(int(counts[b]))]) for b in range(len(internal))]

    # ---- "more like these, less like those" (GpuFlatIndex.recommend_batch; no reference counterpart)
    def recommend(self, positive, negative, k, flt=None):
        """The k stored vectors nearest to the average of the stored vectors `positive`, pushed away from the average of
        `negative` (may be empty), the examples themselves left out, nearest first."""
        return self.recommend_batch([(positive, negative)], k, flt)[0]

    def recommend_batch(self, requests, k, flt=None):
        """recommend for several (positive ids, negative ids) pairs in one device call; the vectors never leave the GPU.  An
        unknown id raises VectorNotFound.  flt is a PRE-filter, as in search_similar_batch: a filtered-out id may still be an
        example, it is simply in nobody's answer."""
        return self._recommend_requests("recommend", requests, k, flt)

    def _recommend_requests(self, what, requests, k, flt):
        """recommend_batch and recommend_best_batch: the string ids to internal ids, the filter on its host or device path, the
        index call `what`_batch, the (id, distance) lists back under the callers' ids"""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError(what + " needs a GpuFlatIndex")
        call = getattr(self._index, what + "_batch")

        def internal(ids):
            out = []
            for id in ids:
                i = self._internal_of(id)
                if i is None:
                    raise VectorNotFound(id)
                out.append(i)
            return out

        pos, neg = [], []
        for p, n in requests:
            pos.append(internal(p))
            neg.append(internal(n))
        if not pos:
            return []
        cm = self.compile_filter_device(flt) if flt is not None and self._table is not None else None
        if cm is not None:
            try:
                res = call(pos, neg, int(k), compiled_mask=cm)
            finally:
                cm.release()
        else:
            mask, bits = self.compile_filter(flt) if flt is not None else (None, 0)
            res = call(pos, neg, int(k), id_mask=mask, mask_bits=bits)
        out_ids, dists, counts = res[0], res[1], res[-1]
        return [self._map([(int(out_ids[b, i]), dists[b, i]) for i in range(int(counts[b]))]) for b in range(len(pos))]

    # ---- "near any of these, nearer to none of those" (GpuFlatIndex.recommend_best_batch; no reference counterpart)
    def recommend_best(self, positive, negative, k, flt=None):
        """The k stored vectors nearest to ANY of the stored vectors `positive`, each scored by its nearest positive and left
        out when some vector of `negative` (may be empty) is at least as near; the examples themselves left out, nearest first."""
        return self.recommend_best_batch([(positive, negative)], k, flt)[0]

    def recommend_best_batch(self, requests, k, flt=None):
        """recommend_best for several (positive ids, negative ids) pairs in one device call; the vectors never leave the GPU.
        An unknown id raises VectorNotFound.  flt is a PRE-filter, as in recommend_batch: a filtered-out id may still be an
        example."""
        return self._recommend_requests("recommend_best", requests, k, flt)

    # ---- "like this item, on the side of what I liked" (GpuFlatIndex.discover_batch; no reference counterpart)
    def discover(self, target, pairs, k, flt=None):
        """The k stored vectors ranked first by how many of the (positive id, negative id) `pairs` they satisfy -- nearer to the
        positive than to the negative -- then by distance to the stored vector `target`; the target and the pair ids themselves
        left out.  Returns (results, ranks): the SearchResults with the distance from the target, and the satisfied pairs of each."""
        return self.discover_batch([(target, pairs)], k, flt)[0]

    def discover_batch(self, requests, k, flt=None):
        """discover for several (target id, pairs) requests in one device call; the vectors never leave the GPU.  An unknown id
        raises VectorNotFound.  flt is a PRE-filter, as in recommend_batch: a filtered-out id may still be an example."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("discover needs a GpuFlatIndex")

        def internal(id):
            i = self._internal_of(id)
            if i is None:
                raise VectorNotFound(id)
            return i

        targets, pairs = [], []
        for t, ps in requests:
            targets.append(internal(t))
            pairs.append([(internal(p), internal(n)) for p, n in ps])
        if not targets:
            return []
        cm = self.compile_filter_device(flt) if flt is not None and self._table is not None else None
        if cm is not None:
            try:
                out_ids, dists, ranks, counts = self._index.discover_batch(targets, pairs, int(k), compiled_mask=cm)
            finally:
                cm.release()
        else:
            mask, bits = self.compile_filter(flt) if flt is not None else (None, 0)
            out_ids, dists, ranks, counts = self._index.discover_batch(targets, pairs, int(k), id_mask=mask, mask_bits=bits)
        return [(self._map([(int(out_ids[b, i]), dists[b, i]) for i in range(int(counts[b]))]), [int(x) for x in ranks[b, :int(counts[b])]])
                for b in range(len(targets))]

    # ---- "k results that are not all the same thing" (GpuFlatIndex.search_batch_mmr; no reference counterpart)
    def search_mmr(self, query, k, lam=0.5, candidates=None, flt=None):
        """k stored vectors near `query` and apart from each other (maximal marginal relevance), in pick order: the nearest
        first, then whichever of the `candidates` nearest rows minimises lam * distance - (1 - lam) * (distance to the nearest
        row already picked)."""
        return self.search_mmr_batch([query], k, lam, candidates, flt)[0]

    def search_mmr_batch(self, queries, k, lam=0.5, candidates=None, flt=None):
        """search_mmr for several queries in one device call.  candidates defaults to min(max(4 k, 32), 1024).  flt is a
        PRE-filter exactly as in search_similar_batch: the candidates are the nearest rows that pass it."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("search_mmr needs a GpuFlatIndex")
        queries = list(queries)
        if not queries or self.is_empty():
            return [[] for _ in queries]
        for q in queries:
            self._check_dim(q)
        k = int(k)
        if candidates is None:
            candidates = min(max(4 * k, 32), 1024)
        qs = np.stack([q.data for q in queries]).astype(np.float32, copy=False)
        cm = self.compile_filter_device(flt) if flt is not None and self._table is not None else None
        if cm is not None:
            try:
                out_ids, dists, _, counts = self._index.search_batch_mmr(qs, k, int(candidates), lam, compiled_mask=cm)
            finally:
                cm.release()
        else:
            mask, bits = self.compile_filter(flt) if flt is not None else (None, 0)
            out_ids, dists, _, counts = self._index.search_batch_mmr(qs, k, int(candidates), lam, id_mask=mask, mask_bits=bits)
        return [self._map([(int(out_ids[b, i]), dists[b, i]) for i in range(int(counts[b]))]) for b in range(len(queries))]

    # ---- "the k nearest documents" (GpuFlatIndex.search_batch_distinct; no reference counterpart)
    def search_distinct(self, query, k, field, flt=None):
        """The k nearest GROUPS of rows that share a value of metadata field `field`, each represented by its nearest row,
        nearest first.  A row without the field is its own group (And an Exists(field) into flt to drop such rows)."""
        return self.search_distinct_batch([query], k, field, flt)[0]

    def search_distinct_batch(self, queries, k, field, flt=None):
        """search_distinct for several queries in one device call.  Needs the device table (set_device_filter(True)): the
        collapse reads the field's resident column.  flt is a PRE-filter, compiled on the device when it fits the program
        limits, else by compile_filter.  A field no row has leaves every row its own group: the plain search."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("search_distinct needs a GpuFlatIndex")
        if self._table is None:
            raise ValueError("the device filter is off: set_device_filter(True) first")
        queries = list(queries)
        if self.is_empty() or not queries:
            return [[] for _ in queries]
        for q in queries:
            self._check_dim(q)
        qs = np.stack([q.data for q in queries]).astype(np.float32)
        cm = self.compile_filter_device(flt) if flt is not None else None
        mask, bits = self.compile_filter(flt) if flt is not None and cm is None else (None, 0)
        try:
            if field not in self._cols:
                out_ids, dists, counts = self._index.search_batch_arrays(qs, int(k), id_mask=mask, mask_bits=bits, compiled_mask=cm)
            else:
                out_ids, dists, _, counts = self._index.search_batch_distinct(qs, int(k), self._table, self._slots[field], id_mask=mask,
                                                                              mask_bits=bits, compiled_mask=cm)
        finally:
            if cm is not None:
                cm.release()
        return [self._map([(int(out_ids[b, i]), dists[b, i]) for i in range(int(counts[b]))]) for b in range(len(queries))]

    # ---- "the best passages of the k nearest documents" (GpuFlatIndex.search_batch_per_group; no reference counterpart)
    def search_groups(self, query, k, field, group_size, flt=None):
        """The k nearest GROUPS of rows that share a value of metadata field `field`, nearest first, each with its up to
        group_size nearest rows: a list of (field value, [SearchResult, ...]).  A row without the field is its own group
        (value None, one member)."""
        return self.search_groups_batch([query], k, field, group_size, flt)[0]

    def search_groups_batch(self, queries, k, field, group_size, flt=None):
        """search_groups for several queries in one device call.  flt is a PRE-filter.  With the device filter on
        (set_device_filter(True)) the field's resident column is read and flt is compiled on the device when it fits the
        program limits, as search_distinct_batch does; with it off the field's column is sent up for this call alone and flt
        is compiled by compile_filter.  A field no row has leaves every row its own group: the plain search."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("search_groups needs a GpuFlatIndex")
        group_size = int(group_size)
        if not 1 <= group_size <= GpuFlatIndex.PER_GROUP_MAX_SIZE:
            raise ValueError(f"group_size must lie in [1, {GpuFlatIndex.PER_GROUP_MAX_SIZE}]")
        queries = list(queries)
        if self.is_empty() or not queries:
            return [[] for _ in queries]
        for q in queries:
            self._check_dim(q)
        qs = np.stack([q.data for q in queries]).astype(np.float32)
        cm = self.compile_filter_device(flt) if flt is not None and self._table is not None else None
        mask, bits = self.compile_filter(flt) if flt is not None and cm is None else (None, 0)
        col, own = self._cols.get(field), None
        try:
            if col is None:
                out_ids, dists, counts = self._index.search_batch_arrays(qs, int(k), id_mask=mask, mask_bits=bits, compiled_mask=cm)
                return [[(None, self._map([(int(out_ids[b, i]), dists[b, i])])) for i in range(int(counts[b]))] for b in range(len(queries))]
            table, slot = self._table, self._slots[field]
            if table is None:
                table = own = MetaTable(self._index._device)
                own.set_codes(0, 0, col.view(max(self._next_id, 1)))
                slot = 0
            out_ids, dists, codes, sizes, counts = self._index.search_batch_per_group(qs, int(k), group_size, table, slot, id_mask=mask,
                                                                                      mask_bits=bits, compiled_mask=cm)
        finally:
            if cm is not None:
                cm.release()
            if own is not None:
                own.close()
        out = []
        for b in range(len(queries)):
            groups = []
            for j in range(int(counts[b])):
                c = int(codes[b, j])
                members = self._map([(int(out_ids[b, j, m]), dists[b, j, m]) for m in range(int(sizes[b, j]))])
                groups.append((col.values[c] if c >= 0 else None, members))
            out.append(groups)
        return out

    def search_batch_prefiltered(self, queries, flt):
        if self.is_empty():
            return [[] for _ in queries]
        for q, _ in queries:
            self._check_dim(q)
        cm = self.compile_filter_device(flt) if self._table is not None else None
        if cm is not None:
            try:
                return [self._map(r) for r in self._index.search_batch(list(queries), compiled_mask=cm)]
            finally:
                cm.release()
        mask, bits = self.compile_filter(flt)
        return [self._map(r) for r in self._index.search_batch(list(queries), id_mask=mask, mask_bits=bits)]

    # ---- one batch, a filter per query (GpuFlatIndex.search_batch_grouped; no reference counterpart)
    @staticmethod
    def _filter_key(flt):
        """A hashable key equal for structurally equal filters (same ops, fields, values, order of children)."""
        done = []                                                  # keys of finished subtrees, a stack
        todo = [("visit", flt)]
        while todo:
            what, f = todo.pop()
            if what == "visit" and f.op in ("and", "or"):
                todo.append(("fold", f))
                todo.extend(("visit", g) for g in reversed(f.filters))
            elif what == "visit":
                v = _bits(f.value) if f.op in NUMERIC_OPS else f.value     # (-0.0 == 0.0 and hash alike: told apart by their bits)
                try:
                    hash(v)
                except TypeError:
                    v = repr(v)
                done.append((f.op, f.field, type(v).__name__, v))
            else:
                n = len(f.filters)
                kids = tuple(done[len(done) - n:]) if n else ()
                del done[len(done) - n:]
                done.append((f.op, kids))
        return done[0]

    def search_batch_with_filters(self, queries, filters):
        """search_batch_prefiltered with a filter PER QUERY: queries holds (Vector, k) pairs, filters[i] is the MetadataFilter of
        query i or None (no filter).  Structurally equal filters share one mask; all queries go to the device as ONE batch
        (GpuFlatIndex.search_batch_grouped).  The masks are compiled on the device when the device table is on and every
        program fits its limits, else by compile_filter.  Results equal search_batch_prefiltered([q], f) query by query."""
        if not isinstance(self._index, GpuFlatIndex):
            raise ValueError("search_batch_with_filters needs a GpuFlatIndex")
        queries, filters = list(queries), list(filters)
        if len(filters) != len(queries):
            raise ValueError(f"{len(queries)} queries but {len(filters)} filters")
        if self.is_empty() or not queries:
            return [[] for _ in queries]
        for q, _ in queries:
            self._check_dim(q)
        group_of, distinct, seen = [], [], {}
        for f in filters:
            if f is None:
                group_of.append(GROUP_NONE)
                continue
            key = self._filter_key(f)
            if key not in seen:
                seen[key] = len(distinct)
                distinct.append(f)
            group_of.append(seen[key])
        qs = np.stack([q.data for q, _ in queries]).astype(np.float32, copy=False)
        ks = np.array([int(k) for _, k in queries], dtype=np.uintp)
        go = np.asarray(group_of, dtype=np.uint32)
        compiled = []
        try:
            if self._table is not None:
                for f in distinct:
                    cm = self.compile_filter_device(f)
                    if cm is None:                                 # one program beyond the limits: every mask from the host
                        break
                    compiled.append(cm)
            if distinct and len(compiled) == len(distinct):
                ids, dists, counts = self._index.search_batch_grouped(qs, 0, go, compiled_masks=compiled, ks=ks)
            elif not distinct:
                ids, dists, counts = self._index.search_batch_grouped(qs, 0, go, ks=ks)
            else:
                bits = max(self._next_id, 1)
                masks = np.zeros((len(distinct), (bits + 63) // 64), dtype=np.uint64)
                for i, f in enumerate(distinct):
                    masks[i] = self.compile_filter(f)[0]
                ids, dists, counts = self._index.search_batch_grouped(qs, 0, go, id_masks=masks, mask_bits=bits, ks=ks)
        finally:
            for cm in compiled:
                cm.release()
        return [self._map([(int(ids[b, i]), dists[b, i]) for i in range(int(counts[b]))]) for b in range(len(queries))]
