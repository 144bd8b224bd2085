/*
 * vdb_flat.h -- C ABI of the MI355X-native brute-force kNN engine.
 *
 * This is the drop-in boundary for the reference's FlatIndex hot path
 * (Ricoledan/vectordb-from-scratch).  The reference has no FFI layer; its seam
 * is the Rust trait `Index` (src/index.rs:11-35) implemented by `FlatIndex`
 * (src/flat_index.rs:37-74) and consumed by `VectorStore<I: Index>`
 * (src/storage.rs:83, :116-127).  Every entry point below names the reference
 * interface it replaces.  The Rust binding a maintainer would add is in
 * INTEGRATION.md; a C++ mirror of the trait lives in
 * vectordb-from-scratch_amd/host/.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ / torch types cross this boundary;
 *  - every function returns a vdb_status (0 = ok); no exception or panic
 *    crosses the boundary; vdb_last_error() gives the message and, for a
 *    dimension mismatch, the expected/actual pair (src/error.rs:12-13);
 *  - inputs are borrowed for the duration of the call; outputs are
 *    caller-allocated;
 *  - ids are the reference's `usize` internal ids, passed as uint64_t;
 *  - vectors are row-major little-endian f32, the byte layout of
 *    src/persistence/mmap.rs:77-84;
 *  - search entry points may be called concurrently from several threads on
 *    one handle (the server holds RwLock::read() around search,
 *    src/server/routes.rs:244,:342); add/remove are externally serialised by
 *    the caller's write lock (routes.rs:141,:210,:300).
 */
#ifndef VDB_FLAT_H
#define VDB_FLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/distance.rs:9-16  enum DistanceMetric */
typedef enum vdb_metric {
    VDB_METRIC_EUCLIDEAN = 0, /* sqrt(sum (a-b)^2)              distance.rs:37-44 */
    VDB_METRIC_COSINE = 1,    /* 1 - clamp(dot/(|a||b|), -1, 1) distance.rs:47-64 */
    VDB_METRIC_DOT = 2        /* -dot(a, b)                     distance.rs:31,:67-73 */
} vdb_metric;

/* src/error.rs:10-31  enum VectorDbError, as integer codes */
typedef enum vdb_status {
    VDB_OK = 0,
    VDB_ERR_DIMENSION_MISMATCH = 1, /* error.rs:12  DimensionMismatch{expected,actual} */
    VDB_ERR_INVALID_VECTOR = 2,     /* error.rs:18  InvalidVector (zero norm under Cosine, distance.rs:51-55) */
    VDB_ERR_NAN = 3,                /* the reference panics on a NaN distance (flat_index.rs:62); a panic cannot cross a C ABI */
    VDB_ERR_DEVICE = 4,             /* HIP runtime failure -> error.rs:30 IndexError(String) */
    VDB_ERR_INVALID_ARGUMENT = 5,   /* null pointer, bad metric, ... -> IndexError(String) */
    VDB_ERR_NOT_FOUND = 6           /* get_vector on an absent id (index.rs:23 returns None) */
} vdb_status;

typedef struct vdb_flat_index vdb_flat_index; /* opaque; owns all device and staging memory */

/* FlatIndex::new(metric)  src/flat_index.rs:19-25.  `device` is the HIP device ordinal. */
int vdb_flat_create(int metric, int device, vdb_flat_index **out);
void vdb_flat_destroy(vdb_flat_index *h);

/*
 * ONE index over several GPUs of one node, in ONE process -- the form the reference's seam needs: a server process holds a
 * single `VectorStore<I: Index>` behind one RwLock (src/storage.rs:83,:116-127, src/server/mod.rs:13-16), so the object that
 * implements `Index` must itself own the row shards (BASELINE.json north_star: "the index shards by database row across the
 * 8 GPUs of one node, each GPU producing a partial top-k that is merged after an RCCL all-gather over xGMI").
 *
 * The handle is an ordinary vdb_flat_index: every call below takes it.  Rows are dealt to the `n_devices` shards (one per
 * entry of `devices`; bulk loads in contiguous blocks, vdb_shard_range in vdb_shard.h; single adds to the shard that already
 * holds the id, else to the emptiest).  A batched search runs the local pipeline of every shard concurrently (one host
 * worker thread and one stream per shard), exchanges the packed partial top-k (ids | distances | counts | status,
 * nq*k*12 bytes per shard) and merges by (distance, id) on devices[0], where queries and outputs live.  Results are
 * identical to a single-GPU index over the same rows, bit for bit; errors keep the reference's semantics (a zero-norm row
 * on ANY shard fails the batch, src/flat_index.rs:57-60).
 *
 * Exchange (vdb_flat_set_exchange): VDB_EXCHANGE_RCCL -- in-process RCCL communicators (ncclCommInitAll), one grouped
 * ncclAllGather per batch; the default whenever the listed devices are distinct.  VDB_EXCHANGE_PEER -- each shard's stream
 * copies its packed block straight into devices[0]'s gather buffer (hipMemcpyPeerAsync over xGMI); the default when a device
 * is listed more than once (several shards on one GPU: how the multi-shard logic is tested on a one-GPU box -- RCCL refuses
 * two ranks on one device).
 *
 * Not available on a sharded handle: the two-half / ticket forms of the device search (begin/finish, submit/wait),
 * vdb_flat_distances_batch, the range searches (vdb_flat_range_search_batch, vdb_flat_range_search_batch_device), the grouped
 * searches (vdb_flat_search_batch_grouped, vdb_flat_search_batch_grouped_filtered, vdb_flat_grouped_stats), the diverse
 * top-k (vdb_flat_search_batch_mmr, vdb_flat_search_batch_mmr_filtered, vdb_flat_mmr_stats), the
 * vdb_flat_debug_* probes and vdb_flat_search_batch_sharded (that one is the process-per-GPU form of the same exchange,
 * vdb_shard.h); they return VDB_ERR_INVALID_ARGUMENT.
 */
int vdb_flat_create_sharded(int metric, const int *devices, size_t n_devices, vdb_flat_index **out);
/* number of shards of the handle (1 for a plain vdb_flat_create handle) */
size_t vdb_flat_shards(const vdb_flat_index *h);
/* live rows of shard `shard` (sharded handle), or vdb_flat_len for a plain handle with shard == 0 */
size_t vdb_flat_shard_len(const vdb_flat_index *h, size_t shard);
enum { VDB_EXCHANGE_RCCL = 0, VDB_EXCHANGE_PEER = 1 };
int vdb_flat_set_exchange(vdb_flat_index *h, int mode);
/* Counters of the last search on a sharded handle: [0] exchanges performed (1, or 2 when a shard needed its host after the
 * first tier), [1] shards, [2] exchange mode used, [3] ranks RCCL reports for the communicators (0 in peer mode),
 * [4] host clock of the call (ns), [5] host clock until every shard's first tier was enqueued (ns). */
int vdb_flat_shard_stats(const vdb_flat_index *h, uint64_t out[8]);

/* Index::add(id, vector)  src/index.rs:13, src/flat_index.rs:38-41.
 * Copies the row.  An existing id is overwritten silently (HashMap::insert).
 * Like the reference there is NO dimension check at add: a row whose dimension
 * differs from the rows already stored is kept (host side) and makes later
 * searches fail with DimensionMismatch, exactly as distance.rs:21-26 does. */
int vdb_flat_add(vdb_flat_index *h, uint64_t id, const float *vector, size_t dim);

/* N adds in one call (what 1M calls of Index::add amount to, storage.rs:135-172).
 * rows is [n][dim] contiguous; ids[i] belongs to row i (ids == NULL: first_id + i). */
int vdb_flat_add_bulk(vdb_flat_index *h, const uint64_t *ids, uint64_t first_id, const float *rows,
                      size_t n, size_t dim);
/* Same, with `d_rows` already resident in this device's HBM (device-to-device copy). */
int vdb_flat_add_bulk_device(vdb_flat_index *h, const uint64_t *ids, uint64_t first_id,
                             const float *d_rows, size_t n, size_t dim);

/* Bulk-load the reference's mmap vector file (src/persistence/mmap.rs:13-15 header `[dim u32 LE][count u32 LE]`,
 * :77-84 body = row-major little-endian f32): the file is memory-mapped and handed to the device in
 * large chunks instead of `count` add() calls.  The file has no id column: row i gets id first_id + i.
 * *out_count receives the number of rows loaded. */
int vdb_flat_load_vector_file(vdb_flat_index *h, const char *path, uint64_t first_id, size_t *out_count);

/* Index::remove(id)  src/index.rs:16, src/flat_index.rs:43-46.  Absent id is VDB_OK. */
int vdb_flat_remove(vdb_flat_index *h, uint64_t id);

/* Index::get_vector(id)  src/index.rs:23.  Copies up to cap floats into out, sets *dim. */
int vdb_flat_get_vector(vdb_flat_index *h, uint64_t id, float *out, size_t cap, size_t *dim);

/* Index::len / Index::metric  src/index.rs:26-29.  vdb_flat_dim: dimension of the stored rows (0 if empty). */
size_t vdb_flat_len(const vdb_flat_index *h);
int vdb_flat_metric(const vdb_flat_index *h);
size_t vdb_flat_dim(const vdb_flat_index *h);

/* Pre-size the device row store (optional; avoids regrowth copies during a bulk build). */
int vdb_flat_reserve(vdb_flat_index *h, size_t rows, size_t dim);

/* Push staged adds/removes to the device now (otherwise done lazily by the next search). */
int vdb_flat_flush(vdb_flat_index *h);

/*
 * Take the device rows of removed and overwritten vectors back (no reference counterpart: a HashMap frees what it removes,
 * src/flat_index.rs:43-46; search results are identical before and after, bit for bit).  remove() only clears a bit, and
 * VectorStore::insert_with_metadata turns every upsert into remove(old) + add(next_id++) (src/storage.rs:157-166), so a
 * long-lived store otherwise grows by a row per upsert and every search scans the dead rows too.
 *
 * vdb_flat_compact: staged adds are uploaded first; then the live rows and everything kept per row (norm, score coefficients,
 * certificate margin, id, the bf16 shadow row) move down over the dead ones ON THE DEVICE, in place and in their old order,
 * bit for bit (nothing is recomputed) -- the index then equals one that was given the surviving rows in the same order.
 * Extra device memory: a bounce buffer of 32 MiB plus 4 bytes per 32 rows, allocated before the first row moves.
 * *out_reclaimed (may be NULL) = device rows given back; 0, and no device work, when no row is dead.  shrink = 0 keeps the
 * capacity, so later adds reuse the freed tail; shrink != 0 then re-allocates the store to the capacity a fresh index of
 * that many rows would have -- THAT step holds the old and the new store at once.  Rows of another dimension are untouched.
 * A mutation like add / remove: under the caller's write lock (routes.rs:141,:210,:300), refused while a submitted search
 * is outstanding.  Failure: an error before the first row moved (allocation) leaves the index as it was; a HIP error after
 * that leaves rows half moved, so the handle then refuses every search, flush and get_vector with VDB_ERR_DEVICE (single
 * adds are still staged on the host, but can no longer be uploaded) -- destroy it.  On a sharded handle every shard compacts its own rows (concurrently); rows never change shards.
 *
 * vdb_flat_set_auto_compact(h, f): with 0 < f < 1 every flush -- and so the next search after a write -- compacts when more
 * than f * (device rows) of the uploaded rows are dead (never while a submitted search is outstanding).  Default 0 = never.
 *
 * vdb_flat_store_stats: [0] device rows, live + dead, staged ones included   [1] live rows   [2] capacity in rows
 *  [3] bytes of device memory the row store holds (rows, per-row columns, live mask, bf16 shadow)
 *  [4] compactions run   [5] rows reclaimed in total   [6] host clock of the last compaction, ns (the whole call: upload of
 *  the plan, the moves, renumbering the host's id -> row map)
 *  [7] the last compaction's device part: bits 0-39 ns from the first enqueue to the synchronise after the last move,
 *      bits 40-51 chunks that went through the bounce buffer, bits 52-63 chunks moved directly (both saturate at 4095).
 * On a sharded handle: sums over the shards; [6] and the time in [7] are maxima.
 */
int vdb_flat_compact(vdb_flat_index *h, int shrink, size_t *out_reclaimed);
int vdb_flat_set_auto_compact(vdb_flat_index *h, double dead_fraction);
int vdb_flat_store_stats(const vdb_flat_index *h, uint64_t out[8]);

/* Index::search(query, k)  src/index.rs:20, src/flat_index.rs:52-65.
 * out_ids/out_dists hold k entries; *out_count = min(k, len).  Ascending by
 * (distance, id): the reference's tie order is HashMap-random. */
int vdb_flat_search(vdb_flat_index *h, const float *query, size_t dim, size_t k, uint64_t *out_ids,
                    float *out_dists, size_t *out_count);

/*
 * The batched hot call.  Replaces the sequential loop of
 * VectorStore::search_batch (src/storage.rs:302-310) over FlatIndex::search,
 * with the per-query k of `&[(Vector, usize)]` (storage.rs:304).
 *   queries   [nq][dim] row-major f32 (host memory)
 *   ks        per-query k, or NULL to use `k` for every query
 *   id_mask   optional pre-filter: bit i (LSB-first in 64-bit words) set = id i
 *             eligible; ids >= mask_bits are not eligible; NULL = no filter.
 *             (BASELINE config 4; the reference post-filters a 3x over-fetch,
 *             storage.rs:249-290, whose result is a prefix of this one.)
 *   out_ids / out_dists   [nq][kstride], caller-allocated, kstride >= max k
 *   out_counts            [nq]: min(k_b, eligible rows)
 * The first failing query fails the whole batch (storage.rs:309).
 */
int vdb_flat_search_batch(vdb_flat_index *h, const float *queries, size_t nq, size_t dim,
                          const size_t *ks, size_t k, const uint64_t *id_mask, size_t mask_bits,
                          size_t kstride, uint64_t *out_ids, float *out_dists, size_t *out_counts);

/*
 * Same call with queries and outputs resident in this device's HBM and one k
 * for the whole batch; `stream` is a hipStream_t (NULL = the handle's own
 * stream).  d_id_mask is a device pointer (or NULL).  The call returns after
 * the results are complete on `stream` (it synchronises that stream once to
 * read the status word).  d_out_counts is uint32_t[nq].
 */
int vdb_flat_search_batch_device(vdb_flat_index *h, const float *d_queries, size_t nq, size_t dim,
                                 size_t k, const uint64_t *d_id_mask, size_t mask_bits,
                                 uint64_t *d_out_ids, float *d_out_dists, uint32_t *d_out_counts,
                                 void *stream);

/*
 * DistanceMetric::distance (src/distance.rs:20-33) for explicit (query, stored id) pairs, batched: the
 * candidate-list distance evaluations of an HNSW search (src/hnsw/graph.rs:155, :182 -- BASELINE config 5),
 * computed on the GPU in the reference's operation order (bit-identical to the CPU).  Query b is paired with
 * ids[offsets[b] .. offsets[b+1]); out_dists has offsets[nq] entries; an id that is not stored gives NaN.
 * Zero norm on either side under Cosine -> VDB_ERR_INVALID_VECTOR (distance.rs:51-55).
 */
int vdb_flat_distances_batch(vdb_flat_index *h, const float *queries, size_t nq, size_t dim,
                             const size_t *offsets, const uint64_t *ids, float *out_dists);

/*
 * Multi-GPU exchange step: merge `nparts` partial top-k lists per query
 * (gathered from the row shards with an RCCL all-gather) into the global
 * top-k, ascending by (distance, id).  All pointers are device pointers on
 * `device`; parts are laid out [nparts][nq][k] with counts [nparts][nq].
 * Any nparts * k (below 2^32): up to 2048 keys per query are sorted in LDS, above that every element is placed by
 * binary searches in the other parts, which requires each part's first counts[part][q] entries to be ascending by
 * (distance, id) -- as every search output is.  Ties between parts go to the lower part index; the result is the same.
 */
int vdb_merge_topk_device(int device, const uint64_t *d_part_ids, const float *d_part_dists,
                          const uint32_t *d_part_counts, size_t nparts, size_t nq, size_t k,
                          uint64_t *d_out_ids, float *d_out_dists, uint32_t *d_out_counts,
                          void *stream);

/* The device-resident search in two halves, for callers that have more work to enqueue behind it (the multi-GPU
 * exchange of sharded.py): _begin runs every check and enqueues the FIRST tier on `stream` without synchronising the
 * host; *d_code (device word, may be NULL) receives 0 when every query was certified by that tier and no error status
 * was raised, else VDB_PENDING_HOST.  _finish waits for the stream, runs the fallback tiers for the queries that need
 * them (*changed = 1 when outputs were rewritten) and reports the errors a plain vdb_flat_search_batch_device call
 * would.  The handle stays locked between the two calls, which must come from the same thread; every _begin that
 * returned VDB_OK must be followed by one _finish. */
#define VDB_PENDING_HOST 100
int vdb_flat_search_batch_device_begin(vdb_flat_index *h, const float *d_queries, size_t nq, size_t dim, size_t k,
                                       const uint64_t *d_id_mask, size_t mask_bits, uint64_t *d_out_ids,
                                       float *d_out_dists, uint32_t *d_out_counts, int32_t *d_code, void *stream);
int vdb_flat_search_batch_device_finish(vdb_flat_index *h, int *changed);

/*
 * The device-resident search ASYNCHRONOUSLY, two batches in flight per handle (no reference counterpart: the reference's
 * batch loop, src/storage.rs:302-310, is synchronous; this is what a server that keeps the GPU busy calls instead).
 * _submit runs every check and enqueues the first tier on `stream` (NULL = a stream of the context it picked) and
 * returns a ticket WITHOUT waiting; _wait(ticket) waits for that search, runs its fallback tiers where needed and reports
 * the errors a plain vdb_flat_search_batch_device call would.  While batch i's HBM-bound pass runs, batch i+1's query
 * preparation and the host's turnaround are hidden behind it.  Rules: at most two tickets outstanding per handle (a third
 * submit fails); every ticket must be waited for exactly once; outputs are complete when _wait returns; add / remove /
 * flush and the host-pointer entry points are refused while a ticket is outstanding (the caller's read lock spans
 * submit .. wait, routes.rs:244,:342); a synchronous vdb_flat_search_batch_device call may run beside ONE outstanding ticket.
 */
int vdb_flat_search_batch_device_submit(vdb_flat_index *h, const float *d_queries, size_t nq, size_t dim, size_t k,
                                        const uint64_t *d_id_mask, size_t mask_bits, uint64_t *d_out_ids,
                                        float *d_out_dists, uint32_t *d_out_counts, void *stream, int *ticket);
int vdb_flat_search_batch_device_wait(vdb_flat_index *h, int ticket);

/* The same merge reading the all-gathered exchange buffer in place.  Each part is `words_per_part` int32
 * words (even): ids int64[nq*k] | dists f32[nq*k] | counts i32[nq] | status i32 | pad.  *d_out_status (may be
 * NULL) receives the maximum status word over the parts, so one host read tells whether any shard failed.  The same
 * range of nparts * k as vdb_merge_topk_device, and the same requirement above 2048 keys: every part ascending. */
int vdb_merge_topk_packed_device(int device, const int32_t *d_packed, size_t nparts, size_t words_per_part,
                                 size_t nq, size_t k, uint64_t *d_out_ids, float *d_out_dists,
                                 uint32_t *d_out_counts, uint32_t *d_out_status, void *stream);

/* Measurement hook for bench.py: when on, every search brackets its fused MFMA kernel launch
 * with HIP events on the launch stream and vdb_flat_last_stats()[7] reports the kernel's
 * duration in nanoseconds (summed over the launches of that search). */
int vdb_flat_set_profile(vdb_flat_index *h, int on);

/* Counters of the last search on this handle (diagnostics, tests, bench):
 *  [0] queries answered by the MFMA path   [1] queries re-done by the exact-scan fallback
 *  [2] candidate-pool overflows            [3] rows scanned by the fused kernel
 *  [4] sample rows used for the thresholds [5] k' (candidates kept per query)
 *  [6] uncertified queries                 [7] fused-kernel time of the search, ns (profiling on) */
int vdb_flat_last_stats(const vdb_flat_index *h, uint64_t out[8]);

/* The same counters followed by (n up to 16, the rest reads 0):
 *  [8] 1 when the bf16 screening tier answered the batch first, 0 when only the f32 MFMA tier ran
 *  [9] queries the screening tier could not certify and handed to the f32 MFMA tier
 *  [10] [11] [12] host clock of the call, ns: first tier enqueued / its flags on the host / return
 *  [13] queries answered by the re-threshold pass (a second screening pass whose thresholds are the score cuts that the
 *       k-th exact distances of the first pass imply; every key under the cut is re-ranked), for every k the screening
 *       tier serves: k <= 112 and the large-k range 112 < k <= 1024
 *  [14] 1 when the screening pass read the bf16 shadow rows (vdb_flat_set_shadow)
 *  [15] 1 when the library is the DIAGNOSTICS build (-DVDB_DIAG) and one of its environment knobs is set: such a run
 *       is not covered by the exactness guarantee.  Always 0 in the release library, which reads no environment.
 * With the screening tier on, [4] [5] [7] describe ITS sample, k' and kernel time. */
int vdb_flat_last_stats_ex(const vdb_flat_index *h, uint64_t *out, size_t n);

/* Tier selection for indexes above 16384 rows (no reference counterpart; results are identical either way):
 *  1 (default): a first pass ranks every row on the bf16 matrix cores (HBM-bound), keeps k' candidates per
 *     query, re-ranks them with the reference's exact f32 arithmetic (distance.rs:37-73) and certifies the
 *     result with a rigorous bound on the bf16 rounding error; uncertified queries go to the f32 tier;
 *  0: the f32-input MFMA tier only (v_mfma_f32_32x32x2_f32, arithmetic-bound), then the exact scan.
 */
int vdb_flat_set_screen(vdb_flat_index *h, int mode);

/* Batches above 256 queries (VectorStore::search_batch takes any number, storage.rs:302-310; BASELINE config 3: 1024):
 *  1 (default): the screening pass serves 512 queries per fetch of the rows (128 rows x 512 queries per workgroup), so a batch
 *     of B queries reads the database ceil(B / 512) times;
 *  0: 256 queries per fetch (the kernel of batches up to 256), ceil(B / 256) reads.
 * No reference counterpart; results are identical either way, bit for bit. */
int vdb_flat_set_wide(vdb_flat_index *h, int on);

/* The layout of the stored rows (no reference counterpart; results are identical in every mode, bit for bit).  An index
 * whose rows have a pitch of a multiple of 64 floats may keep every row SPLIT in place into its bf16 piece and its low
 * halves -- same address, same bytes, no extra memory -- so that the screening tier's filter pass streams 2 bytes per
 * element instead of 4.  Only that pass and its re-ranks read split rows; every other reader or writer of the rows
 * (the f32 and exact tiers, range, by-id, distinct, grouped, recommend, MMR, sparse, get_vector, adds, compaction, ...)
 * first converts the store back, which costs a pass over it.  Rows holding an inf or NaN element stay plain f32.
 *  0: never convert;
 *  1 (default): adaptive -- after a run of screened searches of at most 256 queries with nothing else in between, the
 *     next one converts first (never while another search of the handle is in flight);
 *  2: convert before the next such search.
 * On a sharded handle the mode goes to every shard; each shard decides for itself.
 * vdb_flat_layout: out[0] = 0 plain f32 rows, 1 split rows (a sharded handle: 1 only if every shard is split);
 * out[1] = conversions so far, both directions (summed over the shards).
 * vdb_flat_debug_set_split_after (tests): the length of the run in mode 1 (0 = the default). */
int vdb_flat_set_split(vdb_flat_index *h, int mode);
int vdb_flat_layout(vdb_flat_index *h, uint64_t out[2]);
int vdb_flat_debug_set_split_after(vdb_flat_index *h, size_t searches);

/* The screening tier's LARGE-k range (no reference counterpart; results are identical either way, bit for bit):
 *  1 (default): 112 < k <= 1024 is served by the bf16 screening pass too -- a deeper filter threshold, up to 2048
 *     candidates per query, and the certified re-rank of kernels_aux.hip (rerank_large_kernel) -- on indexes of at least
 *     vdb_flat_large_k_min_rows(k) rows; an uncertified query takes the re-threshold pass (one more filter pass under the
 *     score cut of its k-th exact distance, every key under the cut re-ranked: last_stats_ex()[13]) and goes to the exact
 *     scan only when more than 2048 keys lie under the cut or a candidate pool overflowed.  last_stats_ex()[8] = 1 when the
 *     range ran, [5] = the candidate depth;
 *  0: k > 112 goes to the exact scan, as before the range existed.
 * On a sharded handle it applies to every shard. */
int vdb_flat_set_large_k(vdb_flat_index *h, int on);
/* The smallest row count (of one handle or one shard) on which the large-k range serves k; 0 outside 112 < k <= 1024. */
size_t vdb_flat_large_k_min_rows(size_t k);

/*
 * The SPARSE-FILTER route of pre-filtered searches (no reference counterpart; results are identical whatever the mode, bit for
 * bit).  A search with an id mask normally costs one pass over every stored row, whatever the mask lets through.  On this route
 * the eligible rows (live AND admitted by the mask) are gathered into a list on the device, the reference distance of every
 * (query, eligible row) pair is computed in the reference's operation order (csrc/kernels_sparse.hip), and the k smallest by
 * (distance, id) are written as the results: only the eligible rows are read.
 *  0 (default): never -- every search runs as if this setting did not exist;
 *  1: always -- every search that carries an id mask takes the route when k <= 2048 and at most 131072 rows are eligible
 *     (also on indexes small enough for the direct path); otherwise it continues into the tiers unchanged;
 *  2: automatic -- as 1, but only when the list is at most vdb_flat_sparse_limit(rows, padded dimension, dimension, nq) long,
 *     and indexes of at most 16384 rows with batches of at most 8 queries keep their direct path.
 * In modes 1 and 2 a masked search reads the eligible-row count back (4 bytes, one stream synchronisation) before it chooses.
 * Searches without an id mask are never affected.  Errors are those of the exact scans under a row mask: the dimension checks
 * and the zero-norm-row check under Cosine come first, a zero-norm query is an InvalidVector error, a NaN distance among the
 * ELIGIBLE rows is VDB_ERR_NAN.  A search answered by the route is complete when _begin / _submit return.
 * On a sharded handle the setting applies to every shard, and every shard decides from its own list.
 */
int vdb_flat_set_sparse_filter(vdb_flat_index *h, int mode);
/* out[0] = 1 when the last search on the handle was answered by the route, [1] = eligible rows of the last masked search made
 * with mode != 0, [2] = searches answered by the route since creation, [3] = 0 (reserved).  Sharded handle: [0] is the OR over
 * the shards, [1] and [2] are sums. */
int vdb_flat_sparse_stats(vdb_flat_index *h, uint64_t out[4]);
/* The longest list of eligible rows that mode 2 sends to the route for an index (or shard) of n_rows rows of ld floats (the
 * dimension rounded up to 32), queries of `dim` elements and a batch of nq: E * nq * dim <= C * n_rows * ld with the measured
 * constant C, never above 131072 or n_rows.  0 for an empty index.  Needs no handle and no device. */
size_t vdb_flat_sparse_limit(size_t n_rows, size_t ld, size_t dim, size_t nq);
/* Diagnostics (tests).  vdb_flat_debug_eligible_rows flushes, builds the row mask and the eligible-row list exactly as a search
 * on the route would -- id_mask in the layout of vdb_flat_search_batch, in device OR host memory -- and copies the first `cap`
 * device rows (ascending) to out and the length of the list to *count; no distance is computed.  Not on a sharded handle.
 * vdb_flat_debug_sparse_tile_rows / _queries: the tile of one workgroup of the scan kernel, in list positions and queries. */
int vdb_flat_debug_eligible_rows(vdb_flat_index *h, const uint64_t *id_mask, size_t mask_bits, uint32_t *out, size_t cap,
                                 size_t *count);
size_t vdb_flat_debug_sparse_tile_rows(void);
size_t vdb_flat_debug_sparse_tile_queries(void);

/*
 * EXACT RANGE SEARCH: every neighbour within a radius (no reference counterpart: Index::search, flat_index.rs:52-65, only
 * answers "the k nearest").  For query q and radius r the result is the set of eligible rows (live, admitted by the optional id
 * mask) whose reference distance d -- DistanceMetric::distance in the reference's own f32 operation order, distance.rs:20-73 --
 * satisfies the IEEE comparison d <= r: a row at exactly r is in, -0.0 equals +0.0.  Results are ascending by (distance,
 * unsigned id); the first min(total, max_results) of that order are written and `total`, the number of rows within the radius,
 * is reported whether they fit or not.  This is the prefix with d <= r of what vdb_flat_search_batch returns for k = len, bit
 * for bit, on every route:
 *  - large indexes (screening tier on, at least 65536 rows): the radius becomes a score cut -- the inverse of the screening
 *    tier's certificate: every row scoring above the cut is PROVEN to lie strictly beyond r, so rows at the radius score at or
 *    below it -- the HBM-bound bf16 filter pass runs once under the cuts, and EVERY key that passes (up to 2048 per query) is
 *    evaluated exactly.  No sample pass, no certificate to wait for: the list is complete by construction;
 *  - everything else (small indexes, vdb_flat_set_screen(0), a query with more than 2048 keys under its cut, an overflowed
 *    pool, a radius without a finite cut: +-inf, >= 2 under Cosine, a tiny query norm): an exact scan that keeps the rows with
 *    d <= r, eight queries per pass over the rows;
 *  - more than 32768 rows within the radius: the full exact scan of that query for its first max_results.
 * radii: one radius per query, or NULL to use `radius` for all.  out_ids / out_dists: [nq][max_results], unused slots are not
 * written by the host form (the device form pads them with id ~0 and a NaN distance).  out_counts[b] = entries written,
 * out_totals[b] (may be NULL) = rows within the radius.
 * Errors, in the order of the searches: an empty index gives counts and totals 0 before any check; dimension mismatch; under
 * Cosine one live zero-norm row fails the call, masked or not, and a zero-norm query is VDB_ERR_INVALID_VECTOR; a NaN distance
 * at an eligible row is VDB_ERR_NAN.  A NaN radius, max_results == 0 or max_results > 2048 is VDB_ERR_INVALID_ARGUMENT before
 * any device work.  Locking, workspaces and tickets as vdb_flat_search_batch / _device: concurrent callers are serialised by
 * the handle, the host-pointer form is refused while a submitted search is in flight, staged adds are flushed first.
 * Not available on a sharded handle (totals across shards need another exchange layout).
 */
int vdb_flat_range_search_batch(vdb_flat_index *h, const float *queries, size_t nq, size_t dim,
                                const float *radii, float radius, const uint64_t *id_mask, size_t mask_bits,
                                size_t max_results, uint64_t *out_ids, float *out_dists,
                                size_t *out_counts, uint64_t *out_totals);
/* queries, radii (required), mask and outputs in this device's HBM; d_out_counts uint32[nq], d_out_totals uint64[nq] or NULL */
int vdb_flat_range_search_batch_device(vdb_flat_index *h, const float *d_queries, size_t nq, size_t dim,
                                       const float *d_radii, const uint64_t *d_id_mask, size_t mask_bits,
                                       size_t max_results, uint64_t *d_out_ids, float *d_out_dists,
                                       uint32_t *d_out_counts, uint64_t *d_out_totals, void *stream);
/* counters of the last range search: [0] queries answered by the screened route  [1] by the exact range scan
 * [2] by the dense fallback (more than 32768 rows within the radius)  [3] rows streamed by filter passes
 * [4] keys re-ranked  [5] queries whose pool or select overflowed  [6] queries without a finite score cut  [7] 0 */
int vdb_flat_range_stats(const vdb_flat_index *h, uint64_t out[8]);

/*
 * METADATA FILTERS COMPILED ON THE DEVICE (no reference counterpart: the reference evaluates MetadataFilter::matches row by row
 * on the host, src/storage.rs:60-71, :272-287; search results are identical to those under the same mask built on the host, bit
 * for bit).  A pre-filtered search needs the id bitmask of its filter.  Instead of building it on the host and uploading it with
 * every request, the store keeps its metadata resident in HBM and the mask is computed there: one kernel launch, no transfer
 * larger than the filter expression.
 *
 * vdb_meta_table: the metadata by INTERNAL id, on one device.  It belongs to the store, not to an index handle.  It holds
 * columns, addressed by a small integer slot, of int32 dictionary codes (codes[id]; -1 = the row has no such field; an id never
 * written reads as -1; columns grow independently and may be shorter than a mask), and a presence bitmap in the layout of id_mask.
 * vdb_meta_set_codes / vdb_meta_set_present are WRITES (the caller's write lock, like add / remove, routes.rs:141,:210,:300): they
 * are staged on the host and reach the device as dirty ranges in front of the next compile, the add / flush pattern of the index.
 * A slot is known once vdb_meta_set_codes was called for it (n = 0 is enough).  Ids at or above 2^32: VDB_ERR_INVALID_ARGUMENT.
 *
 * vdb_meta_compile: `ops` is the filter as a POSTFIX program -- EQ slot code, NE slot code, EXISTS slot, CONST 0|1 push a
 * verdict, AND / OR replace the two topmost by one.  Leaves are MetadataFilter::matches' (storage.rs:62-67): EQ is code == c, NE
 * is code != c (a row without the field matches), EXISTS is code >= 0.  Whatever needs the dictionary (an unknown field or value)
 * is resolved to CONST by the caller.  At most 1024 ops, evaluation stack at most 32 deep, exactly one value left, every slot
 * known -- else VDB_ERR_INVALID_ARGUMENT before any device work.  On the table's stream and WITHOUT waiting for it: the staged
 * ranges are uploaded, one kernel writes bit i = present(i) AND program(i) for every i < mask_bits (tail bits of the last word
 * clear; mask_bits == 0 writes nothing) and counts the set bits.  *out is a mask from a pool inside the table (no allocation per
 * request after warm-up) with an event marking its completion.  A read: may be called from several threads at once.
 *
 * NUMERIC LEAVES (no reference counterpart: the reference's filter has Eq / Ne / Exists / And / Or only, src/storage.rs:45-58).
 * LT / LE / GT / GE compare the NUMBER of the row's string with a binary64 constant.  A string is numeric iff all of it matches
 * [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)? in ASCII and its correctly rounded binary64 value is finite; that value is
 * its number (so integers above 2^53 compare by their roundings).  Values stay strings and rows gain no storage: the number of a
 * row is a lookup by its dictionary code.  vdb_meta_set_numbers writes that table for column `slot`: values[i] is the number of
 * code first_code + i, NaN = "no number".  A WRITE like vdb_meta_set_codes: staged, uploaded as a dirty range in front of the
 * next compile; the table grows independently of the codes, a new tail reads as NaN, n = 0 is allowed, first_code + n above 2^31
 * is VDB_ERR_INVALID_ARGUMENT.  A slot without a table has one of length 0.  It does not make a slot known.
 * vdb_meta_compile_num is vdb_meta_compile with constants: for LT / LE / GT / GE, `slot` is the column (it must be known, as for
 * EQ) and `code` an index into consts.  The leaf is true iff the row's code c satisfies 0 <= c < the table's length and
 * table[c] OP consts[code] holds as an IEEE comparison (-0 == +0; a NaN entry fails all four; the constant may be +-inf).  A row
 * without the field, with a non-numeric string, or whose code lies outside the table matches none of the four -- whatever int32
 * the column holds, no memory outside the table is read.  n_consts > 1024, a constant index at or beyond n_consts, a NaN
 * constant and a null consts with n_consts > 0 are VDB_ERR_INVALID_ARGUMENT before any device work; everything else (limits,
 * pool, event, count, locking) is vdb_meta_compile's, which is this call with n_consts = 0 and therefore refuses a numeric op.
 * Opcodes 6..15 are unknown.
 *
 * vdb_meta_mask_ptr: the device pointer, for the d_id_mask of vdb_flat_search_batch_device / _begin / _submit, once the
 * caller's stream is ordered behind the mask with vdb_meta_mask_wait_on (hipStreamWaitEvent, no host wait; stream NULL = the
 * null stream).  vdb_meta_mask_bits: its mask_bits.  vdb_meta_mask_count: waits for the event, reads the number of set bits
 * (8 bytes).  vdb_meta_mask_release: back to the pool -- after the last search that reads it has completed; the next compile may
 * hand the same buffer out again.  vdb_meta_destroy frees the table and every mask it made.
 *
 * vdb_flat_search_batch_filtered: vdb_flat_search_batch (host queries, per-query ks, host outputs) under a compiled mask: the
 * handle's stream is ordered behind the mask's event and nothing is uploaded for the filter; the same search code runs below it
 * (tiers, sparse-filter route), so results are identical to the host-mask call, bit for bit.  Plain and sharded handles (the
 * table must then be on devices[0]); a mask on another device or a null mask is VDB_ERR_INVALID_ARGUMENT.
 */
typedef struct vdb_meta_table vdb_meta_table;
#ifndef VDB_META_MASK_DECLARED                  /* (vdb_hnsw.h declares the same type: either header may come first) */
#define VDB_META_MASK_DECLARED
typedef struct vdb_meta_mask vdb_meta_mask;
#endif
enum { VDB_META_EQ = 0, VDB_META_NE = 1, VDB_META_EXISTS = 2, VDB_META_CONST = 3, VDB_META_AND = 4, VDB_META_OR = 5,
       VDB_META_LT = 16, VDB_META_LE = 17, VDB_META_GT = 18, VDB_META_GE = 19 };
typedef struct vdb_meta_op { uint32_t op; uint32_t slot; int32_t code; } vdb_meta_op; /* CONST: code = 0 | 1; AND / OR: both unused; LT..GE: code = constant index */
int vdb_meta_create(int device, vdb_meta_table **out);
void vdb_meta_destroy(vdb_meta_table *t);
int vdb_meta_set_codes(vdb_meta_table *t, uint32_t slot, uint64_t first_id, const int32_t *codes, size_t n);
int vdb_meta_set_present(vdb_meta_table *t, uint64_t first_id, size_t n, int on);
int vdb_meta_set_numbers(vdb_meta_table *t, uint32_t slot, uint32_t first_code, const double *values, size_t n);
int vdb_meta_compile(vdb_meta_table *t, const vdb_meta_op *ops, size_t n_ops, size_t mask_bits, vdb_meta_mask **out);
int vdb_meta_compile_num(vdb_meta_table *t, const vdb_meta_op *ops, size_t n_ops, const double *consts, size_t n_consts, size_t mask_bits,
                         vdb_meta_mask **out);
const uint64_t *vdb_meta_mask_ptr(const vdb_meta_mask *m);
size_t vdb_meta_mask_bits(const vdb_meta_mask *m);
int vdb_meta_mask_count(vdb_meta_mask *m, uint64_t *eligible);
int vdb_meta_mask_wait_on(vdb_meta_mask *m, void *stream);
int vdb_meta_mask_release(vdb_meta_mask *m);
int vdb_flat_search_batch_filtered(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                   const vdb_meta_mask *mask, size_t kstride, uint64_t *out_ids, float *out_dists,
                                   size_t *out_counts);

/*
 * SEARCH BY STORED ID: "what is near item x?" (no reference counterpart: Index::search, src/index.rs / src/flat_index.rs:52-65,
 * takes a vector; a caller would get_vector, search with k + 1 and drop the item on the host).  One sentence defines the call: for
 * query id x and count k the result is what vdb_flat_search_batch returns for the STORED VECTOR of x with k + 1 under the same
 * mask, with the entry whose id equals x removed if it is there, cut to k -- ids, order, distance bits, counts and errors.
 * Dropping the last of the k + 1 when x is absent is exact: the top k of "eligible rows without x" is the top k + 1 of "eligible
 * rows", minus x, cut to k.  The vectors never leave HBM: the row numbers of the ids go up, a kernel gathers the rows into the
 * query block, the search runs, a second kernel strikes x from each list, the results come down (csrc/kernels_by_id.hip).
 *  - The strike is by 64-bit id EQUALITY among the first `count` entries of a list: never by position ("drop the first hit" is
 *    wrong -- under Dot the row itself is often not among the k + 1 best, and under any metric a duplicate with a lower id sorts in
 *    front of it), never by distance, and no id value is a flag: 2^64 - 1 is a legal stored id and a legal query id.
 *  - out_counts[b] = min(k_b, eligible rows - [x eligible]).  A query id that the mask makes ineligible is still a valid query:
 *    it is then simply not in its list.
 *  - ks: one search with max(ks) + 1 and one strike; each query's answer is the first k_b entries of its struck list (the prefix
 *    property of vdb_flat_search_batch).  k is clamped to len before the 1 is added, so k = SIZE_MAX cannot wrap.
 *  - A query id that is not stored -- never added, or removed -- fails the whole batch with VDB_ERR_NOT_FOUND; staged adds and
 *    removes are flushed first; the message names the first such id; no device search is run.
 *  - A query id whose row has another dimension than the index (vdb_flat_add keeps such rows on the host) fails with
 *    VDB_ERR_DIMENSION_MISMATCH, exactly as searching with that vector would.
 *  - The same query id may appear several times in one batch.
 *  - Zero-norm rows under Cosine (VDB_ERR_INVALID_VECTOR) and NaN distances (VDB_ERR_NAN) are the errors of the equivalent search.
 *  - nq is unbounded, as in vdb_flat_search_batch.  Because the search runs with k + 1, k = 112 is served by the large-k range
 *    (vdb_flat_set_large_k) and k = 1024 by the exact scan: the tier boundaries lie one lower than for a search by vector.
 *  - Locking and tickets as vdb_flat_search_batch: refused while a submitted search is outstanding.
 * On a sharded handle the row of x lives on one shard: that shard gathers its queries on its own device, the block goes to
 * devices[0] device-to-device, the sharded search runs with k + 1 and the strike runs on devices[0]; an id on no shard is
 * VDB_ERR_NOT_FOUND.  _filtered is the same call under a compiled mask (vdb_flat_search_batch_filtered).
 * vdb_flat_by_id_stats describes the last call on the handle: [0] queries, [1] queries whose own id was found and struck,
 * [2] queries cut at k instead, [3] 0.
 */
int vdb_flat_search_batch_by_id(vdb_flat_index *h, const uint64_t *query_ids, size_t nq, const size_t *ks, size_t k,
                                const uint64_t *id_mask, size_t mask_bits, size_t kstride,
                                uint64_t *out_ids, float *out_dists, size_t *out_counts);
int vdb_flat_search_batch_by_id_filtered(vdb_flat_index *h, const uint64_t *query_ids, size_t nq, const size_t *ks, size_t k,
                                         const vdb_meta_mask *mask, size_t kstride,
                                         uint64_t *out_ids, float *out_dists, size_t *out_counts);
int vdb_flat_by_id_stats(const vdb_flat_index *h, uint64_t out[4]);

/*
 * RECOMMEND FROM POSITIVE AND NEGATIVE STORED IDS: "more like these, less like those" (no reference counterpart; a caller would
 * get_vector every example, fold them on the host, upload, search with k + m and strike the examples on the host).  One sentence
 * defines the call: for request b with positives p_1..p_np (np >= 1) and negatives n_1..n_nn (nn >= 0), all stored ids, and count
 * k_b, the result is what vdb_flat_search_batch returns for the vector q_b with k_b + np + nn under the same mask, with every entry
 * whose id is among the examples removed, cut to k_b -- ids, order, distance bits, counts and errors.
 * q_b is computed per element j in f32 without contraction (the library is built with -ffp-contract=off):
 *  - positive fold: sp = p_1[j]; for i = 2..np: sp = sp + p_i[j].  A LEFT fold in list order, started from the first row and not
 *    from 0: -0.0 survives, and np = 1 is the stored row itself.
 *  - positive average: ap = sp when np == 1, else ap = sp * rp with rp = 1.0f / (float)np computed once on the host: a multiply,
 *    never a division on the device.
 *  - query: nn == 0: q[j] = ap; otherwise an is built from the negatives in the same way and q[j] = ap + (ap - an).
 * The order of the adds and the multiply are observable in the distance bits, so they are part of the contract.  The vectors never
 * leave HBM: the lists go up, fold_examples_kernel writes the query block from the stored rows, the search runs, strike_set_kernel
 * removes the examples from each list, the results come down (csrc/kernels_recommend.hip).
 *  - Request b owns example_ids[offsets[b] .. offsets[b + 1]); the first n_pos[b] of them are positives, the rest negatives.
 *  - Recommend with ([x], []) is vdb_flat_search_batch_by_id([x]) bit for bit.
 *  - Removing the m = np + nn examples from the top k + m and cutting to k is exact, for the same reason by-id's + 1 is: the top k
 *    of "eligible rows without the examples" is the top k + m of "eligible rows", minus the examples, cut to k.
 *  - An example that the mask makes ineligible is still a valid example: it is folded, and it is simply in nobody's list.
 *  - The same id may appear several times in a request, on either side or on both: it is folded as often as it is listed.  The
 *    strike is by SET (64-bit id equality); the over-fetch is by COUNT m, which is at least the size of the set.
 *  - No id value is a flag: 2^64 - 1 is a legal example and a legal neighbour.
 *  - ks: ONE search at depth min(min(max ks, len) + max_b m_b, len) and one strike; the answer for k_b is the first k_b entries of
 *    the struck list.  k is clamped to len before m is added, as by-id does, so k = SIZE_MAX cannot wrap.
 * VDB_ERR_INVALID_ARGUMENT before any device work: a null array (nq > 0), offsets[0] != 0, decreasing offsets, n_pos[b] == 0,
 * n_pos[b] above the request's length, more than VDB_RECOMMEND_MAX_EXAMPLES examples in a request, offsets[nq] > 2^20.  After
 * those, in by-id's order: staged adds and removes are flushed; an example that is not stored -- never added, or removed -- fails
 * the whole batch with VDB_ERR_NOT_FOUND, the message naming the first such id in array order; an example whose row has another
 * dimension than the index fails with VDB_ERR_DIMENSION_MISMATCH; everything else is the error of the equivalent search: a fold that
 * comes out all zero under Cosine (p and -p) is VDB_ERR_INVALID_VECTOR, a fold that overflows gives what searching with that vector
 * gives (VDB_ERR_NAN where a distance is NaN).  Locking and tickets as vdb_flat_search_batch_by_id.
 * On a sharded handle every shard gathers the rows of ITS examples on its own device, the blocks go to devices[0] device-to-device
 * and the fold runs there over the staged rows: the fold order is the request's list order wherever the rows live.  _filtered is
 * the same call under a compiled mask (vdb_flat_search_batch_filtered).
 * vdb_flat_recommend_stats describes the last call on the handle: [0] requests, [1] example rows folded (the sum of m_b),
 * [2] entries struck in total (those in front of the cut of the batch-wide list), [3] the depth the search ran at.
 */
#define VDB_RECOMMEND_MAX_EXAMPLES 64   /* per request, positives + negatives */
int vdb_flat_recommend_batch(vdb_flat_index *h, const uint64_t *example_ids, const size_t *offsets /* [nq + 1] */,
                             const uint32_t *n_pos /* [nq] */, size_t nq, const size_t *ks, size_t k,
                             const uint64_t *id_mask, size_t mask_bits, size_t kstride,
                             uint64_t *out_ids, float *out_dists, size_t *out_counts);
int vdb_flat_recommend_batch_filtered(vdb_flat_index *h, const uint64_t *example_ids, const size_t *offsets /* [nq + 1] */,
                                      const uint32_t *n_pos /* [nq] */, size_t nq, const size_t *ks, size_t k,
                                      const vdb_meta_mask *mask, size_t kstride,
                                      uint64_t *out_ids, float *out_dists, size_t *out_counts);
int vdb_flat_recommend_stats(const vdb_flat_index *h, uint64_t out[4]);

/*
 * RECOMMEND BY BEST SCORE: nearest to ANY positive, vetoed by the negatives (no reference counterpart; a caller would search by id
 * once per positive, get_vector every candidate and every negative, and fold on the host).  vdb_flat_recommend_batch answers "more
 * like the centre of these"; this call scores every candidate against every example on its own.  Request b has positives
 * p_1..p_np (np >= 1), negatives n_1..n_nn (nn >= 0), all stored ids, laid out as in vdb_flat_recommend_batch, and a count k_b.
 * d(e, x) is the reference distance with the stored vector of example e as the query and row x as the row: exactly what
 * vdb_flat_search_batch_by_id([e]) reports for x.
 *  - Eligible rows: the live rows the optional mask admits, minus the SET of the request's example ids (64-bit equality).
 *  - dp(x): dp = d(p_1, x); for i = 2..np: if d(p_i, x) < dp then dp = d(p_i, x).  A left fold in list order with the IEEE <: on
 *    equal values, -0.0 and +0.0 included, the earlier positive's bits stay.
 *  - Kept: x is kept iff nn == 0, or dp(x) < d(n_j, x) holds for every j.  A tie is a veto; a NaN d(n_j, x) is a veto.  The rule is
 *    decided row by row and does not depend on the route the engine took.
 *  - dn(x): for a kept row, the same left fold over the negatives; +inf when nn == 0.
 *  - Result: the kept rows ascending by (dp, unsigned id), in the order the plain search gives equal distances (-0.0 in front of
 *    +0.0), cut to min(k_b, len): out_ids, out_dists (dp, bit for bit), out_neg_dists (dn; may be NULL), out_counts.  Fewer than
 *    k_b kept rows is a short list, not an error.  min(max k_b, len) may not exceed VDB_RECOMMEND_BEST_MAX_K.
 * Consequences: one positive and no negatives is vdb_flat_search_batch_by_id bit for bit; an example the mask hides is still an
 * example; the same id may repeat and may stand on both sides; no id value is a flag.
 * Errors, in this order: (1) recommend's argument checks, before any device work, with the same limits; (2) staged writes are
 * flushed; (3) VDB_ERR_NOT_FOUND and VDB_ERR_DIMENSION_MISMATCH as recommend; (4) under Cosine a zero-norm example, like any live
 * zero-norm row, is VDB_ERR_INVALID_VECTOR; (5) a NaN d(p_i, x) at any live row the mask admits -- the examples included: they are
 * struck afterwards -- is VDB_ERR_NAN, on every route.
 * Not built, refused with VDB_ERR_INVALID_ARGUMENT where a caller can reach it: ranking the vetoed rows behind the kept ones,
 * np = 0, sharded handles, device-pointer and ticket forms.  A sharded handle is refused among the checks of (1): before the
 * flush and before any id is resolved, so also on an empty index and for an id that is not stored (unlike
 * vdb_flat_search_batch_mmr and vdb_flat_search_batch_per_group, which answer an empty index with counts 0 first).
 * How (csrc/kernels_recommend_best.hip): the positives of all requests are gathered into one query block on the
 * device and ONE certified search ranks them at depth D.  A list with D entries ends at its frontier, F is the smallest frontier
 * of a request, and an entry with d < F is settled: a row missing from list i has d(p_i, x) >= F, so the smallest distance seen
 * for a settled row is its dp.  A merge kernel walks the settled entries in (dp, id) order, a veto kernel computes the exact
 * d(n_j, x) for those rows, applies the kept rule and keeps the first k_b.  A request is answered when k_b rows were kept or
 * nothing can lie behind its candidates; the others run again at depth min(len, 1024), and what is left gets ONE exact pass over
 * the rows per request.  vdb_flat_recommend_best_depth(k, m, len, stage) is the depth of stage 0 -- min(len, min(1024,
 * max(2 (k + m), 32))), k = min(max k_b, len), m = the longest request -- and of stage 1; 0 for any other stage.
 * vdb_flat_recommend_best_stats describes the last call: [0] requests, [1] example rows, [2] requests answered at stage 0, [3] at
 * stage 1, [4] by the exact scan, [5] the stage-0 depth, [6] list searches run (the sum of np over every stage a request went
 * through), [7] 0.  vdb_flat_debug_set_recommend_best_route (tests): 0 automatic (lists first unless the stage-0 depth is the whole
 * index), 1 lists first always, 2 the exact scan only; the answers are the same bits on every route.
 */
#define VDB_RECOMMEND_BEST_MAX_K 1024
int vdb_flat_recommend_best_batch(vdb_flat_index *h, const uint64_t *example_ids, const size_t *offsets /* [nq + 1] */,
                                  const uint32_t *n_pos /* [nq] */, size_t nq, const size_t *ks, size_t k,
                                  const uint64_t *id_mask, size_t mask_bits, size_t kstride,
                                  uint64_t *out_ids, float *out_dists, float *out_neg_dists, size_t *out_counts);
int vdb_flat_recommend_best_batch_filtered(vdb_flat_index *h, const uint64_t *example_ids, const size_t *offsets /* [nq + 1] */,
                                           const uint32_t *n_pos /* [nq] */, size_t nq, const size_t *ks, size_t k,
                                           const vdb_meta_mask *mask, size_t kstride,
                                           uint64_t *out_ids, float *out_dists, float *out_neg_dists, size_t *out_counts);
int vdb_flat_recommend_best_stats(const vdb_flat_index *h, uint64_t out[8]);
size_t vdb_flat_recommend_best_depth(size_t k, size_t m, size_t len, int stage);
int vdb_flat_debug_set_recommend_best_route(vdb_flat_index *h, int mode);

/*
 * DISCOVERY SEARCH: a target ranked inside context pairs (no reference counterpart; a caller would download the distance columns
 * of 2P + 1 stored vectors over the whole store and fold them on the host).  Request b has a target t, pairs (p_1, n_1) ..
 * (p_P, n_P), 0 <= P <= VDB_DISCOVER_MAX_PAIRS, all stored ids, and a count k_b.  pair_ids holds p_1 n_1 p_2 n_2 ... of every
 * request side by side; request b owns pairs [offsets[b], offsets[b + 1]).  d(e, x) is the reference distance with the stored
 * vector of e as the query and row x as the row: exactly what vdb_flat_search_batch_by_id([e]) reports for x.
 *  - Eligible rows: the live rows the optional mask admits, minus the SET {t, p_i, n_i} (64-bit equality).  An example the mask
 *    hides is still an example; ids may repeat and may stand on both sides of a pair; no id value is a flag.
 *  - rank(x): the number of pairs i with d(p_i, x) < d(n_i, x) under the IEEE <.  A tie is "not satisfied"; a NaN on either side
 *    is "not satisfied" (so a pair whose two ids are equal never is).  The rule is decided row by row and does not depend on
 *    the route the engine took.
 *  - Result: the eligible rows by (rank descending, d(t, x) ascending in the order the plain search gives equal distances --
 *    -0.0 in front of +0.0 --, unsigned id ascending), cut to min(k_b, len): out_ids, out_dists (d(t, x), bit for bit), out_ranks
 *    (may be NULL), out_counts.  Fewer than k_b eligible rows is a short list, not an error.  min(max k_b, len) may not exceed
 *    VDB_DISCOVER_MAX_K.
 * Consequences: P = 0 is vdb_flat_search_batch_by_id bit for bit; with t = p, one pair (p, n) and k = len the rank-1 prefix of
 * the answer is vdb_flat_recommend_best_batch([p], [n]) with k = len, ids and dp bits.
 * Errors, in this order: (1) the argument checks, before any device work: NULL arguments, offsets that do not start at 0 or
 * decrease, more than VDB_DISCOVER_MAX_PAIRS pairs in a request, the stride, the k limit, and a sharded handle -- refused with
 * VDB_ERR_INVALID_ARGUMENT before the flush and before any id is resolved; (2) staged writes are flushed; (3) VDB_ERR_NOT_FOUND
 * and VDB_ERR_DIMENSION_MISMATCH as recommend, over the ids in the order t_b, p_1, n_1, ... request by request; (4) under Cosine a
 * zero-norm example (the target included), like any live zero-norm row, is VDB_ERR_INVALID_VECTOR; (5) a NaN d(t, x) at any live
 * row the mask admits -- the examples included: they are struck afterwards -- is VDB_ERR_NAN, on every route.  A NaN d(p_i, x) or
 * d(n_i, x) is no error: the pair is not satisfied.
 * Not built: a raw-vector target, context-only search without a target, sharded handles (refused as in (1)), device-pointer
 * and ticket forms, HNSW.
 * How (csrc/kernels_discover.hip): the targets of all requests are gathered into one query block on the device
 * and ONE certified search ranks the store for each at depth D; the examples are struck.  What is left is the front of the
 * ranking of the eligible rows by (d(t, x), id): a row outside it sorts behind its last entry.  A kernel finds every candidate's
 * device row, computes the exact d(p_i, x), d(n_i, x) from the stored rows and counts.  A request is answered when k_b candidates
 * have rank P (the first k_b of them are the answer: nothing outside has a higher rank or sorts in front) or when the list is
 * complete -- the search returned fewer rows than D, or D is the whole index --: then the answer is the list's stable sort by rank
 * descending.  The others run again at depth min(len, 1024), and what is left gets ONE exact pass over the rows per request
 * (the rows are read as f32: a SPLIT store converts back first), keyed (P - rank, d(t, x), id rank) in 5 + 32 + 27 bits for the
 * full-scan select; a store of 2^27 rows or more is refused there with VDB_ERR_INVALID_ARGUMENT rather than answered wrongly.
 * vdb_flat_discover_depth(k, P, len, stage) is the search depth D of stage 0 -- min(len, min(1024, max(2 k 2^P' + 2 P' + 1, 64))),
 * k = min(max k_b, len), P' = min(the most pairs of any request, 10): a pair of unrelated examples is satisfied by about half of
 * the rows, so the depth has room for twice the k rows of rank P at that rate and for the examples -- and of stage 1; 0 for any
 * other stage.  vdb_flat_discover_stats describes the last call: [0] requests, [1] example rows (targets included), [2]
 * requests answered at stage 0, [3] at stage 1, [4] by the exact scan, [5] the stage-0 depth, [6] list searches run (one per
 * request and stage it went through), [7] 0.  vdb_flat_debug_set_discover_route (tests): 0 automatic (lists first unless the
 * stage-0 depth is the whole index), 1 lists first always, 2 the exact scan only; the answers are the same bits on every route.
 */
#define VDB_DISCOVER_MAX_PAIRS 16
#define VDB_DISCOVER_MAX_K 1024
int vdb_flat_discover_batch(vdb_flat_index *h, const uint64_t *target_ids /* [nq] */,
                            const uint64_t *pair_ids /* p_1 n_1 p_2 n_2 ..., 2 * offsets[nq] ids */,
                            const size_t *offsets /* [nq + 1], in pairs */, size_t nq, const size_t *ks, size_t k,
                            const uint64_t *id_mask, size_t mask_bits, size_t kstride,
                            uint64_t *out_ids, float *out_dists, uint32_t *out_ranks, size_t *out_counts);
int vdb_flat_discover_batch_filtered(vdb_flat_index *h, const uint64_t *target_ids /* [nq] */, const uint64_t *pair_ids,
                                     const size_t *offsets /* [nq + 1], in pairs */, size_t nq, const size_t *ks, size_t k,
                                     const vdb_meta_mask *mask, size_t kstride,
                                     uint64_t *out_ids, float *out_dists, uint32_t *out_ranks, size_t *out_counts);
int vdb_flat_discover_stats(const vdb_flat_index *h, uint64_t out[8]);
size_t vdb_flat_discover_depth(size_t k, size_t P, size_t len, int stage);
int vdb_flat_debug_set_discover_route(vdb_flat_index *h, int mode);

/*
 * DIVERSE TOP-K (MAXIMAL MARGINAL RELEVANCE): k results that are not all the same thing (no reference counterpart; a caller would
 * search at depth m, get_vector every candidate and run an O(k m dim) loop on the host).  A request is a query q, a count k, a
 * candidate depth m and a trade-off lambda, 1 <= k <= m <= VDB_MMR_MAX_CANDIDATES, lambda an f32 in [0, 1].
 *  1. Candidates: what vdb_flat_search_batch returns for q with depth m under the same mask -- (id_i, d_i), i = 0..c-1, ascending by
 *     (distance, unsigned id), c = min(m, eligible rows); ids, order, distance bits and errors are the search's own.  The POSITION
 *     i in this list is the tie-break of everything below.
 *  2. Pair distance: D(i, j) is DistanceMetric::distance between the stored rows of candidates i and j in the reference's f32
 *     operation order (the exact-order folds; the norms of Cosine are sqrt(sum x*x) in the order of vector.rs:35-37, recomputed
 *     from the rows).  It is symmetric bit for bit under all three metrics.
 *  3. Selection: mu = 1.0f - lambda, computed once on the host in f32.  Pick 1 is candidate 0, its score lambda * d_0 (one
 *     multiply).  After pick s_t, IF another pick follows, D(i, s_t) is evaluated for every candidate i not yet picked, then
 *     near_i = min(near_i, D(i, s_t)) (near_i starts at +inf), then score_i = lambda * d_i - mu * near_i: two multiplies and one
 *     subtraction, each rounded on its own, never contracted.  The next pick is the unpicked candidate with the smallest
 *     (score is NaN, score, position): IEEE < compares the scores, so -0 equals +0, and a NaN score ranks after every number.
 *     The selection stops after min(k, c) picks.
 *  4. Outputs: out_ids / out_dists hold the picks in pick order, out_dists[t] the d of the pick in the bits of the search;
 *     out_scores (may be NULL) the score each pick was chosen with; out_counts[b] = min(k_b, c_b).
 *  5. ks: one k per query, or NULL for k.  The answer for k_b is the first k_b picks of the answer for any larger k at the same m
 *     (greedy selection is prefix-stable) -- except for the NaN rule below, which covers only the pairs the k_b picks evaluate.
 *  6. lambdas: one lambda per query, or NULL for lambda.
 *  7. lambda = 1 returns the first k entries of the plain search, ids and distance bits, whenever the evaluated pair distances are
 *     finite.
 *  8. Errors, in this order.  An empty index or k = 0 (every k of ks) gives counts 0 before any other check.
 *     VDB_ERR_INVALID_ARGUMENT before any device work: a null array; a NaN lambda or one outside [0, 1]; m = 0;
 *     m > VDB_MMR_MAX_CANDIDATES; the largest k above m; a sharded handle (the candidates' rows live on several devices).  Then
 *     everything the search at depth m reports.  Then VDB_ERR_NAN when an EVALUATED pair distance (item 3) is NaN for any query of
 *     the batch.
 *  9. Locking, tickets and flushing are those of vdb_flat_search_batch.  _filtered is the same call under a compiled mask.
 * The selection runs where the rows are: the search's ids come down once, the host's id -> row map turns them into row numbers
 * (under the handle's lock: none can be missing), nq x depth uint32 go up, and mmr_select_kernel (csrc/kernels_mmr.hip), one
 * workgroup per query, runs the k_b dependent steps over rows that never leave HBM.  It evaluates the pairs of item 3 and no
 * others: no m x m matrix exists anywhere.  The direct mapped-memory path of small indexes is not taken.
 * vdb_flat_mmr_stats describes the last call on the handle: [0] queries, [1] the depth the search ran at, [2] candidates summed
 * over the queries, [3] pair distances evaluated = sum_b sum_{t=1}^{count_b - 1} (c_b - t), [4] rows returned, [5] host ns spent
 * turning candidate ids into device rows (download, map, upload), [6], [7] 0.
 */
#define VDB_MMR_MAX_CANDIDATES 1024
int vdb_flat_search_batch_mmr(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                              size_t candidates, const float *lambdas, float lambda,
                              const uint64_t *id_mask, size_t mask_bits, size_t kstride,
                              uint64_t *out_ids, float *out_dists, float *out_scores, size_t *out_counts);
int vdb_flat_search_batch_mmr_filtered(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                       size_t candidates, const float *lambdas, float lambda,
                                       const vdb_meta_mask *mask, size_t kstride,
                                       uint64_t *out_ids, float *out_dists, float *out_scores, size_t *out_counts);
int vdb_flat_mmr_stats(const vdb_flat_index *h, uint64_t out[8]);

/*
 * ONE NEAREST ROW PER GROUP: the k nearest documents, videos, products of a store of chunked items, each represented by its nearest
 * row (no reference counterpart: a caller of Index::search over-fetches by a guessed factor and dedupes on the host, the failure of
 * the 3x post-filter of storage.rs:249-290).  One sentence defines the call: for query q, count k, column `slot` of `table` and an
 * optional id mask, take the FULL ranking of the eligible rows -- what vdb_flat_search_batch returns under that mask with k = len,
 * ascending by (distance, unsigned id) -- walk it from the front, keep a row iff its group code is -1 or no earlier row of the
 * ranking has the same code, stop after k kept rows: ids, order, distance bits, counts and errors.
 *  - Group code of id i: codes[i] of the column as vdb_meta_compile reads it; -1 when the row has no such field or i lies at or
 *    beyond the column's length.
 *  - ROWS WITH CODE -1 ARE NEVER COLLAPSED: each is its own group.  A caller who wants them gone ANDs an EXISTS on the slot into
 *    the filter; the opposite default could not be undone.
 *  - The representative of a group is its first row in the ranking; exact duplicates at one distance are decided by the lower id.  A
 *    mask that removes the representative makes the group's next eligible row the representative.
 *  - out_counts[b] = min(k_b, distinct groups among the eligible rows, each -1 row counting as one).  out_codes (may be NULL)
 *    receives the group code of every returned row, in the layout of out_ids.
 *  - ks: the answer for k_b is the first k_b entries of the answer for max(ks).
 * The result is exact and does not depend on how it was reached.  Stage A searches the batch at depth
 * vdb_flat_distinct_depth(kmax, len, 0) = min(len, min(1024, max(4 kmax, 32))) and collapses every list on the device; a query that
 * kept kmax rows, or whose list came back short, is complete.  Stage B searches the others at vdb_flat_distinct_depth(kmax, len, 1)
 * = min(len, 1024).  Stage C, for a query whose 1024 nearest rows hold fewer than kmax groups, repeats: a mask without the groups
 * already answered is written on the device, the query is searched under it, the new groups are appended -- at most kmax rounds.
 * Errors, all before any device search: a null table or a slot never written, k or max(ks) above 1024, a table (or compiled mask) on
 * another device than the handle's (devices[0] of a sharded handle), an index that has EVER held an id at or above 2^32 (the table
 * cannot describe such ids): VDB_ERR_INVALID_ARGUMENT.  An empty index or k = 0 gives counts 0 before any of these.  Everything else
 * is the error of the equivalent search.  Staged adds and the table's staged column writes are flushed first; the handle's stream
 * is ordered behind the table's by an event.  Locking and tickets as vdb_flat_search_batch; the table stays locked for the call.
 * Plain and sharded handles (the collapse and the exclusion masks run on devices[0]).
 * vdb_flat_distinct_stats describes the last call: [0] queries, [1] completed by stage A, [2] by stage B, [3] by exclusion rounds,
 * [4] exclusion searches run, [5] depth of stage A, [6] depth of stage B, [7] rows returned in total.
 * vdb_flat_distinct_depth needs no handle and no device; any other stage gives 0.
 */
int vdb_flat_search_batch_distinct(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                   vdb_meta_table *table, uint32_t slot, const uint64_t *id_mask, size_t mask_bits, size_t kstride,
                                   uint64_t *out_ids, float *out_dists, int32_t *out_codes, size_t *out_counts);
int vdb_flat_search_batch_distinct_filtered(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                            vdb_meta_table *table, uint32_t slot, const vdb_meta_mask *mask, size_t kstride,
                                            uint64_t *out_ids, float *out_dists, int32_t *out_codes, size_t *out_counts);
int vdb_flat_distinct_stats(const vdb_flat_index *h, uint64_t out[8]);
size_t vdb_flat_distinct_depth(size_t k, size_t len, int stage);

/*
 * THE K NEAREST GROUPS WITH UP TO G ROWS OF EACH: the three best chunks of each of the ten nearest documents, the best offers per
 * product -- what other vector stores call "search groups" (a group-by field, a limit, a group size).  No reference counterpart,
 * and no deeper plain search answers it: the 2nd and 3rd best row of a group are ordinary rows anywhere in the ranking.  One
 * sentence defines the call: for query q, count k, size g = group_size, column `slot` of `table` and an optional id mask, the
 * GROUPS are the first k entries of what vdb_flat_search_batch_distinct returns under the same arguments (ids, order, codes,
 * count), and the MEMBERS of a group with code c >= 0 are the first min(g, E) rows of the full ranking of the eligible rows --
 * vdb_flat_search_batch with k = len under that mask, ascending by (distance, unsigned id) -- restricted to the rows whose code
 * is c, E being the number of eligible rows with that code.
 *  - A row with code -1 is its own group with one member, itself; a row without the field, or with an id at or beyond the column's
 *    length, reads as -1, exactly as vdb_flat_search_batch_distinct reads it.
 *  - Outputs: group j of query b has its members at out_ids / out_dists [(b * kstride + j) * group_size ..], their number in
 *    out_sizes[b * kstride + j], its code in out_codes[b * kstride + j] (out_codes may be NULL); out_counts[b] is the number of
 *    groups.  Member 0 of every group is the group's representative: the id and the distance bits vdb_flat_search_batch_distinct
 *    returns.  On success only the first out_sizes slots of the first out_counts groups are meaningful, the others unspecified.
 *  - All distance bits are the search's own (the reference's f32 operation order); +-inf distances are ordinary members; no id
 *    value is a flag.  group_size = 1 gives vdb_flat_search_batch_distinct's answer bit for bit, with every size 1.
 *  - ks: the answer for k_b is the first k_b groups of the answer for max(ks).
 * How it runs (csrc/kernels_per_group.hip): the search by group runs and leaves its answers on the device; the
 * codes come down in one copy and the host sorts them into the table of wanted codes (vdb_flat_debug_per_group_plan); one pass
 * over the rows -- id, live bit, mask bit and code, 12 bytes per row -- counts every wanted code's eligible rows, a host prefix sum
 * and a second pass write the member lists; one workgroup per (query, group) pair then walks its list in chunks staged through
 * LDS, evaluates every row with the reference's arithmetic and keeps the best g by (distance, id).  A code with more than 131072
 * eligible rows (a capacity limit, that of the sparse and grouped routes) is answered by one ordinary search of its queries at
 * depth g under the mask "caller's mask AND code == c"; results are identical either way.  Nothing survives the call: no list can
 * go stale after an add, a remove, a compaction or a column write.  The first member of every filled group is compared with the
 * representative on the device; a difference is VDB_ERR_DEVICE "internal error".
 * Errors, in this order: an empty index or k = 0 gives counts 0 before any other check; VDB_ERR_INVALID_ARGUMENT before any device
 * work for group_size = 0 or above VDB_PER_GROUP_MAX_SIZE, a NULL out_sizes, out_ids or out_dists, everything
 * vdb_flat_search_batch_distinct refuses, and a sharded handle (the member rows live on several devices; the message says so);
 * then every error of the search by group; a NaN distance met while the members are ranked gives VDB_ERR_NAN.  On any error
 * nothing is written to the outputs.  Locking, flushing, tickets, the table's lock and stream ordering are those of
 * vdb_flat_search_batch_distinct, whose counters (vdb_flat_distinct_stats) describe the first step of this call as well.
 * vdb_flat_per_group_stats describes the last call: [0] queries, [1] groups returned, [2] pairs filled by the member scan, [3] pairs
 * answered by a giant's masked search, [4] distinct wanted codes, [5] member rows listed (the lengths of the lists, summed),
 * [6] pair distances evaluated by the fill, [7] representative mismatches (always 0).
 * vdb_flat_debug_per_group_plan needs no handle and no device: the host plan for the answers' codes [nq][kmax] and kept counts
 * [nq] (clamped to kmax, and to ks[b] where ks is given).  wanted receives the distinct codes >= 0 of the counted entries,
 * ascending (at most cap are written); index [nq][kmax] receives the place of every counted entry's code in that table,
 * 0xffffffff for an entry with code -1 or beyond its count.  wanted and index may be NULL.  Returns the number of wanted codes,
 * (size_t)-1 for a NULL input or kmax above 1024.
 * vdb_flat_debug_set_per_group_scan_cap (tests): the longest list the fill takes on this handle, in rows (0 = the default 131072,
 * which is also the maximum); lower, small indexes take the giants' route.
 */
#define VDB_PER_GROUP_MAX_SIZE 32
int vdb_flat_search_batch_per_group(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                    size_t group_size, vdb_meta_table *table, uint32_t slot, const uint64_t *id_mask,
                                    size_t mask_bits, size_t kstride, uint64_t *out_ids /* [nq][kstride][group_size] */,
                                    float *out_dists /* same shape */, int32_t *out_codes /* [nq][kstride], may be NULL */,
                                    uint32_t *out_sizes /* [nq][kstride] */, size_t *out_counts /* [nq] */);
int vdb_flat_search_batch_per_group_filtered(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks,
                                             size_t k, size_t group_size, vdb_meta_table *table, uint32_t slot,
                                             const vdb_meta_mask *mask, size_t kstride, uint64_t *out_ids, float *out_dists,
                                             int32_t *out_codes, uint32_t *out_sizes, size_t *out_counts);
int vdb_flat_per_group_stats(const vdb_flat_index *h, uint64_t out[8]);
size_t vdb_flat_debug_per_group_plan(const int32_t *codes, const uint32_t *kept, const size_t *ks, size_t nq, size_t kmax,
                                     int32_t *wanted, size_t cap, uint32_t *index);
int vdb_flat_debug_set_per_group_scan_cap(vdb_flat_index *h, size_t rows);

/*
 * ONE BATCH, A FILTER PER QUERY (no reference counterpart: search_batch_with_filter, src/storage.rs:313-322, takes one filter for
 * the batch, while every request of POST /search carries its own, routes.rs:30-35).  One sentence defines the call: the answer for
 * query b is what vdb_flat_search_batch returns for that query ALONE with k_b under mask group_of[b] -- under no mask for
 * VDB_GROUP_NONE: ids, order, distance bits and count, on every route.
 *  - id_masks: n_masks masks of (mask_bits + 63) / 64 words each, one after the other, host memory; layout and eligibility are those
 *    of vdb_flat_search_batch (LSB first, an id at or beyond mask_bits is ineligible, 64-bit ids compared as unsigned).  The
 *    _filtered form takes compiled masks (vdb_meta_compile), each with its own length, all on the handle's device; the handle's
 *    stream is ordered behind the event of every referenced mask and nothing is uploaded.
 *  - group_of[b]: the mask of query b, or VDB_GROUP_NONE.  A mask no query references is never read.
 *  - ks: the answer for k_b is the first k_b entries of the answer for max(ks).
 * The queries that share a mask form a group, and the groups are answered in ONE launch chain, not one per mask (csrc/
 * kernels_grouped.hip): one kernel writes the row mask of every referenced group (a row's id and live bit are read
 * once for all of them), the eligible-row counts E_g of all groups come back in one copy, the host permutes the queries so that a
 * group's are contiguous and plans a table of tiles -- 64 list positions x 64 queries of ONE group -- per pass of 256 queries, one
 * launch writes all eligible-row lists, and per pass one scan (the tile of the sparse-filter route, the reference's operation order)
 * and one select in EMIT mode answer the queries; one launch puts the results back into the caller's order.  Exact by construction.
 * A group with E_g = 0 has counts 0.  Two capacity limits, not tuning: a group with E_g > 131072, and every group when k (clamped to
 * the index's length) exceeds 2048, is answered by one ordinary masked search of its queries; the unfiltered queries by one ordinary
 * search.  The route never consults vdb_flat_set_sparse_filter.
 * Errors, in this order: an empty index or k = 0 gives counts 0 before any check; VDB_ERR_INVALID_ARGUMENT before any device work
 * for a NULL group_of, an index >= n_masks that is not VDB_GROUP_NONE, n_masks > 1024, n_masks > 0 with a NULL mask array or a NULL
 * entry among the referenced masks, a compiled mask on another device; the dimension mismatch of a search; under Cosine one live
 * zero-norm row fails the call, masked or not; a zero-norm query anywhere in the batch gives VDB_ERR_INVALID_VECTOR (before any NaN);
 * a NaN distance at a row eligible FOR THAT QUERY'S MASK gives VDB_ERR_NAN -- a NaN row only other groups admit does not.
 * Locking and tickets as vdb_flat_search_batch: refused while a submitted search is outstanding; staged adds are flushed first.
 * Not available on a sharded handle.
 * vdb_flat_grouped_stats describes the last call: [0] queries, [1] masks referenced, [2] queries answered by the grouped scan, [3] by
 * a per-group ordinary search, [4] unfiltered queries, [5] eligible rows summed over the scanned groups, [6] tiles launched, [7] passes.
 * vdb_flat_debug_group_plan needs no handle and no device: the plan for group_of and the eligible-row counts elig[n_masks] at
 * k <= 2048.  perm[i] = the caller's index of permuted query i (scanned groups first, then the groups with nothing eligible, the
 * groups beyond the capacity, the unfiltered queries; a group's queries contiguous and in the caller's order); tiles[t] = {group,
 * first list position, first permuted query, queries}; pass of a tile = first permuted query / 256.  Returns the number of tiles
 * (at most cap are written; perm and tiles may be NULL), (size_t)-1 for a bad group index.
 */
#define VDB_GROUP_NONE 0xffffffffu      /* this query is searched without a filter */
int vdb_flat_search_batch_grouped(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                  const uint64_t *id_masks, size_t n_masks, size_t mask_bits, const uint32_t *group_of,
                                  size_t kstride, uint64_t *out_ids, float *out_dists, size_t *out_counts);
int vdb_flat_search_batch_grouped_filtered(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, const size_t *ks, size_t k,
                                           const vdb_meta_mask *const *masks, size_t n_masks, const uint32_t *group_of,
                                           size_t kstride, uint64_t *out_ids, float *out_dists, size_t *out_counts);
int vdb_flat_grouped_stats(const vdb_flat_index *h, uint64_t out[8]);
size_t vdb_flat_debug_group_plan(const uint32_t *group_of, size_t nq, const uint32_t *elig, size_t n_masks, uint32_t *perm,
                                 uint32_t *tiles, size_t cap);

/*
 * Opt-in bf16 SHADOW of the rows for the screening pass (no reference counterpart; results are identical with and without
 * it).  on = 1: the index keeps, next to the f32 rows, their bf16 roundings (+50 % device memory: 2 bytes per element on top
 * of 4) -- exactly the values the screening kernel otherwise produces in registers -- and the filter pass streams THOSE:
 * half the HBM bytes per batch (csrc/kernels_fused_s16.hip).  The exact re-rank, the f32 tier and the exact scan keep
 * reading the f32 rows, so the returned ids and distances do not change by a bit.  Used when the padded row length is a
 * multiple of 64 elements (otherwise the f32-row pass runs as before).  Existing rows are converted by this call, later
 * adds at their flush.  on = 0 frees the shadow.  last_stats_ex()[14] = 1 when the last search used it.
 */
int vdb_flat_set_shadow(vdb_flat_index *h, int on);

/*
 * The screening tier's SAMPLE CACHE (on by default; no reference counterpart; results identical either way).  The tier
 * derives its per-query filter thresholds from the scores of S <= 65536 sample rows spread over the index.  With the cache
 * the index keeps a compact bf16 copy of exactly those rows (S * padded dimension * 2 bytes: 100 MB beside a 3 GB index;
 * S <= max(16384, rows / 8), so never more than an eighth of the f32 store),
 * rebuilt by the first search after rows were added, and the sample pass streams it instead of gathering the rows from
 * the f32 store: half the bytes, contiguous.  Same roundings, same MFMA order -> the same thresholds, bit for bit.
 * Used when the padded row length is a multiple of 64 elements.  on = 0 frees the copy and restores the f32 gather.
 */
int vdb_flat_set_sample_cache(vdb_flat_index *h, int on);

/* Test hook (no reference counterpart; results are identical whatever the flags): force the hand-over of queries to
 * the slower tiers so that every tier can be compared with every other on the same index.  Not read from the
 * environment -- the release library has no getenv on any path. */
#define VDB_TIERS_NO_RETHRESHOLD 1u /* skip the re-threshold pass: uncertified queries go straight to the f32 MFMA tier (k <= 112) or the exact scan */
#define VDB_TIERS_FORCE_F32 2u      /* hand EVERY query the screening tier answered to the f32 MFMA tier as well */
#define VDB_TIERS_FORCE_EXACT 4u    /* hand every query to the exact scan */
#define VDB_TIERS_NO_DIRECT 8u      /* small indexes (<= 16384 rows), batches of <= 8 queries: the tiered pipeline instead of the direct exact scan */
#define VDB_TIERS_FORCE_RETHRESHOLD 16u /* hand every query the screening tier answered to the re-threshold pass as well (small and large k); a query
                                         * without a finite score cut or with a pool overflow goes on as an uncertified one does.  Ignored together
                                         * with FORCE_F32, FORCE_EXACT or NO_RETHRESHOLD */
int vdb_flat_set_tiers(vdb_flat_index *h, unsigned flags);

/*
 * Diagnostics of the screening tier's CERTIFICATE (tests/test_gpu_certificate.py).  The default tier ranks rows by
 * bf16-MFMA scores and returns exact f32 distances only because a bound on the score error proves that no excluded row
 * can enter the top k.  These entry points expose the inputs of that proof so that it can be tested
 * directly instead of end to end.  They do not alter any search.
 *
 * vdb_flat_debug_screen_scores: runs query preparation and the PRODUCTION filter kernel over every live row with
 * thresholds that let everything pass, and returns the ranking score of every (query, row) pair:
 *   out_scores [nq][rows uploaded] f32 (the NaN pattern 0xffffffff = no key: tombstoned row); nq <= 256 (512 with VDB_DEBUG_SCORES_WIDE);
 *   raw = 0: the scores the tier ranks by (Dot / Euclid: lower-bound scores, score - g_q * margin_row);
 *   raw = 1: the plain scores fma(acc, alpha, beta) (under Dot: -acc, the raw MFMA accumulator);
 *   raw = 2: the f32 MFMA TIER's scores (v_mfma_f32_32x32x2_f32; dense_scores_kernel over every row, bit-identical to the
 *            fused f32 kernel's); a following cert_probe then evaluates the f32 tier's certificate (eps_coef only);
 *   raw | VDB_DEBUG_SCORES_SPLIT (with raw 0 or 1): the scores a search over SPLIT rows ranks by.  An F32 store is converted first
 *            (whatever vdb_flat_set_split says; the adaptive run of mode 1 is neither fed nor reset; vdb_flat_layout counts the
 *            conversion) and stays SPLIT; the filter pass reads the store as it lies.  VDB_ERR_INVALID_ARGUMENT, the rows left as
 *            they were, when the store cannot be SPLIT (pitch not a multiple of 64 or above 16384, no rows), when the index keeps
 *            a usable bf16 shadow (the filter pass would read that), or with raw 2 (the f32 tier reads f32 rows).  Rows with a
 *            non-finite element: refused as well, after the one attempt a search would make (forward, found out, straight back).
 *            Without the bit a SPLIT store is converted back first;
 *   raw | VDB_DEBUG_SCORES_WIDE (with raw 0 or 1): the WIDE filter kernel (512 queries per fetch of the rows, batches above 256
 *            queries) over f32 rows, launched as a search launches it: 256 < nq <= 512, the two 256-query blocks' pools turned
 *            into their halves of the dump.  VDB_ERR_INVALID_ARGUMENT with nq <= 256 (no search runs it there), with a usable
 *            shadow, with raw 2 or together with VDB_DEBUG_SCORES_SPLIT; VDB_ERR_DEVICE if a sub-pool counted more keys than it
 *            holds (the dump would have holes);
 *   out_qinfo [nq][4]: exact-order |q|, the bound on |q - bf16(q)|, g_q, 0;
 *   out_consts [8]: eps_coef, c_acc, kappa, max |d|, max |d - bf16(d)|, max |d - bf16(d)|/|d|, 1 if lower-bound scores, ld.
 * vdb_flat_debug_rows: number of device rows.  vdb_flat_debug_row_info: out [rows][4] = exact-order |d|, alpha, beta, margin (0 under Cosine).
 * vdb_flat_debug_cert_probe: out[i] = the production certification test (kernels_aux.hip cert_test) for prepared query
 *   qi[i] of the last debug_screen_scores call, unexamined-row score bound T[i] and k-th exact distance ek[i].
 *   Soundness means: probe(T = score of row r, ek = exact distance of row r) is 0 for EVERY pair.
 */
#define VDB_DEBUG_SCORES_SPLIT 4 /* OR-ed into raw: over SPLIT rows */
#define VDB_DEBUG_SCORES_WIDE 8  /* OR-ed into raw: the 512-query kernel */
int vdb_flat_debug_screen_scores(vdb_flat_index *h, const float *queries, size_t nq, size_t dim, int raw,
                                 float *out_scores, float *out_qinfo, double *out_consts);
size_t vdb_flat_debug_rows(const vdb_flat_index *h); /* device rows incl. tombstoned ones (row i = i-th row added since the last reset or vdb_flat_compact: a compaction renumbers the rows) */
int vdb_flat_debug_row_info(vdb_flat_index *h, float *out, size_t n_rows);
/* the per-query filter thresholds of the screening tier as the LAST search on this handle derived them from its sample pass (first nq queries) */
int vdb_flat_debug_last_thresholds(vdb_flat_index *h, float *out, size_t nq);
int vdb_flat_debug_cert_probe(vdb_flat_index *h, const uint32_t *qi, const float *T, const float *ek, size_t n,
                              uint32_t *out);

/* Diagnostics of vdb_flat_compact (tests).  vdb_flat_debug_compact_plan needs no handle and no device: for a live mask
 * (bit r & 31 of word r >> 5 = row r alive; bits at and above n_rows clear) it returns the number of chunks the compaction
 * moves and writes the first `cap` of them to out as [first source row, end source row, first destination row, mode]
 * (mode 0 = moved directly, 1 = through the bounce buffer); bounce_rows = 0 means the default for rows of `ld` floats.
 * vdb_flat_debug_set_compact_bounce: the bounce buffer of this handle in rows (rounded down to 32, at least 32; 0 = default),
 * so that small indexes exercise many chunks.  Results are identical whatever the value. */
size_t vdb_flat_debug_compact_plan(const uint32_t *live, size_t n_rows, size_t bounce_rows, size_t ld, uint32_t *out, size_t cap);
int vdb_flat_debug_set_compact_bounce(vdb_flat_index *h, size_t rows);

/* Thread-local message of the last failing call on this thread, plus the
 * DimensionMismatch pair (error.rs:12-13).  Any pointer may be NULL. */
void vdb_last_error(char *buf, size_t cap, size_t *expected, size_t *actual);

/* Library/ABI version and the GPU architecture the kernels were built for ("gfx950"). */
int vdb_abi_version(void);
const char *vdb_build_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* VDB_FLAT_H */
