/*
 * vdb_ivf.h — C ABI of the MI355X-native IVF-Flat engine (libvdb_ivf.so).
 *
 * This is the drop-in boundary for the reference's search path. Each entry point
 * names the reference interface it replaces (paths relative to the reference
 * repository, wedevxer/CUDA-AcceleratedVectorDatabaseEngine):
 *
 *   vdb_ivf_create        IVFFlatIndex::IVFFlatIndex(const Config&, TransferManager*)   engine/ivf_flat_index.h:44, .cpp:13-33
 *   vdb_ivf_destroy       IVFFlatIndex::~IVFFlatIndex()                                 engine/ivf_flat_index.h:45, .cpp:36-46
 *   vdb_ivf_train         IVFFlatIndex::train(const float*, uint64_t)                   engine/ivf_flat_index.h:47, .cpp:49-145
 *   vdb_ivf_add           IVFFlatIndex::add(const float*, const uint64_t*, uint64_t)    engine/ivf_flat_index.h:49, .cpp:148-202
 *   vdb_ivf_search        IVFFlatIndex::search(const float*, uint32_t, const SearchParams&, float*, uint64_t*)
 *                                                                                       engine/ivf_flat_index.h:51-53, .cpp:205-256
 *   vdb_ivf_warmup        IVFFlatIndex::warmup_lists(const std::vector<uint32_t>&)      engine/ivf_flat_index.h:60
 *   vdb_ivf_evict         IVFFlatIndex::evict_list(uint32_t)                            engine/ivf_flat_index.h:61
 *   vdb_ivf_gpu_bytes     IVFFlatIndex::get_gpu_memory_usage()                          engine/ivf_flat_index.h:63, .cpp:707-709
 *   vdb_ivf_ntotal        IVFFlatIndex::get_total_vectors()                             engine/ivf_flat_index.h:64
 *
 * The remaining entry points have no single reference counterpart; they expose the
 * device-resident and multi-GPU forms of the same path (the reference searches one
 * query and one list at a time on device 0, ivf_flat_index.cpp:214-255).
 *
 * Conventions: every call returns 0 on success and a negative code on failure;
 * vdb_last_error() then describes the failure (thread-local). Host buffers are
 * caller-owned and row-major (queries n x dim fp32; outputs n x k). Metric
 * ordinals follow kernels::Metric (engine/kernels.cuh:24-28): L2 = 0 (squared
 * L2), InnerProduct = 1 (negated dot), Cosine = 2 (the reference CPU path leaves
 * its distance at 0.0f, ivf_flat_index.cpp:351-362; mirrored exactly);
 * CosineDistance = 3 is this engine's own (true cosine distance, see below).
 * Unfilled result slots are (FLT_MAX, UINT64_MAX) as in ivf_flat_index.cpp:513-517.
 * Results are bit-identical to the reference CPU path (ids and distance bits).
 * No torch or HIP types appear in these signatures; streams are passed as void*.
 */
#ifndef VDB_IVF_H
#define VDB_IVF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    VDB_OK = 0,
    VDB_ERR_INVALID_ARGUMENT = -1,
    VDB_ERR_DEVICE = -2,
    VDB_ERR_OUT_OF_MEMORY = -3,
    VDB_ERR_UNSUPPORTED = -4,
    VDB_ERR_STATE = -5
};

enum { VDB_METRIC_L2 = 0, VDB_METRIC_INNER_PRODUCT = 1, VDB_METRIC_COSINE = 2, VDB_METRIC_COSINE_DISTANCE = 3 };

/*
 * VDB_METRIC_COSINE_DISTANCE (3): true cosine distance, 1 - cos(query, row). Ordinal 2 keeps the
 * reference CPU path's behaviour (0.0f everywhere), bit for bit.
 *
 * Definition. A handle created with metric 3 is an inner-product handle over UNIT ROWS: every
 * row is normalised once when it enters the index (train, add, add_device, add_to_lists,
 * add_to_lists_device, assign_device, a group's add), every query when it enters a batch, and
 * every filled result distance d (the inner-product handle's -dot) is reported as 1.0f + d, one
 * fp32 add. Every call's result is exactly the result of the same call on an InnerProduct handle
 * with the same centroids that stores unit(row) for each row and is asked unit(query), each
 * distance whose id is not UINT64_MAX then replaced by 1.0f + d; unfilled slots stay
 * (FLT_MAX, UINT64_MAX). Order, the unique-id merge, stale_slots, nprobe clamping, k limits and
 * the refusals are the InnerProduct handle's, unchanged. The screened scan, the list-cache tier
 * (host home, or vdb_ivf_open_lists of a plain metric-3 file), groups, remove_ids, filters and
 * prepared filters serve it as they serve inner product.
 *
 * Order. Entries stay ordered by (-dot, id); they are NOT re-sorted by the mapped value.
 * fl(1 + d) is monotone but collapses neighbours: two entries with distinct -dot may report
 * equal distances, and then stand in -dot order, not id order.
 *
 * unit(x), fixed so that a host restatement gives the same bits (tests/cosine_ref.py): with
 * j = i / 4, element i belongs to lane j % 64; a lane adds the squares of its elements in
 * ascending i (fp32, product rounded, then sum rounded, no fused multiply-add); the 64 partials
 * combine by p[l] += p[l + s] for s = 32, 16, 8, 4, 2, 1; norm = sqrt of that sum, correctly
 * rounded; if norm is finite and > 0 every element becomes x[i] / norm (a correctly rounded
 * division), otherwise (a zero row, an overflowing sum, a NaN) the row is kept as it is.
 * Denormal intermediates are unspecified. This deliberately differs from the reference's
 * unported GPU functor (kernels.cuh:63-80), which adds 1e-8 to a per-pair product of norms.
 *
 * Stored rows. vdb_ivf_get_list, save files and the tier's homes hold unit rows. unit() is not
 * idempotent bit for bit, so rows are normalised exactly once: vdb_ivf_load stores a file's rows
 * as they are. vdb_ivf_train runs the reference algorithm on the unit rows and then normalises
 * the final centroids (spherical k-means' last step; a zero centroid stays zero);
 * vdb_ivf_set_centroids stores what it is given. A save file records metric 3: it loads only
 * into a metric-3 handle, and no L2 / InnerProduct / Cosine file loads into one.
 *
 * Range search. The radius is in reported distances: the scan thresholds -dot at the largest
 * fp32 t with fl(1.0f + t) <= radius, and returned distances are 1.0f + d.
 *
 * Refused in this version with VDB_ERR_UNSUPPORTED, the handle untouched: vdb_ivf_set_shard*,
 * vdb_ivf_plan_shard*, vdb_ivf_attach_comm and opening a shard file. A sharded rank hands out
 * partials the caller merges by (distance, id) with vdb_merge_ranks_*; mapped distances would
 * merge in another order than one GPU gives.
 */

typedef struct vdb_ivf vdb_ivf;

/* Mirrors IVFFlatIndex::Config (engine/ivf_flat_index.h:16-22) plus the device. */
typedef struct vdb_ivf_config {
    uint32_t dimension;
    uint32_t nlist;
    int32_t metric;
    int32_t use_gpu;          /* accepted for API parity; the engine always runs on the GPU */
    uint64_t max_gpu_memory;  /* HBM cap on resident list bytes (count * (dim * 4 + 8) per list, the
                                 reference's gpu_memory_used_, ivf_flat_index.cpp:398-402). Once an add
                                 takes the lists above it, the handle switches to the list-cache tier
                                 with an HBM cache of this many bytes (lists home in page-locked host
                                 memory; results unchanged); lifting or raising the cap above the lists
                                 brings them back. Only list bytes count: the screen's bf16 shadow
                                 (about half the list bytes) is not list data. 0 = no cap: every list
                                 HBM-resident (288 GB per GPU). The reference searches lists that do
                                 not fit on the CPU; here an exact-path search (k > 64, Cosine, screen
                                 off) whose single query probes more than the cap fails with
                                 VDB_ERR_OUT_OF_MEMORY; the screened tier loads no list. */
    int32_t device;           /* HIP device ordinal */
} vdb_ivf_config;

/* Per-handle measurement, filled by vdb_ivf_profile_read (see DESIGN.md "Measurement"). */
typedef struct vdb_ivf_profile {
    uint64_t batches;          /* search batches executed since the last reset */
    uint64_t scan_launches;    /* ivf_scan kernel launches */
    double scan_ms;            /* summed ivf_scan durations (HIP events on the search stream) */
    double coarse_ms;          /* summed coarse-quantiser durations (distance + select) */
    double total_ms;           /* summed per-batch durations (first to last kernel) */
    uint64_t scan_vectors;     /* sum over batches of sum_{distinct probed local lists} n_l */
    uint64_t distinct_lists;   /* sum over batches of distinct probed local lists */
    uint64_t work_items;       /* sum over batches of scan work items */
    uint64_t scan_bytes;       /* algorithmic bytes read by ivf_scan: 4 * dim * scan_vectors */
    uint64_t pair_vectors;     /* sum over batches and (query, probe) pairs of n_l: distances computed */
    uint64_t exact_reranks;    /* screened / bounded scan: (query, vector) distances recomputed exactly (option bounded_stats) */
    uint64_t bounded_blocks;   /* screened / bounded scan: 64-vector blocks bounded on the matrix cores (option bounded_stats) */
    uint64_t computed_vectors; /* query slots the scan streams per vector: pair_vectors plus one per
                                  odd wide group (its last query runs alone, on scalar ops) */
    double local_merge_ms;     /* summed per-batch merges after the scan (segment, slot, query top-k) */
    uint64_t exchanges;        /* multi-GPU: exchanges timed below */
    double exchange_ms;        /* summed: this rank's results ready -> all-gather done (the wait for the
                                  slowest rank plus the collective itself) */
    double rank_merge_ms;      /* summed: all-gather done -> final results merged */
    uint64_t screen_collected; /* deferred screened scan: (query, vector) pairs collected against the
                                  upper-bound thresholds (option bounded_stats); exact_reranks counts
                                  the survivors of each pair's final threshold, recomputed exactly */
    double collect_ms;         /* deferred screened scan: summed durations of its collect kernel (the
                                  stream of the bf16 shadow; scan_ms covers it and the re-check kernels) */
    double recheck_ms;         /* ... and of the final thresholds, selection and exact re-checks after it */
    uint64_t screen_floor_batches; /* batches the run-time floor ran on the exact scan */
    uint64_t screen_floor_trips;   /* screened batches that tripped the floor */
    uint32_t screen_shadow;        /* the screen's shadow now: 0 none, 1 bf16, 2 int8 (option screen_i8) */
    uint32_t reserved0;
} vdb_ivf_profile;

const char* vdb_last_error(void);
const char* vdb_version(void);
/* Hash of the sources that shape the scan kernels and their launches (16 hex digits):
 * measurements (PMC traffic) are tied to the library they were taken on. */
const char* vdb_build_id(void);
int vdb_device_count(int* count);

int vdb_ivf_create(const vdb_ivf_config* config, vdb_ivf** out);
int vdb_ivf_destroy(vdb_ivf* index);

/* Training (k-means++ seeded with mt19937(42), then 10 Lloyd iterations), exactly
 * the reference algorithm; distances run on the GPU. */
int vdb_ivf_train(vdb_ivf* index, const float* vectors, uint64_t n);
int vdb_ivf_train_device(vdb_ivf* index, const float* d_vectors, uint64_t n);
int vdb_ivf_set_centroids(vdb_ivf* index, const float* centroids);  /* nlist x dim, host */
int vdb_ivf_get_centroids(vdb_ivf* index, float* centroids);        /* nlist x dim, host */

/* add: exact nearest-centroid assignment, lists appended in input order. */
int vdb_ivf_add(vdb_ivf* index, const float* vectors, const uint64_t* ids, uint64_t n);
int vdb_ivf_add_device(vdb_ivf* index, const float* d_vectors, const uint64_t* d_ids, uint64_t n);

/* Append rows to explicitly given lists (no assignment), input order kept per list.
 * Used by vdb_ivf_load and for indexes whose assignment was computed elsewhere. */
int vdb_ivf_add_to_lists(vdb_ivf* index, const float* vectors, const uint64_t* ids, const uint32_t* lists,
                         uint64_t n);
/* Exact assignment only (assign_to_lists, engine/ivf_flat_index.cpp:259-295): one list id
 * per row into a device array, nothing stored. With add_to_lists_device it splits `add`
 * (cpp:148-202) into two passes, so a sharded build can learn the final list sizes first. */
int vdb_ivf_assign_device(vdb_ivf* index, const float* d_vectors, uint64_t n, uint32_t* d_lists);
int vdb_ivf_add_to_lists_device(vdb_ivf* index, const float* d_vectors, const uint64_t* d_ids,
                                const uint32_t* d_lists, uint64_t n);
/* Remove every stored row whose id is one of ids[0..n) (host array). All rows carrying a
 * listed id go (an index may hold an id more than once); ids that are not stored, and
 * repeats within ids[], are ignored. The surviving rows of every list keep their order, so
 * the handle is afterwards indistinguishable from one given the same centroids and the
 * surviving rows in their original add order. *removed (may be NULL) receives the number of rows
 * removed. Centroids are unchanged; a list may become empty.
 * No counterpart in the reference (it cannot delete). The lists are compacted on the device
 * into a fresh arena (peak memory old + new arena, the cost class of one add; the rows never
 * travel through the host); searches in flight are quiesced first, as by add, and the next
 * search rebuilds the screen. When n == 0 or no stored row matches, nothing is reallocated or
 * rebuilt. Pad slots are never matched, whatever ids[] holds. n >= 2^31: VDB_ERR_UNSUPPORTED.
 * Lists served from a file (vdb_ivf_open_lists): VDB_ERR_STATE, read-only as for add. If the
 * fresh arena cannot be allocated: VDB_ERR_OUT_OF_MEMORY, the lists unchanged. A group handle
 * removes on every member (*removed is the sum; list ownership does not change). A sharded
 * handle (world > 1: vdb_ivf_set_shard, vdb_ivf_plan_shard, an opened shard file, an attached
 * communicator) gives VDB_ERR_UNSUPPORTED and is left untouched: a rank cannot see ids in
 * lists it does not store, and the ranks' list sizes must stay equal for vdb_ivf_attach_comm. */
int vdb_ivf_remove_ids(vdb_ivf* index, const uint64_t* ids, uint64_t n, uint64_t* removed);
/* Diagnostics: the calling thread's latest vdb_ivf_remove_ids on a single-device handle, by
 * step: the mark kernel and the compact kernel (HIP events), the host plan between them, and
 * the rows the compact pass moved. Any pointer may be NULL. */
int vdb_remove_last_timing(double* mark_ms, double* plan_ms, double* compact_ms, uint64_t* rows_kept);
/* Upsert: replace the rows of ids that are stored and insert the others, in one call. No
 * counterpart in the reference (it can neither delete nor change a row).
 * Winners: the winners W of a request are, for every distinct id in ids[0..n), the entry with
 * the largest index carrying it (last write wins); W stays in request order.
 * After the call the handle is indistinguishable from the same handle after
 * vdb_ivf_remove_ids(all request ids) followed by vdb_ivf_add(rows of W, ids of W): totals, list
 * sizes, every list's ids and row bits in vdb_ivf_get_list order, and every search result. So:
 * every stored copy of a listed id goes (an index may hold an id more than once); survivors
 * keep their order in each list; each winner is assigned by the exact nearest-centroid
 * assignment of add and appended after its list's survivors, in request order; a row whose new
 * vector lands in the list it was in still moves to that list's end. Centroids do not change; a
 * list may become empty. No id value is special, and pad slots are never matched.
 * *replaced receives the number of stored rows removed, *inserted |W|; either may be NULL. With
 * VDB_METRIC_COSINE_DISTANCE the winners are normalised once, as add normalises them.
 * n == 0 succeeds and leaves the handle untouched (prepared filters stay live,
 * vdb_ivf_gpu_bytes_allocated is unchanged). A request none of whose ids is stored is exactly an
 * add of W, as is any request on a trained, empty index. Any call with n > 0 makes the handle's
 * prepared filters stale. Searches in flight are quiesced first, as by add, and the next search
 * rebuilds the screen; the call holds the handle's lock and has finished its device work when it
 * returns.
 * The request is resolved on the device (a stable sort of (id, position), the winners marked
 * and packed densely), and the lists are rebuilt once: the survivors are compacted into one
 * fresh arena sized for survivors and winners, and the winners scattered behind them (peak
 * memory old arena + that arena; the sequence of the two calls allocates and fills an arena
 * twice). The rows never travel through the host after the host variant's upload.
 * vdb_ivf_upsert_device is the same on buffers of the handle's device that are complete before
 * the call (replaced and inserted stay host pointers).
 * The list-cache tier with its home in host memory is served as remove serves it: an upsert that
 * grows the lists past max_gpu_memory switches the handle into the tier, one that shrinks them
 * below the cap brings them back.
 * Refusals leave the handle untouched: a null handle, or null vectors / ids with n > 0, give
 * VDB_ERR_INVALID_ARGUMENT before any device call; n >= 2^31 VDB_ERR_UNSUPPORTED; lists served
 * from a file (vdb_ivf_open_lists) VDB_ERR_STATE, read-only as for add; a sharded handle (world >
 * 1 by any route) VDB_ERR_UNSUPPORTED, for remove's reason; a group handle VDB_ERR_UNSUPPORTED. An
 * untrained handle gets what vdb_ivf_add gives it. If the fresh arena cannot be allocated:
 * VDB_ERR_OUT_OF_MEMORY, the lists unchanged. Not offered yet: a group handle, the gRPC service,
 * a caller's stream for the device variant. */
int vdb_ivf_upsert(vdb_ivf* index, const float* vectors, const uint64_t* ids, uint64_t n,
                   uint64_t* replaced, uint64_t* inserted);
int vdb_ivf_upsert_device(vdb_ivf* index, const float* d_vectors, const uint64_t* d_ids, uint64_t n,
                          uint64_t* replaced, uint64_t* inserted);
/* Diagnostics: the calling thread's latest vdb_ivf_upsert(_device), by step: the resolution of
 * the request (sort, winners, pack), the mark kernel, and the move (the compact of the survivors
 * and the scatter of the winners) by HIP events, the host plan between them, the stored rows the
 * compact moved and the winners written. Any pointer may be NULL; a thread without a call, and a
 * call with n == 0, read zeros. */
int vdb_upsert_last_timing(double* resolve_ms, double* mark_ms, double* plan_ms, double* move_ms,
                           uint64_t* rows_kept, uint64_t* rows_written);
/* Filtered search: vdb_ivf_search over the stored rows an id filter allows. filter_ids[0..
 * n_filter) is a host array in any order; repeats and ids that are not stored are ignored.
 * VDB_FILTER_EXCLUDE: a stored row is allowed unless its id is listed (tombstones: n_filter
 * == 0 is valid and equals vdb_ivf_search). VDB_FILTER_INCLUDE: a stored row is allowed only
 * if its id is listed (pre-filtering; nothing allowed: every slot unfilled). Pad slots are
 * never allowed, whatever filter_ids holds. Host buffers in and out, as for vdb_ivf_search.
 * The result is, bit for bit (ids and distance bits), the one vdb_ivf_search(n, nprobe, k)
 * gives on a handle with the same centroids, metric and stale_slots setting that stores only
 * the allowed rows in their original order: probe selection unchanged (centroids only, nprobe
 * clamped to nlist), per list the top-k by (distance, id), the unique-id merge over the slots,
 * (FLT_MAX, UINT64_MAX) in unfilled slots; with stale_slots = 1 a slot whose list has no
 * allowed row keeps the content of the latest earlier query of the call whose probe at that
 * slot had one. Results never depend on the `batch` option. Cosine is served (every distance
 * 0.0f, ties by id).
 * No counterpart in the reference. Nothing moves and nothing is rebuilt: the allow masks are
 * taken per call from the ids, a masked exact scan computes the allowed rows' distances only
 * (the screen is not used: its shadow and thresholds describe whole lists), and the handle is
 * left exactly as found. The call holds the handle's lock and has finished its device work
 * when it returns.
 * Limits of this version (the handle is untouched by a refusal): k > 64 and n_filter >= 2^31
 * give VDB_ERR_UNSUPPORTED; an invalid mode or a null buffer VDB_ERR_INVALID_ARGUMENT; a handle
 * in the list-cache tier (option list_cache_bytes, or max_gpu_memory exceeded), a file-home
 * handle (vdb_ivf_open_lists), a sharded handle (world > 1) and a group handle give
 * VDB_ERR_UNSUPPORTED. A filter many calls share is prepared once with vdb_ivf_filter_create
 * (below), which also takes the ids from the device. Not offered yet: the gRPC service,
 * coalescing of concurrent filtered calls (queries under different prepared filters share one
 * call through vdb_ivf_search_prepared_multi, below). */
enum { VDB_FILTER_EXCLUDE = 0, VDB_FILTER_INCLUDE = 1 };
int vdb_ivf_search_filtered(vdb_ivf* index, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                            const uint64_t* filter_ids, uint64_t n_filter, int mode,
                            float* distances, uint64_t* ids);
/* Diagnostics: the calling thread's latest vdb_ivf_search_filtered, by step (HIP events: the
 * mark and count kernels; the masked scan and the merge, each summed over the call's
 * batches), and the (query, row) distances computed. Any pointer may be NULL. */
int vdb_filter_last_timing(double* mark_ms, double* scan_ms, double* merge_ms, uint64_t* pairs_scanned);
/* Range search: every stored row within `radius` of each query (FAISS: range_search). For each
 * of the n host queries on its own, the result holds every entry (d, id) of the result
 * vdb_ivf_search gives that single query with the same nprobe and a k no smaller than the rows
 * it probes, keeping the entries with id != UINT64_MAX and d <= radius, in that result's order:
 * probe selection unchanged (centroids only, nprobe clamped to nlist); distances the
 * reference's sequential fp32 sums, bit for bit (L2 squared, inner product negated, Cosine
 * 0.0f for every row); the comparison the fp32 d <= radius, inclusive (a NaN distance is never
 * returned; +inf and FLT_MAX return every probed row); an id stored more than once among the
 * probed lists once, at its smallest distance; a query's entries ascending by (distance, id),
 * -0.0f and +0.0f equal and tied by id, the returned bits the computed ones. The result depends
 * on neither stale_slots nor batch; pad slots are never returned.
 * The size of the answer is not known before the call, so the library owns it: *out (written
 * only on success) holds host memory alone, nothing of the handle, outlives it, and is released
 * with vdb_range_result_free (NULL is fine). Query i owns entries [lims[i], lims[i + 1]) of
 * distances and ids; lims has n + 1 entries. n == 0 gives lims = {0}; an empty index or nprobe
 * == 0 all-zero lims.
 * reserve is the capacity, in entries, of the device hit buffer a batch starts with (about 56
 * bytes of device workspace per entry); 0 chooses 262,144. A batch that finds more hits than the
 * buffer holds is scanned once more with a buffer of the size it counted (at most one re-run
 * per batch; results are identical).
 * Nothing moves and nothing is rebuilt: a thresholded exact scan appends the hits, three stable
 * device sorts order and de-duplicate them, and the handle is left exactly as found (the screen
 * is not used). The call holds the handle's lock and has finished its device work when it
 * returns.
 * Limits of this version (the handle is untouched by a refusal): a null handle, queries or out
 * and a NaN radius give VDB_ERR_INVALID_ARGUMENT; a handle in the list-cache tier, a file-home
 * handle, a sharded handle and a group handle give VDB_ERR_UNSUPPORTED, as does a batch with
 * more than 2^31 - 1 hits (lower the `batch` option). A filter combined with a radius is
 * vdb_ivf_range_search_prepared, the same result through the screen vdb_ivf_range_search_screened
 * (both below). Not offered yet: per-query radii, a device-pointer variant, the gRPC service,
 * coalescing of concurrent range calls. */
typedef struct vdb_range_result vdb_range_result;
int vdb_ivf_range_search(vdb_ivf* index, const float* queries, uint32_t n, uint32_t nprobe, float radius,
                         uint64_t reserve, vdb_range_result** out);
uint32_t vdb_range_result_n(const vdb_range_result* r);
const uint64_t* vdb_range_result_lims(const vdb_range_result* r);      /* n + 1 entries; query i owns [lims[i], lims[i+1]) */
const float* vdb_range_result_distances(const vdb_range_result* r);    /* lims[n] entries */
const uint64_t* vdb_range_result_ids(const vdb_range_result* r);
void vdb_range_result_free(vdb_range_result* r);                       /* NULL is fine */
/* Diagnostics: the calling thread's latest vdb_ivf_range_search (HIP events summed over the
 * call's batches, re-runs included): the scan with the pair grouping, the ordering (sorts,
 * de-duplication, per-query counts), the (query, row) distances computed, the entries returned
 * and the batches run again. Any pointer may be NULL; a thread without a call reads zeros. */
int vdb_range_last_timing(double* scan_ms, double* order_ms, uint64_t* pairs_scanned, uint64_t* hits,
                          uint32_t* reruns);
/* Prepared filters: the allow masks vdb_ivf_search_filtered takes from its ids on every call,
 * taken once and kept on the device (8 bytes per 64 stored rows and 4 per list, nothing else)
 * for any number of searches and range searches: a tombstone set, a tenant's ids, an ACL.
 * vdb_ivf_filter_create takes a host array, vdb_ivf_filter_create_device an array on the
 * handle's device that is complete before the call; mode, order, repeats, ids that are not
 * stored, n_filter == 0 and the pad slots are as for vdb_ivf_search_filtered. The ids are sorted
 * on the device, so a large set costs no host sort. *out is written on success only. Refused
 * as vdb_ivf_search_filtered refuses: a null handle, ids or out and an invalid mode
 * VDB_ERR_INVALID_ARGUMENT; n_filter >= 2^31, the list-cache tier, a file-home, a sharded and a
 * group handle VDB_ERR_UNSUPPORTED.
 * vdb_filter_combine makes a third filter of two live filters of one handle: VDB_FILTER_AND
 * allows the rows both allow, VDB_FILTER_OR the rows either allows, VDB_FILTER_ANDNOT the rows
 * a allows and b does not. (No bare NOT: no mask ever has a bit in a pad slot.) Filters of two
 * handles give VDB_ERR_INVALID_ARGUMENT.
 * A filter describes the handle's rows where they lay when it was made. It stays valid across
 * searches of every kind, including the switch between the lists' two fp32 layouts; it is stale
 * once a call has run that can move a row: vdb_ivf_add*, a vdb_ivf_remove_ids that removed a
 * row, a vdb_ivf_upsert* with n > 0, vdb_ivf_load, vdb_ivf_open_lists, vdb_ivf_set_shard* / vdb_ivf_plan_shard*,
 * vdb_ivf_set_option of list_cache_bytes or max_gpu_memory, and vdb_ivf_destroy. A stale filter
 * is refused with VDB_ERR_STATE by every call that takes one; vdb_filter_stale tells (1 also for
 * NULL), and vdb_filter_free releases it, before or after the handle was destroyed.
 * vdb_ivf_search_prepared returns, bit for bit, what vdb_ivf_search_filtered returns for the id
 * set the filter was made from (for a combined filter: for the row set it allows), with the
 * same limits (k <= 64); vdb_filter_last_timing reports it with mark_ms = 0.
 * vdb_ivf_range_search_prepared returns the result of vdb_ivf_range_search on a handle with the
 * same centroids and metric that stores only the allowed rows in their original order; all
 * else (the inclusive comparison, ids stored twice, the order, reserve and the re-run, the
 * independence of stale_slots and batch) as described there. filter == NULL is
 * vdb_ivf_range_search. vdb_range_last_timing reports it; pairs_scanned counts the distances
 * of allowed rows only. A block of 64 slots without an allowed row is skipped unread, and while
 * the lists are held row-major only the allowed rows' bytes are read.
 * A filter of another handle gives VDB_ERR_INVALID_ARGUMENT; what the one-shot calls refuse is
 * refused the same way; a refusal leaves the handle untouched. Every call here holds the
 * handle's lock and has finished its device work when it returns. Not offered yet: coalescing
 * of concurrent prepared calls; a caller that holds queries of several filters puts them into
 * one vdb_ivf_search_prepared_multi (below). */
typedef struct vdb_filter vdb_filter;
enum { VDB_FILTER_AND = 0, VDB_FILTER_OR = 1, VDB_FILTER_ANDNOT = 2 };
int vdb_ivf_filter_create(vdb_ivf* index, const uint64_t* filter_ids, uint64_t n_filter, int mode, vdb_filter** out);
int vdb_ivf_filter_create_device(vdb_ivf* index, const uint64_t* d_filter_ids, uint64_t n_filter, int mode,
                                 vdb_filter** out);
int vdb_filter_combine(const vdb_filter* a, const vdb_filter* b, int op, vdb_filter** out);
uint64_t vdb_filter_allowed(const vdb_filter* filter);   /* stored rows it lets through */
int vdb_filter_stale(const vdb_filter* filter);          /* 1 once the handle's rows changed or the handle is gone */
void vdb_filter_free(vdb_filter* filter);                /* NULL is fine; valid after the handle was destroyed */
int vdb_ivf_search_prepared(vdb_ivf* index, const vdb_filter* filter, const float* queries, uint32_t n,
                            uint32_t nprobe, uint32_t k, float* distances, uint64_t* ids);
int vdb_ivf_range_search_prepared(vdb_ivf* index, const vdb_filter* filter, const float* queries, uint32_t n,
                                  uint32_t nprobe, float radius, uint64_t reserve, vdb_range_result** out);
/* Per-query prepared filters: one search for a batch whose queries each belong to their own
 * filter (a mixed-tenant batch). filters[0..n_filters) are prepared filters of this handle and
 * filter_of[i] < n_filters names the filter of query i; host buffers throughout, as for
 * vdb_ivf_search_prepared. Two entries of filters[] may be the same filter; a filter no query
 * names is still validated.
 * For every filter index f, let S_f be the queries i with filter_of[i] == f, in call order. The
 * result rows of S_f are, bit for bit (ids and distance bits), what vdb_ivf_search_prepared(index,
 * filters[f], the queries of S_f, |S_f|, nprobe, k) returns: the mixed call equals the
 * per-filter calls scattered back into request order. So the stale-slot reuse (stale_slots = 1)
 * never crosses filters: a slot whose list has no row the query's filter allows keeps the
 * content of the latest earlier query of the same filter whose probe at that slot had an
 * allowed row. With stale_slots = 0, row i is the single-query prepared search of query i.
 * Results never depend on the `batch` option. Cosine is served (every distance 0.0f, ties by
 * id); VDB_METRIC_COSINE_DISTANCE is mapped after the last merge, as the prepared call maps it.
 * One pass serves the batch: one upload, one coarse step, one pair grouping, and a masked exact
 * scan that looks the mask up per query, so queries of different filters that probe the same
 * list share the read of its blocks. A block is read where the mask of any of the (up to four)
 * queries that share the read has a bit; a row is offered to a query only where that query's
 * own mask has its bit.
 * The call builds, refreshes and releases nothing: vdb_ivf_gpu_bytes_allocated is the same
 * before and after, every filter stays live, and a following vdb_ivf_search returns the bits it
 * returns without the call. It holds the handle's lock and has finished its device work when it
 * returns. vdb_filter_last_timing reports it: mark_ms = 0, scan_ms and merge_ms summed over the
 * batches, pairs_scanned the sum over the (query, probe) pairs of the rows that query's filter
 * allows in that list.
 * Refusals (the handle untouched, the outputs not written): VDB_ERR_INVALID_ARGUMENT, before any
 * device call, for a null handle, for null queries, distances or ids with n > 0, for null filters
 * or filter_of with n > 0, for n_filters == 0 with n > 0, for a null entry of filters[] and for
 * a filter_of[i] >= n_filters; VDB_ERR_INVALID_ARGUMENT for a filter of another handle;
 * VDB_ERR_STATE for a stale filter; VDB_ERR_UNSUPPORTED for k > 64 and for the list-cache tier,
 * a file-home, a sharded and a group handle, exactly what vdb_ivf_search_prepared refuses. n == 0
 * or k == 0 succeeds and touches nothing; an empty index or nprobe == 0 fills every slot with
 * (FLT_MAX, UINT64_MAX).
 * Not offered: the gRPC service, a device-pointer variant, per-query filters for the range
 * search and for the screen. */
int vdb_ivf_search_prepared_multi(vdb_ivf* index, const vdb_filter* const* filters, uint32_t n_filters,
                                  const uint32_t* filter_of, const float* queries, uint32_t n,
                                  uint32_t nprobe, uint32_t k, float* distances, uint64_t* ids);
/* Range search through the screen: vdb_ivf_range_search (filter == NULL) or
 * vdb_ivf_range_search_prepared served from the shadow the screened search keeps. The result is,
 * bit for bit (lims, ids, distance bits), what the exact call returns, with its reserve, its
 * re-run and its independence of stale_slots and batch; only the bytes read differ.
 * Per batch the pairs are grouped sixteen to an item, the screened search's own pairs kernel
 * prepares them, a bound kernel computes the screen's lower bound of every (query, row) pair on
 * the matrix cores from the int8 or bf16 shadow (a quarter or half of the fp32 bytes) and keeps
 * the pairs whose bound is not above the radius, and a re-check computes exactly those pairs'
 * sequential fp32 distances from the row-major copy; the hits are ordered as the exact call
 * orders them. A huge or non-finite row, query or centroid has no finite bound and is always
 * re-checked. With a filter, a block of 64 slots without an allowed row is skipped unread.
 * Routing: the call uses the screen the handle holds at that moment and builds, refreshes and
 * releases nothing (vdb_ivf_gpu_bytes_allocated is the same before and after, prepared filters
 * stay live). A handle without a live screen (before its first search, after an add, remove,
 * upsert or new centroids until the next search, with the option screen 0, with
 * VDB_METRIC_COSINE) is served by the exact path, unchanged. L2, inner product and
 * VDB_METRIC_COSINE_DISTANCE (thresholded and mapped as the exact call does) go through the
 * screen.
 * Fallback: a batch's candidate buffer holds 4 entries (8 bytes each) per entry of its hit
 * buffer, so 1,048,576 at reserve == 0, and at most 2^28. A batch whose bound keeps more than
 * that is served by the exact scan instead (a radius that wide is the exact scan's work); a
 * batch whose hits exceed the hit buffer runs its re-check once more, the candidates kept.
 * Refusals are those of vdb_ivf_range_search(_prepared), the handle untouched and *out written
 * on success only: a null handle, queries or out and a NaN radius VDB_ERR_INVALID_ARGUMENT, as
 * a filter of another handle; the list-cache tier, a file-home, a sharded and a group handle
 * VDB_ERR_UNSUPPORTED; a stale filter VDB_ERR_STATE. The call holds the handle's lock and has
 * finished its device work when it returns.
 * vdb_range_last_timing reports this call too: scan_ms covers grouping, pairs, bound and
 * re-check (or the exact scan of a batch that fell back), pairs_scanned the exact distances
 * computed (the re-checked candidates, and every pair of a batch that fell back).
 * Not offered: the list-cache tier, group and sharded handles, per-query radii, a device-pointer
 * variant, the gRPC service; vdb_ivf_range_search(_prepared) keep the exact route. */
int vdb_ivf_range_search_screened(vdb_ivf* index, const vdb_filter* filter, const float* queries, uint32_t n,
                                  uint32_t nprobe, float radius, uint64_t reserve, vdb_range_result** out);
/* Diagnostics: the calling thread's latest vdb_ivf_range_search_screened by step (HIP events
 * summed over the call's batches): the pairs kernel, the bound kernel, the re-check (re-runs
 * included); the (query, row) pairs the bound kernel judged (with a filter: of allowed rows) and
 * those it kept; the batches served through the screen and by the exact scan. Any pointer may be
 * NULL; a thread without a call reads zeros. */
int vdb_range_screen_last_timing(double* pairs_ms, double* bound_ms, double* recheck_ms, uint64_t* pairs_bounded,
                                 uint64_t* candidates, uint32_t* screened_batches, uint32_t* exact_batches);
/* Diagnostics: the calling thread's latest vdb_ivf_filter_create(_device) (HIP events): the
 * device sort of the ids, and the mark and count kernels. Either pointer may be NULL. */
int vdb_filter_create_last_timing(double* sort_ms, double* mark_ms);
/* Fetch by id: the stored rows that carry ids[0..n), and a search with stored rows as the
 * queries. No counterpart in the reference; without it a row is only reachable through
 * vdb_ivf_get_list over every list.
 * vdb_ivf_fetch_ids, for request entry i: if a stored row carries ids[i], found[i] = 1 and
 * vectors[i] holds its dim floats, bit for bit as vdb_ivf_get_list returns them (with
 * VDB_METRIC_COSINE_DISTANCE the unit row as stored, not normalised again); otherwise found[i] =
 * 0 and the row is dim zeros. An id stored more than once gives the row at the lowest list id
 * and, within that list, the earliest position in add order. A repeat within ids[] gets the same
 * row each time; the order of the request is kept. Pad slots are never matched, whatever ids[]
 * holds, UINT64_MAX included. vectors (n x dim fp32), found (n bytes) and n_found may each be
 * NULL (found alone: an existence check); *n_found counts entries, a repeated id every time it
 * appears. n == 0 succeeds and touches no buffer. Host buffers.
 * vdb_ivf_fetch_ids_device is the same on buffers of the handle's device that are complete
 * before the call (n_found stays a host pointer).
 * Nothing moves and nothing is rebuilt: the request is sorted on the device, one pass over the
 * stored ids (8 bytes per stored row, no row data) finds each id's slot, and one wave per
 * request entry copies its row from whichever fp32 layout the handle holds at that moment, the
 * interleaved arena or the screen's row-major copy. Temporaries are the call's own:
 * vdb_ivf_gpu_bytes_allocated is unchanged, prepared filters stay valid, no screen is built or
 * dropped. The call holds the handle's lock and has finished its device work when it returns.
 * vdb_ivf_search_ids: let F be the request entries that are found, in request order. Their
 * result rows are, bit for bit, what vdb_ivf_search(index, rows of F, |F|, nprobe, k) returns
 * (one call over the found rows only, so with stale_slots = 1 a slot's content passes from a found
 * query to the next found query); entries that are not found get (FLT_MAX, UINT64_MAX) in every
 * slot and found[i] = 0 (found may be NULL). The rows go from the gather's device buffer into
 * the entry vdb_ivf_search_device uses, on the handle's stream, and never leave the device;
 * every route serves them as it serves any device query (the screen, the exact scan, k > 64,
 * the run-time floor), and a VDB_METRIC_COSINE_DISTANCE handle normalises them like any query.
 * Like any search, this one may build the screen. Host buffers.
 * Limits of this version (the handle is untouched by a refusal): a null handle, null ids with
 * n > 0, and null distances or result_ids give VDB_ERR_INVALID_ARGUMENT; n >= 2^31, k or nprobe
 * above 1024, a handle in the list-cache tier (option list_cache_bytes, or max_gpu_memory
 * exceeded), a file-home handle (vdb_ivf_open_lists), a sharded handle (world > 1) and a group
 * handle give VDB_ERR_UNSUPPORTED: the set vdb_ivf_search_filtered refuses, for the same reasons
 * (the rows are not all in this device's HBM). Not offered yet: those four kinds of handle, the
 * gRPC service, a caller's stream for the device variant, coalescing of concurrent fetches. */
int vdb_ivf_fetch_ids(vdb_ivf* index, const uint64_t* ids, uint64_t n,
                      float* vectors, uint8_t* found, uint64_t* n_found);
int vdb_ivf_fetch_ids_device(vdb_ivf* index, const uint64_t* d_ids, uint64_t n,
                             float* d_vectors, uint8_t* d_found, uint64_t* n_found);
int vdb_ivf_search_ids(vdb_ivf* index, const uint64_t* ids, uint32_t n, uint32_t nprobe, uint32_t k,
                       float* distances, uint64_t* result_ids, uint8_t* found);
/* Diagnostics: the calling thread's latest vdb_ivf_fetch_ids(_device) or vdb_ivf_search_ids, by
 * step (HIP events): the device sort of the request, the locate pass, the gather (search_ids:
 * its two passes, the marks and then the found rows), and the entries found. Any pointer may be
 * NULL; a thread without a call reads zeros. */
int vdb_fetch_last_timing(double* sort_ms, double* locate_ms, double* gather_ms, uint64_t* rows_found);
/* Persist / restore centroids and lists (IVFFlatIndex::save/load, engine/ivf_flat_index.h:66-67,
 * declared but never defined in the reference; this engine's own file format). */
int vdb_ivf_save(vdb_ivf* index, const char* path);
int vdb_ivf_load(vdb_ivf* index, const char* path);

/* search: host buffers in and out (PCIe included). nprobe is clamped to nlist.
 * Thread-safe: concurrent callers are coalesced into shared device batches (calls with
 * the same nprobe and k), each call keeping exactly the results it would get alone
 * (option "coalesce" = 0 serialises calls instead). */
int vdb_ivf_search(vdb_ivf* index, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k,
                   float* distances, uint64_t* ids);
/* search on device buffers, enqueued on `stream` (NULL = the handle's stream),
 * asynchronous. When a shard is set (vdb_ivf_set_shard with world > 1) the outputs
 * are this rank's partial results, to be combined with vdb_merge_ranks_device. */
int vdb_ivf_search_device(vdb_ivf* index, const float* d_queries, uint32_t n, uint32_t nprobe,
                          uint32_t k, float* d_distances, uint64_t* d_ids, void* stream);

/* Multi-GPU: restrict this handle to the lists rank `rank` owns out of `world`
 * (size-balanced LPT over list lengths, identical on every rank), and free the
 * rest of the list arena. Emptiness of non-owned lists is still tracked. */
int vdb_ivf_set_shard(vdb_ivf* index, uint32_t rank, uint32_t world);
/* Sharded build of an index larger than one GPU (100M x 768 over 8 GPUs): on an empty,
 * trained index, fix this rank's lists from the final list sizes (the same LPT plan as
 * set_shard); later adds store only those lists' rows and count the others. */
int vdb_ivf_plan_shard(vdb_ivf* index, uint32_t rank, uint32_t world, const uint64_t* final_sizes);
/* Combine per-rank partials gathered as [nranks][n][k] into final [n][k]. */
int vdb_merge_ranks_device(const float* d_dist, const uint64_t* d_ids, uint32_t nranks, uint32_t n,
                           uint32_t k, float* d_out_dist, uint64_t* d_out_ids, void* stream);
/* One rank's partials as a single record for ONE collective per batch: f32 dist[n][k],
 * padded to 8 bytes, then u64 ids[n][k]. vdb_rank_record_bytes gives its size; a
 * search writes into it with d_distances = record, d_ids = record + that padding. */
uint64_t vdb_rank_record_bytes(uint32_t n, uint32_t k);
/* Combine gathered records [nranks][record] into final [n][k]. */
int vdb_merge_ranks_packed_device(const void* d_records, uint32_t nranks, uint32_t n, uint32_t k,
                                  float* d_out_dist, uint64_t* d_out_ids, void* stream);
/* Host-only: the LPT owner of every list for `world` ranks (no GPU needed). */
int vdb_shard_plan(const uint64_t* list_sizes, uint32_t nlist, uint32_t world, uint32_t* owner);
/* Host-only: LPT over each list's expected scan cost per batch of `batch` queries, from a
 * probe census (probe_counts[l] of n_sample query-like rows probe list l): the list is
 * streamed once per group of 16 queries that probe it (binomial expectation) plus the
 * per-query distance arithmetic. Balances the ranks' scan time where list popularity, not
 * only list size, differs. Identical on every rank for the same inputs. */
int vdb_shard_plan_probe_weighted(const uint64_t* list_sizes, const uint64_t* probe_counts, uint64_t n_sample,
                                  uint32_t batch, uint32_t nlist, uint32_t world, uint32_t* owner);
/* counts[l] = how many of the n device rows d_rows (n x dim) probe list l with `nprobe`
 * (the exact probe selection of search; nlist entries written). */
int vdb_ivf_probe_census(vdb_ivf* index, const float* d_rows, uint64_t n, uint32_t nprobe, uint64_t* counts);
/* set_shard / plan_shard with an explicit plan (owner[l] = rank of list l, the same array
 * on every rank), e.g. from vdb_shard_plan_probe_weighted. */
int vdb_ivf_set_shard_owners(vdb_ivf* index, uint32_t rank, uint32_t world, const uint32_t* owner);
int vdb_ivf_plan_shard_owners(vdb_ivf* index, uint32_t rank, uint32_t world, const uint64_t* final_sizes,
                              const uint32_t* owner);

/* ---- Multi-GPU inside the engine (RCCL over xGMI) ----
 * One process per GPU: rank 0 draws a communicator id (vdb_comm_unique_id) and shares it
 * with the other ranks (any channel); every rank, after set_shard / plan_shard with the
 * same (rank, world), calls vdb_ivf_attach_comm. From then on vdb_ivf_search_device /
 * vdb_ivf_search on that handle all-gather every batch's per-rank partials (ONE RCCL
 * all-gather per batch of vdb_rank_record_bytes per rank) and merge them on the device,
 * so every rank receives the FINAL results. Every rank must issue the same search calls
 * (same n, nprobe, k and batch option) in the same order; on such a handle vdb_ivf_search
 * does not coalesce concurrent callers (the grouping would depend on each rank's timing):
 * calls run one at a time. At world > 1 a call ends in ONE all-gather of the whole call's
 * partials (not one per batch): a rank's own state (its list-cache tier, which its shard's
 * size may switch on, and what its cache holds) shapes its batches, so only per-call
 * exchanges are the same on every rank. */
#define VDB_COMM_ID_BYTES 128
int vdb_comm_unique_id(void* id); /* VDB_COMM_ID_BYTES bytes (ncclGetUniqueId) */
int vdb_ivf_attach_comm(vdb_ivf* index, const void* id, uint32_t rank, uint32_t world);
int vdb_ivf_detach_comm(vdb_ivf* index);
/* The communicator's deadline (option "comm_timeout_ms", default 120000): init is
 * non-blocking and polled, so a rank that never joins makes vdb_ivf_attach_comm fail with
 * VDB_ERR_DEVICE naming this rank; at attach every rank's dimension, nlist, metric, batch,
 * stale_slots and list sizes are compared, and the ranks' stored lists must
 * partition the non-empty lists (VDB_ERR_STATE otherwise). Each exchange's completion is watched; one
 * still pending after the deadline marks the communicator failed (later searches fail with
 * the message). vdb_ivf_comm_status returns VDB_OK, or VDB_ERR_DEVICE with that message,
 * and the exchanges issued / completed so far (either pointer may be NULL): a caller
 * waiting on its streams polls it to stop waiting on a stalled peer. After a failure the
 * process is expected to exit; vdb_ivf_detach_comm then aborts the communicator. */
int vdb_ivf_comm_status(vdb_ivf* index, uint64_t* exchanges_issued, uint64_t* exchanges_done);
/* One process driving several GPUs: a group handle with one member index per device
 * (devices[0] holds the host-API staging; device pointers passed to the group's calls
 * live on devices[0]). The group is used through every call of this header like a
 * single-device handle: train runs on devices[0] and its centroids are copied to every
 * member; add places each list on a member when the list first receives vectors
 * (largest first on the least-loaded member: the LPT plan of vdb_shard_plan for a bulk
 * add) and every member stores its lists; a search broadcasts the queries (RCCL), runs
 * each member's shard and all-gathers + merges per batch, with results bit-identical to
 * one device. Members on distinct devices use ncclCommInitAll; members sharing a device
 * (a one-GPU rehearsal) exchange through device copies. The list-cache tier and the
 * max_gpu_memory cap act per member (per GPU); a call on a group with tiered members ends
 * in one exchange for the whole call. Not available on a group: set_shard, plan_shard,
 * open_lists. */
int vdb_ivf_create_group(const vdb_ivf_config* config, const int* devices, uint32_t ndevices, vdb_ivf** out);
uint32_t vdb_ivf_group_size(const vdb_ivf* index); /* members; 1 for a single-device handle */
/* Per list the member (group) or rank (sharded handle) storing it; UINT32_MAX: none. */
int vdb_ivf_list_owners(vdb_ivf* index, uint32_t* owner);

/* List residency. By default the whole index is HBM-resident (288 GB per GPU) and
 * these keep the API. With the list-cache tier (option "list_cache_bytes" > 0) the
 * lists live in page-locked host memory and HBM caches whole lists under that byte
 * cap, like the reference's load_list_to_gpu / evict_list_from_gpu
 * (engine/ivf_flat_index.cpp:387-471, ivf_flat_index.h:60-61): warmup loads lists
 * (one that cannot fit is skipped), evict drops one, and a search loads the lists
 * each batch probes first (least recently used lists make room). Results are the
 * same in both modes. */
int vdb_ivf_warmup(vdb_ivf* index, const uint32_t* lists, uint32_t n);
int vdb_ivf_evict(vdb_ivf* index, uint32_t list);
typedef struct vdb_ivf_cache_stats_t {
    uint64_t capacity_bytes;  /* 0: tier off */
    uint64_t resident_bytes;
    uint64_t resident_lists;
    uint64_t loads;           /* lists copied host -> HBM */
    uint64_t evictions;       /* lists evicted to make room (not counting vdb_ivf_evict) */
    uint64_t bytes_loaded;
    uint64_t file_bytes_read; /* lists served from a file: bytes read from it */
    uint64_t subbatches;      /* sub-batches searched through the tier (cut to fit the cache) */
    uint64_t prefetches;      /* sub-batches whose lists were loaded while the previous one scanned */
    uint64_t sync_loads;      /* sub-batches whose lists were loaded before their own scan */
    int32_t io_uring;         /* 1: the file home is read through io_uring (0: pread fallback) */
    int32_t o_direct;         /* 1: the file home is read with O_DIRECT */
    /* The screen in the tier (L2 / IP, k <= 64): the lists' bf16 shadow, norms and ids stay in
     * HBM and only the exact re-checks' rows are read from the home, per batch. */
    int32_t screen_resident;      /* 1: the shadow of every stored list is HBM-resident */
    int32_t reserved;
    uint64_t screen_bytes;        /* HBM of the resident shadow, norms and ids */
    uint64_t screen_batches;      /* batches the screen served in the tier */
    uint64_t screen_rows_fetched; /* survivors' rows read from the file home (host home: read over PCIe) */
    uint64_t screen_row_bytes;
    uint64_t screen_reruns;       /* batches re-run after overflowing the candidate buffer */
    uint64_t screen_rows_cached;  /* survivor rows read from the HBM cache instead of the file
                                     (option tier_row_cache: the largest lists' rows kept there) */
    uint64_t screen_fallbacks;    /* batches whose candidates would exceed "tier_cand_max": served
                                     by the exact list-cache path instead */
} vdb_ivf_cache_stats_t;
int vdb_ivf_cache_stats(vdb_ivf* index, vdb_ivf_cache_stats_t* out);
/* The screened tier's row cache (file home, option tier_row_cache): refill the HBM list
 * cache with the lists that save the most survivor-row reads per cached byte, by
 * weights[l] / count[l] (weights: per list its expected survivor rows, e.g. the histogram of
 * the batches served so far from vdb_ivf_survivor_histogram), or by list size when weights is
 * null (the default). The order is kept for later fills (a rebuilt screen). */
int vdb_ivf_fill_row_cache(vdb_ivf* index, const uint64_t* weights);
/* Per list (nlist entries): the survivor rows the screened tier's batches needed so far. */
int vdb_ivf_survivor_histogram(vdb_ivf* index, uint64_t* out);
/* Diagnostics (option "collect_stamps" = N records): the screened collect kernel's timeline,
 * 4 x u64 per record {batch << 40 | item << 16 | workgroup, start, end (wall clock ticks),
 * queries | segments << 8 | kind << 16 (0 wide item, 1 narrow item, 2 workgroup start) |
 * list << 32}; copies min(cap, *n) records, *clock_hz = the wall clock's rate, and resets the
 * buffer. Synchronises the handle. */
int vdb_ivf_collect_stamps(vdb_ivf* index, uint64_t* out, uint64_t cap, uint64_t* n, uint64_t* clock_hz);
/* Diagnostics: one named buffer of the most recently issued batch of the deferred screened
 * scan (rows in HBM), read-only: synchronises the handle, copies the buffer to `out` (cap_bytes
 * at least its size) and sets *bytes; out null: the size only. Nothing is changed. Per batch:
 * "probes" u32[B P], "sorted_pair" u32[B P] (query << 16 | probe), "counters" u32 (the whole
 * array), "cand" u32[n][4] {sorted pair, slot, lower bound bits, rank or ~0} for n = min(reserved,
 * capacity), "ovf", "ubcnt", "scnt" u32[B P], "thr" u32[B P] and "thr4" u32[B P][4] (order-
 * preserving float encoding), "ublist" f32[B P][lists][k], "soff" u32[B P + 1], "surv"
 * u32[survivors][2] {slot, sorted pair}, "pst" f32[B P][4], "qscale" f32[B P] (int8 shadow; else
 * empty), "qres" (int8 or bf16 [B P][dp]); per handle: "block_off" u64[nlist], "count"
 * u32[nlist], "meta" f32[slots][4], "sscale" f32[slots] (int8), "shadow" (bytes); and "scalars"
 * u64[18] {B, P, k, dp, seg_blocks, segs_item, wide_q, cand_cap, int8 shadow, metric, collect
 * workgroups, nlist, blocks, upper-bound lists per pair, candidate chunk, dim, workspace slot,
 * entries allocated for candidates}; "cand_alloc": the slot's whole candidate allocation (what
 * lies past the capacity must never change).
 * VDB_ERR_INVALID_ARGUMENT: a null or unknown name, a group handle, or a last batch that took
 * another route (the inline screen, the exact scan, the tier). */
int vdb_ivf_screen_snapshot(vdb_ivf* index, const char* name, void* out, uint64_t cap_bytes, uint64_t* bytes);
/* Diagnostics: the coarse step's buffers for n rows of the caller's ([n][dim], host memory),
 * read-only: the rows staged as a batch's queries are (zero-padded, or brought to unit length on
 * a VDB_METRIC_COSINE_DISTANCE handle), the matrix-core bounds over the handle's centroids by
 * the kernel the engine would pick for n rows of this dimension, then the search's selection for
 * nprobe (its top min(nprobe, nlist) lists by exact (distance, list)) and the add's assignment,
 * on buffers of the call's own that are freed on return. The option coarse_mode is not consulted.
 * Host outputs, any of which may be null: approx and delta f32[n][nlist], the approximate
 * distance and its error bound, |approx - exact| <= delta wherever both are finite; cand
 * u32[n][nlist], row i: the lists of row i whose interval can reach the top, in any order, then
 * UINT32_MAX; probes u32[n][min(nprobe, nlist)]; assign u32[n]. nprobe 0 skips the selection:
 * cand and probes must then be null. Synchronises the handle and changes nothing in it:
 * vdb_ivf_gpu_bytes_allocated and the bits of a following search are as without the call.
 * Refused before any launch: a null handle or null rows, a group handle, nprobe > 0 with cand
 * and probes both null, nprobe 0 with either, n * nlist above 2^27 VDB_ERR_INVALID_ARGUMENT;
 * VDB_METRIC_COSINE (no matrix-core path), a dimension whose query row does not fit the
 * selection's LDS, min(nprobe, nlist) above 1024 VDB_ERR_UNSUPPORTED. */
int vdb_ivf_coarse_snapshot(vdb_ivf* index, const float* rows, uint32_t n, uint32_t nprobe,
                            float* approx, float* delta, uint32_t* cand, uint32_t* probes, uint32_t* assign);
/* The tier's home on disk (ListPrefetcher::register_list_file / prefetch_lists,
 * engine/prefetcher.h:139-183; list files of format/storage.h): serve this handle's lists
 * from an index file written by vdb_ivf_save, without reading them into memory.
 * Centroids and list sizes are read at once; a list is read (pread -> pinned staging ->
 * HBM -> pad + interleave on the device) when a batch first probes it or on
 * vdb_ivf_warmup, and evicted like any cached list. Needs "list_cache_bytes" > 0 set
 * first; the handle becomes read-only (add fails with VDB_ERR_STATE). A shard file
 * (vdb_ivf_save of a handle with world > 1: every list's count, only the rank's own lists'
 * rows) makes this handle that rank's shard: rank and world come from the file and the lists
 * it stores define the shard (any plan; nothing is checked against a plan here, only
 * vdb_ivf_attach_comm's partition check across the ranks); vdb_ivf_attach_comm then serves a
 * sharded index larger than the node's HBM from every rank's own file.
 * With the screen (L2 / IP, k <= 64) the first search streams the file once to build the
 * lists' bf16 shadow, norms and ids in HBM; later searches read only the exact re-checks'
 * rows from the file (one O_DIRECT read each, option "tier_row_direct" 0: buffered). */
int vdb_ivf_open_lists(vdb_ivf* index, const char* path);

/* get_gpu_memory_usage's definition: count * (dim * 4 + 8) bytes per GPU-resident list. */
uint64_t vdb_ivf_gpu_bytes(const vdb_ivf* index);
/* Device memory this handle really holds: the lists in every layout it keeps (row-major
 * fp32 copy, bf16 shadow and norms while the screen serves; the interleaved arena otherwise
 * or when an exact-path search rebuilt it; the whole cache in the list-cache tier), ids,
 * centroids, directories, every search workspace and staging buffer. */
uint64_t vdb_ivf_gpu_bytes_allocated(const vdb_ivf* index);
uint64_t vdb_ivf_ntotal(const vdb_ivf* index);
uint32_t vdb_ivf_dimension(const vdb_ivf* index);
uint32_t vdb_ivf_nlist(const vdb_ivf* index);
int vdb_ivf_list_sizes(const vdb_ivf* index, uint64_t* sizes);  /* nlist entries */
/* Copy list `list` out row-major (count x dim) with its ids, in add order. */
int vdb_ivf_get_list(vdb_ivf* index, uint32_t list, float* vectors, uint64_t* ids);

/* Queries per internal batch (default 256; bounded so batch * nprobe <= 8192). */
int vdb_ivf_set_batch(vdb_ivf* index, uint32_t batch);
/* Reference quirk A1: an empty probed list leaves the previous query's
 * slot content in the merge. 1 (default) reproduces it; 0 drops empty slots. */
int vdb_ivf_set_stale_slots(vdb_ivf* index, int enable);

/* Coarse-quantiser mode: 1 (default) = MFMA distance bounds + exact re-rank of the
 * lists that can reach the top nprobe (same probe sets as mode 0); 0 = exact VALU
 * distances of every centroid. Cosine always uses mode 0. */
int vdb_ivf_set_coarse_mode(vdb_ivf* index, int mode);
/* Engine tuning knobs by name (results never change, only speed): "coarse_mode"
 * (0/1, as above), "wide_scan" (0/1: large lists as multi-query workgroup items),
 * "wide_stride" (prime dispatch stride of wide items; 1 = plan order), "batch",
 * "stale_slots" (as vdb_ivf_set_batch / vdb_ivf_set_stale_slots), "seg_vectors" (0 = auto, or
 * 64/128/256/512/1024: list vectors per scan segment), "coalesce" (0/1), "coalesce_max_queries",
 * "coalesce_window_us" (0: no waiting; calls arriving while the device is busy batch up),
 * "fused_scan" (1, default: one persistent scan grid takes both the wide and the narrow
 * items; 0: narrow items on a second stream), "screen" (1, default: the screened scan — bf16
 * matrix-core distance bounds from a shadow of the lists, exact fp32 sums only for pairs that can
 * reach a list's top-k; L2/IP, k <= 64; the lists are then held as a row-major fp32 copy plus the
 * bf16 shadow and norms, ~1.5x the list bytes, for every k: exact-path searches, k > 64, scan
 * the row-major copy; in the list-cache tier the shadow alone stays
 * in HBM and the rows at home; 0: the exact VALU scan of every pair), "screen_group" (16,
 * default, or 32: queries per screened wide item; with the deferred scan every shadow tile
 * then feeds two 16-query A operands, inline: two wave halves), "screen_defer" (1, default:
 * the screen collects candidates against upper-bound thresholds and re-checks afterwards only
 * the survivors of each (query, list) pair's final threshold; 0: re-checks inline as
 * candidates appear), "screen_recheck2" (1, default: the survivors are re-checked in two passes —
 * each pair's k smallest lower bounds first, then only the others not above their k-th exact
 * distance; in the file-home tier as two read phases; 0: every survivor in one pass; results are
 * identical), "screen_cand_cap" (collected candidates per batch, default 4M; a pair
 * beyond it is recomputed over its whole list, a file-home tier batch re-run with more, up to
 * "tier_cand_max" (32M: beyond it that batch is served by the exact list-cache path)),
 * "tier_row_direct" (1, default: the screened tier reads survivors' rows with O_DIRECT),
 * "tier_row_qd" (256: survivor-row reads in flight), "tier_row_cache" (1, default: a file-home
 * screened tier fills its idle HBM cache with the largest lists, whose survivors' rows are then
 * copied from HBM instead of read from the file), "screen_i8" (2, default: automatic —
 * int8 for lists in HBM unless the build's calibration batch vetoes it (survivors beyond k above
 * 1.5 % of the pairs, or an overflow), bf16 in the list-cache tier; 1: int8 with a per-vector
 * scale, a quarter of the fp32 bytes, a wider bound; 0: bf16, half the fp32 bytes), "screen_thr_every" (0 = automatic: blocks
 * between the collect kernel's re-reads of the shared thresholds; 4 for 32-query items, else 1),
 * "screen_floor_ppm" (50000, default: a screened batch of at least "screen_floor_min" (4M)
 * (query, vector) pairs that overflowed its candidate buffer, or whose survivors beyond k per
 * (query, list) pair exceed this many per million of its pairs, sends the next
 * "screen_floor_skip" (32) batches to the exact scan, twice as many after each further trip in
 * a row (at most 32x), then the screen is tried again; 0: never; lists in HBM only),
 * "list_cache_bytes" (0 = every list HBM-resident; > 0 = the list-cache tier above with an
 * HBM cache of that many bytes; a search whose single query probes more fails with
 * VDB_ERR_OUT_OF_MEMORY, a batch probing more is split; setting it replaces the
 * max_gpu_memory cap), "max_gpu_memory" (the Config cap, applied at once), "bounded_stats"
 * (0/1: count the screened / bounded scan's exact re-checks and blocks in vdb_ivf_profile). Timing experiments
 * that change results exist only as separate builds (VDB_SCAN_DIAG), never as options. */
int vdb_ivf_set_option(vdb_ivf* index, const char* name, int64_t value);
/* Host-API coalescing counters: device batches run and search() calls they served. */
int vdb_ivf_coalesce_stats(vdb_ivf* index, uint64_t* batches, uint64_t* requests);

int vdb_ivf_profile_enable(vdb_ivf* index, int enable);
int vdb_ivf_profile_reset(vdb_ivf* index);
int vdb_ivf_profile_read(vdb_ivf* index, vdb_ivf_profile* out);  /* synchronises the stream */

/* Wait for all work the handle enqueued on its own stream. */
int vdb_ivf_synchronize(vdb_ivf* index);
/* The handle's stream (hipStream_t as void*). */
void* vdb_ivf_stream(vdb_ivf* index);

/* Deterministic N(0,1) fp32 generator on the device (synthetic benchmark data):
 * element e of the stream (seed, offset + i) is written to d_out[i]. */
int vdb_gen_normal_device(float* d_out, uint64_t n, uint64_t seed, uint64_t offset, void* stream);
/* Gaussian-mixture rows (synthetic clustered data, balanced IVF lists): row row0 + r
 * belongs to a component drawn from (seed, row), x = d_centers[comp] (ncomp x dim,
 * device) + sigma * N(0,1). Independent of how the rows are split into calls. */
int vdb_gen_mixture_device(float* d_out, uint64_t rows, uint32_t dim, const float* d_centers, uint32_t ncomp,
                           float sigma, uint64_t seed, uint64_t row0, void* stream);

/* unit(row) of VDB_METRIC_COSINE_DISTANCE for n device rows (d_in, n x dim) into d_out (n x dim,
 * device; may not alias d_in, which is only read): the kernel a metric-3 handle applies to every
 * ingested row and every query, for callers who normalise themselves (an InnerProduct handle
 * fed these rows and queries gives the metric-3 handle's results before the 1.0f + d map). */
int vdb_unit_rows_device(const float* d_in, uint64_t n, uint32_t dim, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VDB_IVF_H */
