/*
 * vers_hip.h -- C ABI of libvers_hip.so: the MI355X (gfx950) IVFFlat hot path
 * that drops in behind ashrielbrian/vers's `Index` trait.
 *
 * Every entry point names the reference interface it replaces
 * (paths relative to /root/reference/vers/src).  The Rust-side binding a vers
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - every function returns an int32 status (VERS_OK == 0); nothing unwinds
 *     across the boundary.  The reference panics where these return
 *     VERS_ERR_NAN / VERS_ERR_INSUFFICIENT / VERS_ERR_EMPTY; a Rust shim
 *     turns a non-zero status back into a panic to keep the behaviour;
 *   - vers_last_error() returns a thread-local message for the last failure;
 *   - pointers are HOST pointers unless the function name ends in `_dev`;
 *     `_dev` functions take device pointers plus a hipStream_t (as void*,
 *     NULL = the null stream), enqueue work and return without synchronising;
 *   - rows are f32, row-major; host row pitch is passed in BYTES so that a
 *     Rust Vec<Vector<N>> (#[repr(align(256))], base.rs:14-17, pitch =
 *     round_up(4*N, 256)) can be handed over without repacking;
 *   - ids are u64 (Rust usize), distances f32.  All distances are produced
 *     with the reference's own arithmetic (sequential f32 sum of (a-b)^2, no
 *     FMA), so they are bit-identical to the reference's, not merely close.
 */
#ifndef VERS_HIP_H
#define VERS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VERS_OK 0
#define VERS_ERR_INVALID 1      /* bad argument / unsupported size */
#define VERS_ERR_NAN 2          /* reference: partial_cmp().unwrap() panics on NaN */
#define VERS_ERR_INSUFFICIENT 3 /* reference: index out of bounds at ivfflat.rs:169 */
#define VERS_ERR_HIP 4          /* HIP runtime failure */
#define VERS_ERR_EMPTY 5        /* reference: min_by(..).unwrap() on zero centroids, ivfflat.rs:207 */
#define VERS_ERR_COMM 6         /* a vers_comm_t callback of the host reported failure */

#define VERS_METRIC_L2SQ 0    /* Vector::squared_euclidean, base.rs:119-126 (what IVFFlat uses) */
#define VERS_METRIC_COSDIST 1 /* Vector::cosine_similarity(normalized=true) = 1 - dot, base.rs:153-155 */

#define VERS_MAX_TOPK 64 /* one key per lane: the width of a result list inside the kernels.  NOT a limit of any entry point:
                          * every search takes any top_k (and nprobe) like the reference; beyond 64 the result comes 64 ranks
                          * per pass. */

/* Thread-local description of the most recent failure on this thread. */
const char* vers_last_error(void);
/* ABI version of this header (bumped on incompatible change). */
int32_t vers_abi_version(void);
/* Number of visible HIP devices. */
int32_t vers_device_count(int32_t* out_count);

/* ------------------------------------------------------------------------ *
 * Flat corpus: brute-force scan.                                            *
 * Replaces utils::search_exhaustive (utils.rs:68-82): every row scored with *
 * squared_euclidean, stable ascending sort (ties -> lower index), take k.   *
 * ------------------------------------------------------------------------ */
typedef struct vers_flat vers_flat_t;

int32_t vers_flat_create(int32_t device, uint32_t d, vers_flat_t** out);
int32_t vers_flat_destroy(vers_flat_t* h);
/* Copies n rows (pitch row_stride_bytes >= 4*d) into HBM; position = vec_id.  With vers_set_option("shadow", 1) (default) the
 * handle also keeps an fp16 shadow of the rows (+ 2 d + 8 bytes per row, optional memory: dropped when it does not fit): a single
 * query (b == 1, top_k <= 48) then streams the shadow -- half the bytes -- and is finished exactly (pre-selection, certificate,
 * exact re-score; exact re-scan when the certificate fails); vers_set_option("single_shadow", 0) keeps the f32 scan.  Same results. */
int32_t vers_flat_upload(vers_flat_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes);
/* Same from rows already in HBM (row-major, pitch ld_floats >= d).  The handle keeps its own
 * copy in the scan layout (lane-transposed 64-row tiles); the caller's buffer can be freed. */
int32_t vers_flat_upload_dev(vers_flat_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats);
/* b queries (pitch q_stride_bytes).  out_ids/out_dist: [b * top_k], row q at
 * q*top_k; out_count[q] = min(top_k, n) results written for query q.  Any top_k (utils.rs:79 `take(k)` has no cap). */
int32_t vers_flat_search(vers_flat_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b,
                         uint32_t top_k, uint32_t metric, uint64_t* out_ids, float* out_dist,
                         uint32_t* out_count);
/* Same, everything in HBM; queries pitch ldq_floats (any value >= d).  Errors
 * found on the device (NaN) are latched and reported by vers_flat_poll. */
int32_t vers_flat_search_dev(vers_flat_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                             uint32_t top_k, uint32_t metric, uint64_t* out_ids_dev, float* out_dist_dev,
                             uint32_t* out_count_dev, void* stream);
/* Synchronises `stream` and returns (then clears) the latched device status. */
int32_t vers_flat_poll(vers_flat_t* h, void* stream);
/* Duration in ms of the most recent scan-kernel launch of this handle
 * (HIP events on the launch stream; synchronises on those events). */
int32_t vers_flat_last_scan_ms(vers_flat_t* h, float* out_ms);

/* ------------------------------------------------------------------------ *
 * k-means primitives on host arrays (unit-test / integration surface; the   *
 * index build below chains the same kernels without leaving the device).    *
 * ------------------------------------------------------------------------ */
/* IVFFlatIndex::assign_to_clusters (ivfflat.rs:29-46): out_assign[i] = FIRST
 * argmin_c squared_euclidean(rows[i], centroids[c]).  out_min_dist (nullable)
 * receives that minimum.  k == 0 with n > 0 -> VERS_ERR_EMPTY; NaN distance
 * with k >= 2 -> VERS_ERR_NAN (the reference panics in both cases). */
int32_t vers_kmeans_assign(int32_t device, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                           const float* centroids, uint64_t k, uint64_t c_stride_bytes, uint32_t d,
                           uint64_t* out_assign, float* out_min_dist);
/* The same on DEVICE-resident arrays (row-major, pitches in floats, multiples of 4, >= d; padding columns may hold
 * anything): out_assign_dev [n] u64 (the reference's usize), out_min_dist_dev [n] f32 or NULL.  Synchronous.  What a host
 * that streams a corpus larger than one GPU through a trained quantiser calls per chunk (cfg4: 100M rows in chunks).
 * The call's device scratch (centroid operands, workspaces: up to ~1 GiB at k = 65536) is kept per DEVICE between calls, under a
 * lock (calls on one device take turns); a call with n == 0 releases it. */
int32_t vers_kmeans_assign_dev(int32_t device, const float* rows_dev, uint64_t n, uint64_t ld_floats,
                               const float* centroids_dev, uint64_t k, uint64_t c_ld_floats, uint32_t d,
                               uint64_t* out_assign_dev, float* out_min_dist_dev);
/* Diagnostics of the matrix-core assign path (large builds; VERS_ASSIGN=1 forces the exact scan, =2 the
 * matrix cores): process-wide number of points assigned through it and how many of those failed the
 * certificate and were re-done by the exact scan.  Results are bit-identical either way. */
int32_t vers_assign_stats(uint64_t* out_points, uint64_t* out_fallbacks, int32_t reset);
/* Measurement hook: where the time of this process's build_index / k-means calls went (HIP events on the build's
 * stream).  out[8]: [0] ms in the assign contraction launches (queries x centroids on the matrix cores, ivfflat.rs:29-46),
 * [1] their count, [2] their algorithmic flop (2 * points * k * d), [3] wall ms of whole matrix-core assign passes (contraction
 * + arg-min + exact re-score + exact re-scans), [4] passes, [5] ms in update_centroids (:47-71), [6] ms in the cost fold
 * (:138-149), [7] points whose certificate failed and were settled by the exact kernels.  reset != 0 zeroes them. */
int32_t vers_build_stats(double* out8, int32_t reset);
/* The same builds by PHASE, host wall clock in ms (the build synchronises at every phase boundary anyway).  out[10]:
 * [0] whole build_index calls, [1] the build's device allocations, [2] assign passes (all of them; [3] the FIRST since the
 * last reset -- it pays the process's cold start: code load, first launches, first touch of 10s of GB -- and [4] their count),
 * [5] update_centroids, [6] the cost fold, [7] the inverted lists (grouping, storage plan + allocation, row placement; sharded:
 * + the rows-to-owners exchange), [8] what derives from the stored rows (centroid operands, |x|^2, fp16 shadow, row-major
 * copy), [9] the rest (init draws, convergence tests, read-back).  reset != 0 zeroes them (and vers_build_stats'). */
int32_t vers_build_phases(double* out10, int32_t reset);
/* The add_batch calls of this process by PHASE (host wall clock in ms, the stream synchronised at each phase's end).  out[9]:
 * [0] calls, [1] rows added, [2] re-layouts, [3] staging of the rows (host pack + copy, or the device copy), [4] assignment,
 * [5] grouping by list, [6] re-layout, [7] placement + length tables, [8] derived arrays (|x|^2, shadow, row-major copy).
 * reset != 0 zeroes them. */
int32_t vers_add_batch_phases(double* out9, int32_t reset);
/* IVFFlatIndex::update_centroids (ivfflat.rs:47-71): per cluster the f32 sum
 * of its members in ascending row order divided by the count; empty cluster
 * -> zero vector.  out_centroids is packed [k * d]. */
int32_t vers_kmeans_update(int32_t device, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                           const uint64_t* assign, uint64_t k, uint32_t d, float* out_centroids);
/* IVFFlatIndex::calculate_kmeans_cost (ivfflat.rs:138-149): left-to-right f32
 * fold of squared_euclidean(rows[i], centroids[assign[i]]). */
int32_t vers_kmeans_cost(int32_t device, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                         const float* centroids, uint64_t k, uint64_t c_stride_bytes, const uint64_t* assign,
                         uint32_t d, float* out_cost);

/* ------------------------------------------------------------------------ *
 * IVFFlat index.  The handle is the DEVICE CACHE of the five fields of       *
 * IVFFlatIndex<N> (ivfflat.rs:8-15); the host side (Rust) keeps owning        *
 * values / centroids / assignments / ids for serde and rebuilds the cache    *
 * with vers_ivf_upload after Index::load_index (base.rs:45-58).              *
 * ------------------------------------------------------------------------ */
typedef struct vers_ivf vers_ivf_t;

int32_t vers_ivf_create(int32_t device, uint32_t d, vers_ivf_t** out);
int32_t vers_ivf_destroy(vers_ivf_t* h);
/* Metric of the index (extension; set before build / upload).  VERS_METRIC_L2SQ (default) is what
 * the reference's IVFFlat computes everywhere (ivfflat.rs:37-38,146,159,175,205).  VERS_METRIC_COSDIST puts
 * Vector::cosine_similarity(normalized=true) = 1 - dot_product (base.rs:91-93,153-155: sequential f32 dot) in each of
 * those places -- assign_to_clusters, the k-means cost, add, the ranking of the lists and the scoring of their rows
 * -- with the same first-minimum / stable-sort rules; centroids stay plain means (not re-normalised), as in the
 * reference.  Results carry the bits of the sequential f32 arithmetic in both metrics. */
int32_t vers_ivf_set_metric(vers_ivf_t* h, uint32_t metric);
int32_t vers_ivf_get_metric(vers_ivf_t* h, uint32_t* out_metric);

/* IVFFlatIndex::build_index(num_clusters, num_attempts, max_iterations, &vectors)
 * (ivfflat.rs:102-136), k-means included (build_kmeans :73-100, cost :138-149).
 * init_indices [num_attempts * num_clusters]: the draws of initialize_centroids
 * (ivfflat.rs:18-27: k indices WITH replacement from an unseeded thread_rng) are made
 * by the caller, so the Rust shim keeps using rand::thread_rng and tests can inject.
 * Outputs (host, caller-owned, nullable): out_centroids k rows of pitch c_stride_bytes
 * (>= 4*d; a Vec<Vector<N>> is written in place with its own pitch round_up(4*N, 256),
 * bytes between rows are left untouched), out_assignments [n], out_cost (best cost),
 * out_kept (0 when no attempt beat +inf, e.g. num_attempts == 0: the index then has
 * EMPTY centroids/assignments exactly like the reference), out_iterations
 * [num_attempts] loop bodies executed per attempt. */
int32_t vers_ivf_build(vers_ivf_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                       uint64_t num_clusters, uint64_t num_attempts, uint64_t max_iterations,
                       const uint64_t* init_indices, float* out_centroids, uint64_t c_stride_bytes,
                       uint64_t* out_assignments, float* out_cost, int32_t* out_kept, uint64_t* out_iterations);
/* Same with the vectors already in HBM (row-major, pitch ld_floats >= d, a multiple of 4; columns
 * d .. ld_floats-1 are the caller's padding: never read into the index, they may hold anything). */
int32_t vers_ivf_build_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats,
                           uint64_t num_clusters, uint64_t num_attempts, uint64_t max_iterations,
                           const uint64_t* init_indices, float* out_centroids, uint64_t c_stride_bytes,
                           uint64_t* out_assignments, float* out_cost, int32_t* out_kept, uint64_t* out_iterations);
/* Rebuilds the device cache from the host fields (after Index::load_index): values,
 * centroids, assignments; ids[c] is implied (ascending positions with assignments == c,
 * which is what build_index + add produce). */
int32_t vers_ivf_upload(vers_ivf_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                        const float* centroids, uint64_t k, uint64_t c_stride_bytes,
                        const uint64_t* assignments);
/* The same from DEVICE-resident fields (a host that keeps `values` in HBM, or re-shards one built index over another
 * world with vers_ivf_set_shard): rows row-major with pitch ld_floats >= d (a multiple of 4; the padding columns may hold
 * anything), centroids with pitch c_ld_floats >= d, assignments as the reference's usize = u64.  Synchronous. */
int32_t vers_ivf_upload_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats,
                            const float* centroids_dev, uint64_t k, uint64_t c_ld_floats,
                            const uint64_t* assignments_dev);
/* STREAMED rebuild of the device cache: the reference's save -> load -> search sequence (utils.rs:140-148, base.rs:45-58)
 * for an index that no single GPU can hold.  The five fields (ivfflat.rs:8-15) arrive in chunks; a handle sharded with
 * vers_ivf_set_shard keeps only the rows of the lists it owns, with their GLOBAL vec ids, and no buffer of n_total rows
 * exists anywhere (device memory = the owned lists + one bounded staging chunk).  vers_ivf_upload is this sequence.
 *   begin : centroids [k] (pitch c_stride_bytes), list_lengths [k] = ids[c].len() of every list (ALL lists, also the ones
 *           another rank owns: the search plans with global lengths), n_total = assignments.len().  The handle holds no
 *           index until _end succeeds (searches in between see an empty index).
 *   chunk : rows of vec ids first_vec_id .. first_vec_id + n - 1 and their assignments.  Chunks arrive in ascending,
 *           contiguous order (first_vec_id == rows seen so far; checked): a list then fills in ascending vec id, which is
 *           what build_index + add produce (ivfflat.rs:123-127, 209-211).  Any chunk size; host rows are staged through a
 *           bounded pinned buffer, and only the rows this rank owns cross PCIe.
 *   end   : checks that n_total rows arrived and that every list received exactly list_lengths[c] of them
 *           (VERS_ERR_INVALID otherwise, the handle stays empty), then derives |x|^2, the shadow and the row-major copy.
 * Any other build / upload / add on the handle abandons a streamed upload in progress. */
int32_t vers_ivf_upload_begin(vers_ivf_t* h, const float* centroids, uint64_t k, uint64_t c_stride_bytes,
                              const uint64_t* list_lengths, uint64_t n_total);
int32_t vers_ivf_upload_chunk(vers_ivf_t* h, const float* rows, uint64_t row_stride_bytes, const uint64_t* assignments,
                              uint64_t first_vec_id, uint64_t n);
/* rows_dev row-major with pitch ld_floats >= d (a multiple of 4; padding columns may hold anything), assignments_dev u64. */
int32_t vers_ivf_upload_chunk_dev(vers_ivf_t* h, const float* rows_dev, uint64_t ld_floats, const uint64_t* assignments_dev,
                                  uint64_t first_vec_id, uint64_t n);
int32_t vers_ivf_upload_end(vers_ivf_t* h);
/* Index::add (ivfflat.rs:200-213): nearest centroid by first minimum; the new vector gets
 * vec_id = assignments.len() (the reference ignores the caller's vec_id, :209) and is appended
 * to that list.  Returns both so the host can mirror values/assignments/ids. */
int32_t vers_ivf_add(vers_ivf_t* h, const float* row, uint64_t* out_cluster, uint64_t* out_vec_id);
/* Index::add for n vectors in one call: exactly what n calls of vers_ivf_add with rows[0], rows[1], ... in that order
 * would leave behind (same clusters, vec ids, list order, stored bits, search results), in one pass over the batch.
 *   vec ids   : *out_first_vec_id .. *out_first_vec_id + *out_added - 1 (= assignments.len() at the call, ascending);
 *               each list receives its new rows after its existing ones, in ascending vec id (ivfflat.rs:200-213).
 *   clusters  : out_clusters[i] = first-minimum centroid of row i in the index's metric (the build's assign pass).
 *   errors    : the first row with a NaN distance (k >= 2) ends the call with VERS_ERR_NAN; the rows before it are added
 *               (*out_added = its index), as the loop of single adds would have left them.  k == 1 accepts a NaN row.
 *               No centroids: VERS_ERR_EMPTY.  n_total + n beyond the u32 vec id space: VERS_ERR_INVALID, nothing added.
 *               n == 0: no-op.
 *   rows      : host, row_stride_bytes >= 4 d (a multiple of 4; Vec<Vector<N>>'s 256-byte pitch as it is); streamed through a
 *               bounded staging buffer (option "add_batch_rows" rows per chunk, default 131072) -- no device copy of the batch.
 *   _dev      : rows_dev [n][ld_floats], ld_floats >= d a multiple of 4; columns d .. ld_floats-1 may hold anything (never read
 *               into the index); out_clusters_dev is a device array.
 * Synchronous; holds the handle exclusively and waits for searches in flight.  Sharded handles (vers_ivf_set_shard): every rank
 * calls with the same rows and gets the same clusters and vec ids; only a list's owner stores its rows, every rank counts them. */
int32_t vers_ivf_add_batch(vers_ivf_t* h, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                           uint64_t* out_clusters /* [n], nullable */, uint64_t* out_first_vec_id, uint64_t* out_added);
int32_t vers_ivf_add_batch_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n, uint64_t ld_floats,
                               uint64_t* out_clusters_dev /* [n], nullable */, uint64_t* out_first_vec_id, uint64_t* out_added);
/* Index::search_approximate (ivfflat.rs:153-198) for b queries.
 *   nprobe == 0 : the reference's semantics -- nearest list, spill into the next-nearest while
 *                 fewer than top_k results; results CONCATENATED per list (not globally sorted);
 *                 fewer than top_k vectors reachable -> VERS_ERR_INSUFFICIENT (reference panics).
 *   nprobe >= 1 : extension named by BASELINE.json (not in the reference): all rows of the nprobe
 *                 nearest lists, one global stable order by (distance, probe rank, list position).
 * out_ids/out_dist [b*top_k], out_count[q] results for query q.  Any top_k and nprobe (like the reference: its walk has
 * no cap); top_k <= 54 and nprobe <= 64 is the fast domain (matrix-core list scan), wider results take one ordered-chain
 * pass per 64 ranks.  Reference mode follows the spill through ALL lists if it must (like the reference's walk): the
 * host-pointer call retries deeper, a device-pointer call -- which cannot come back -- ranks up front as many lists as the
 * list lengths can make the walk need (48 unless the index holds that many near-empty lists). */
int32_t vers_ivf_search(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b,
                        uint32_t top_k, uint32_t nprobe, uint64_t* out_ids, float* out_dist,
                        uint32_t* out_count);
int32_t vers_ivf_search_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                            uint32_t top_k, uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev,
                            uint32_t* out_count_dev, void* stream);
/* Synchronises `stream`, returns and clears the status latched by _dev calls. */
int32_t vers_ivf_poll(vers_ivf_t* h, void* stream);
/* utils::search_exhaustive (utils.rs:68-82) over the index's own values (ties -> lower vec_id);
 * the recall ground truth. */
int32_t vers_ivf_search_exhaustive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b,
                                   uint32_t top_k, uint32_t metric, uint64_t* out_ids, float* out_dist,
                                   uint32_t* out_count);
int32_t vers_ivf_search_exhaustive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats,
                                       uint32_t b, uint32_t top_k, uint32_t metric, uint64_t* out_ids_dev,
                                       float* out_dist_dev, uint32_t* out_count_dev, void* stream);
/* n = vectors in the index (assignments.len()), k = centroids, longest list. */
int32_t vers_ivf_info(vers_ivf_t* h, uint64_t* out_n, uint64_t* out_k, uint64_t* out_max_list_len);
int32_t vers_ivf_list_lengths(vers_ivf_t* h, uint64_t* out_lengths /* [k] */);
/* Measurement hook: the most recent inverted-list scan launch -- duration (HIP events on its
 * stream), rows of the union of probed lists (algorithmic), rows actually streamed, work items.
 * out_streamed_rows is the PLANNED figure (rows x query groups): tiles the scan abandons early
 * (option "pre_prune") still count whole; vers_ivf_prune_stats has what was skipped. */
int32_t vers_ivf_last_scan(vers_ivf_t* h, float* out_ms, uint64_t* out_union_rows,
                           uint64_t* out_streamed_rows, uint32_t* out_items);

/* Throughput serving loops (extension; no reference counterpart -- ivfflat.rs:155-161 ranks the lists inside the
 * search itself): note the queries of the NEXT batch; the following search on this handle (the current batch) then
 * stages them and ranks their lists on a side stream of the handle right behind its own list-scan launch, i.e. under its
 * exact finish, which leaves the chip mostly idle.  A later vers_ivf_search_dev / vers_ivf_search_partial_dev call with
 * the SAME queries_dev, ldq_floats, b and nprobe picks the prepared result up (same bits) instead of computing it; the
 * query block must not change in between.  Two batches can be prepared at a time; a no-op for nprobe == 0, for more than
 * 48 probes and for batches the coarse quantiser does not run on the matrix cores for (b < 32).  `stream` is ignored
 * (kept for ABI stability): the work is ordered on the stream of the search that starts it. */
int32_t vers_ivf_coarse_ahead_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t nprobe, void* stream);

/* ---- one process per GPU: the corpus shards BY CLUSTER ------------------------------------------
 * Every rank holds the centroids and all list LENGTHS, but stores only the lists it owns.  A search
 * runs the (cheap, replicated) coarse quantiser everywhere, scans the local lists, and yields a
 * partial top-k as (key, vec_id) pairs; key = (order-preserving distance bits << 32) | sequence
 * number of the row in the query's probe order, identical on every rank, so that ONE all-gather of
 * [b][top_k] pairs (RCCL, done by the caller) followed by vers_topk_merge_dev reproduces the
 * single-GPU result bit for bit.  No reference analogue (the reference is single-process). */
/* Deterministic LPT plan (host only, no GPU): owner rank of every list from the list lengths. */
int32_t vers_shard_plan(const uint64_t* list_lengths, uint64_t k, uint32_t world, uint8_t* out_owner);
/* Before build/upload: this handle keeps only the lists vers_shard_plan gives to `rank`. */
int32_t vers_ivf_set_shard(vers_ivf_t* h, uint32_t rank, uint32_t world);
int32_t vers_ivf_owners(vers_ivf_t* h, uint8_t* out_owner /* [k] */);
/* ---- build_index over a ROW-SHARDED corpus (one process per GPU; no process ever holds all rows) ----------
 * The library owns no communicator: the host hands it one as a table of callbacks over device buffers (RCCL over
 * xGMI in vers_amd/dist.py through torch.distributed; a Rust host would put its own RCCL communicator behind the
 * same five functions).  Every callback is SYNCHRONOUS from the library's point of view: the library has
 * synchronised its stream before the call, and the data is in place when the callback returns 0.
 *   all_gather   : recv_dev[r*bytes .. (r+1)*bytes) = rank r's send_dev[0 .. bytes)
 *   send / recv  : point to point with `peer` (the chain of running sums below)
 *   broadcast    : buf_dev of `root` to everyone
 *   all_to_all_v : byte counts / offsets per peer, [world] each (rows to the owners of their lists) */
typedef struct vers_comm {
  void* ctx;
  uint32_t rank, world;
  int32_t (*all_gather)(void* ctx, const void* send_dev, void* recv_dev, uint64_t bytes);
  int32_t (*send)(void* ctx, const void* buf_dev, uint64_t bytes, uint32_t peer);
  int32_t (*recv)(void* ctx, void* buf_dev, uint64_t bytes, uint32_t peer);
  int32_t (*broadcast)(void* ctx, void* buf_dev, uint64_t bytes, uint32_t root);
  int32_t (*all_to_all_v)(void* ctx, const void* send_dev, const uint64_t* send_bytes, const uint64_t* send_off,
                          void* recv_dev, const uint64_t* recv_bytes, const uint64_t* recv_off);
} vers_comm_t;
/* IVFFlatIndex::build_index (ivfflat.rs:102-136) where rank r holds rows [row_begin, row_begin + n_local) of the
 * n_total vectors (contiguous ascending ranges in rank order; checked).  Bit-identical to the single-process build:
 *   assign_to_clusters (:29-46)  every rank assigns its own rows -- no exchange;
 *   update_centroids   (:47-71)  the reference adds the members of a cluster in ascending vec_id; rank r CONTINUES
 *                                rank r-1's per-cluster running sums over its own range (k*d*4 bytes hop to the next
 *                                rank, 12.6 MB at k=4096 d=768), the last rank divides by the all-gathered counts
 *                                and broadcasts the centroids.  (A reduce-scatter of partial sums re-associates the
 *                                f32 additions and cannot match the reference's order.)
 *   cost               (:138-149) the f32 fold over the points is chained through the ranks the same way (4 bytes);
 *   lists              (:123-127) lists are dealt to ranks by vers_shard_plan over the global lengths; every rank
 *                                sends each row to the owner of its list (ONE all_to_all_v), where rows arrive in
 *                                rank order = ascending vec_id.
 * init_indices are GLOBAL row indices.  On return the handle is sharded by cluster exactly like
 * vers_ivf_set_shard(rank, world) + build: centroids and all list lengths everywhere, rows of the owned lists only.
 * out_assignments_local (host, nullable): [n_local] clusters of this rank's rows. */
int32_t vers_ivf_build_sharded_dev(vers_ivf_t* h, const float* rows_dev, uint64_t n_local, uint64_t ld_floats,
                                   uint64_t row_begin, uint64_t n_total, uint64_t num_clusters, uint64_t num_attempts,
                                   uint64_t max_iterations, const uint64_t* init_indices, const vers_comm_t* comm,
                                   uint64_t* out_assignments_local, float* out_cost, int32_t* out_kept,
                                   uint64_t* out_iterations);
/* Removal (extension: the reference has no remove; defined in its own terms).  Removing vec id v is, on the five fields of
 * IVFFlatIndex<N> (ivfflat.rs:8-15),
 *     ids[assignments[v]].retain(|&x| x != v)
 * and nothing else: `values` and `assignments` keep their entry (positions ARE vec ids: they never shift), the centroids do not move,
 * assignments.len() -- n of vers_ivf_info, the vec id the next add hands out -- is unchanged, a removed id is never reused.  Every search
 * of the reference walks ids[c] only (ivfflat.rs:166-178), so everything observable afterwards is what the shortened lists imply:
 *   searches  : every mode and path ranks the surviving rows only, in their unchanged relative order; reference mode (nprobe == 0) spills
 *               over live rows, fewer than top_k of them reachable -> VERS_ERR_INSUFFICIENT; an emptied list is skipped;
 *               vers_ivf_search_exhaustive* ranks live rows, out_count = min(top_k, live).
 *   getters   : vers_ivf_get_list, vers_ivf_list_lengths and the longest list of vers_ivf_info report the shortened lists.
 *   add       : vers_ivf_add / _add_batch afterwards append behind a list's survivors, into the freed rows (capacity is kept: the freed
 *               rows become the list's slack; vers_ivf_compact gives the storage back).
 *   vec_ids   : any order, repeats allowed; an id that is in no list any more (removed earlier, or repeated in the call) is skipped.
 *               *out_removed = distinct rows that left the index.  ANY id >= n -> VERS_ERR_INVALID and NOTHING is removed (all ids are
 *               checked before anything is written).  n_ids == 0: no-op.  A streamed upload in progress: VERS_ERR_EMPTY (as add).
 *   host ids  : staged through a bounded pinned buffer (option "remove_batch_ids" ids per chunk, default 1048576); the device holds one
 *               bit per vec id, never the id array.
 *   _dev      : vec_ids_dev is a device array.  comm: NULL on an unsharded handle; on a handle sharded by cluster (world > 1) the
 *               callbacks of vers_ivf_build_sharded_dev -- EVERY rank calls with the same ids, the owner of a list removes its rows, ONE
 *               all_gather of the per-list removed counts ([k] u32 per rank) gives every rank the new GLOBAL lengths and the same
 *               *out_removed.  world > 1 with comm == NULL (and the host-pointer call on a sharded handle): VERS_ERR_INVALID, nothing
 *               removed.  (A rank that fails locally before the exchange returns its error without entering it: the host aborts the
 *               group on any non-zero return, as for the sharded build.)
 * Synchronous; holds the handle exclusively and waits for searches in flight, like vers_ivf_add_batch.  The running maxima the search
 * certificates charge (max |x|^2, max fp16 residual) are not re-tightened by a removal: they stay upper bounds, results are exact;
 * vers_ivf_compact recomputes them over the rows the lists still hold. */
int32_t vers_ivf_remove_batch(vers_ivf_t* h, const uint64_t* vec_ids, uint64_t n_ids, uint64_t* out_removed);
int32_t vers_ivf_remove_batch_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, uint64_t n_ids, const vers_comm_t* comm,
                                  uint64_t* out_removed);
/* Vectors currently in the lists (sum of the global list lengths) = n of vers_ivf_info minus everything removed. */
int32_t vers_ivf_live_count(vers_ivf_t* h, uint64_t* out_live);
/* The remove calls of this process by PHASE (host wall clock in ms, the stream synchronised at each phase's end).  out[8]: [0] calls,
 * [1] ids passed, [2] rows removed, [3] staging of the ids (host copy through the pinned buffer), [4] marking (bitmap, range check, the
 * pass over row_ids, a sharded handle's exchange), [5] compaction, [6] length tables, [7] derived arrays (|x|^2, shadow, row-major
 * copy of the touched tiles).  reset != 0 zeroes them. */
int32_t vers_remove_phases(double* out8, int32_t reset);
/* Update (extension: the reference cannot change a stored vector; defined on its five fields, like the removal).  For every i of the call,
 * with v = vec_ids[i] and x = rows[i]:
 *     if v is in no list (removed earlier)   -> skipped, nothing changes for v
 *     else values[v] = x;  c = first-minimum centroid of x in the index's metric (ivfflat.rs:201-207, the rule of add)
 *          if c != assignments[v] { ids[assignments[v]].retain(|&y| y != v); assignments[v] = c;
 *                                   ids[c].insert(ids[c].partition_point(|&y| y < v), v) }       -- its SORTED place, not the end
 * A row that keeps its cluster keeps its position in the list; a row that changes cluster enters the new list at its sorted place by vec
 * id, so every list stays ascending in vec id -- what vers_ivf_upload ("ids[c] is implied"), load_index and the streamed upload rely on.
 * In one sentence: AFTER AN UPDATE THE HANDLE IS, BIT FOR BIT IN EVERYTHING OBSERVABLE, A HANDLE THAT RECEIVED
 * vers_ivf_upload(values', centroids, assignments') FOLLOWED BY vers_ivf_remove_batch OF THE IDS THAT ARE IN NO LIST.  The vec ids are kept
 * (bitmap filters and prepared vers_filter_t stay valid), centroids do not move, n of vers_ivf_info, the id the next add hands out and the
 * live count do not change; ties in the (distance, probe rank, list position) order break as on that fresh handle.
 *   out_status   : [n] nullable; 0 = overwritten in place (cluster kept), 1 = moved to another list, 2 = skipped (the id is in no list).
 *   out_clusters : [n] nullable; the first-minimum centroid of rows[i] for EVERY i, skipped ones included (the host mirrors assignments).
 *   out_counts   : [4] nullable, host memory in both calls; stayed | moved | skipped | re-layouts of the storage (0 or 1).
 *   rows         : as vers_ivf_add_batch: pitch >= 4 d bytes (a multiple of 4), resp. ld_floats >= d and a multiple of 4; padding columns
 *                  are never read.
 *   ALL OR NOTHING -- every check happens before the first byte of the index is written: any id >= n -> VERS_ERR_INVALID; the same id
 *                  twice in one call -> VERS_ERR_INVALID (a loop of single updates would let the last one win; refusing keeps the batch
 *                  order-free); a NaN distance on any row with k >= 2 -> VERS_ERR_NAN (k == 1: a NaN row is accepted, as in add); no
 *                  centroids, or a streamed upload in progress -> VERS_ERR_EMPTY; a handle sharded by cluster (world > 1) ->
 *                  VERS_ERR_INVALID (not supported yet).  On any of these the index is unchanged and searchable and the outputs are
 *                  untouched.  THIS DIFFERS FROM vers_ivf_add_batch ON PURPOSE, which keeps the rows in front of a NaN.  A call of more
 *                  than one staging chunk (option "add_batch_rows") stages its rows twice for it: once to assign and check, once to place.
 *                  n == 0: no-op.  A NULL handle: VERS_ERR_INVALID before anything else is looked at.
 *   _dev         : vec_ids_dev, rows_dev, out_clusters_dev and out_status_dev are device memory.
 * Synchronous; holds the handle exclusively and waits for searches in flight, like vers_ivf_add_batch / vers_ivf_remove_batch.  The maxima
 * the search certificates charge only grow (an overwritten larger row still counts), as after a removal; vers_ivf_compact re-tightens
 * them.  Prepared filters: an update that moved a row (or re-laid-out storage) makes them rebuild at their next use; an update in which
 * every row stayed leaves them valid as they are. */
int32_t vers_ivf_update_batch(vers_ivf_t* h, const uint64_t* vec_ids, const float* rows, uint64_t n, uint64_t row_stride_bytes,
                              uint64_t* out_clusters, uint8_t* out_status, uint64_t* out_counts);
int32_t vers_ivf_update_batch_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, const float* rows_dev, uint64_t n, uint64_t ld_floats,
                                  uint64_t* out_clusters_dev, uint8_t* out_status_dev, uint64_t* out_counts);
/* The update calls of this process by PHASE (host wall clock in ms, the stream synchronised at each phase's end).  out[10]: [0] calls,
 * [1] rows passed, [2] rows that stayed, [3] rows that moved, [4] staging of the rows, [5] assign, [6] mark + locate (id table, range and
 * duplicate check, the pass over row_ids), [7] overwrite in place (and the movers into their stage), [8] compaction + merge (the movers'
 * sort and a re-layout, if any, included), [9] tables + derived arrays.  reset != 0 zeroes them. */
int32_t vers_update_phases(double* out10, int32_t reset);
/* Compaction (extension; in the reference's terms: nothing -- ids[c].shrink_to_fit()).  Nothing observable through the reference's five
 * fields changes: n of vers_ivf_info, the vec id the next add hands out, centroids, live count, every list's rows, ids and order, and every
 * search result in every mode and on every path, bit for bit.  What changes is the storage behind them:
 *   storage   : every owned list goes back to the capacity a fresh upload of the CURRENT lengths plans (len + max(8, len / 16) rounded up
 *               to 64 rows; lists in ascending order on tile boundaries; 0 for another rank's list), with every table as after that
 *               upload.  *out_rows_before / *out_rows_after (nullable): storage rows of this handle before and after.
 *   maxima    : max |x|^2 and the fp16 residual maximum the search certificates charge are recomputed over the rows the lists hold --
 *               an outlier that was added and removed stops widening every later certificate window -- and the fp16 shadow's
 *               self-retirement state restarts as at an upload: a shadow that an element beyond +-65504 had retired comes back once
 *               that row is removed.
 *   options   : "shadow", "rowmajor" and "memory" are read as a build reads them (a handle compacted under "memory" = 1 drops its
 *               row-major copy).  "compact_fused" (1): one kernel moves a tile and writes its shadow, row-major rows, |x|^2 and maxima
 *               from the same read; 0: copies, then the passes of an upload over the new storage.  Same bits either way.
 *   memory    : the old shadow and row-major copy are released before the new arrays are allocated; the old tiles are freed after the
 *               move.  When the new derived arrays do not fit beside the old tiles the call takes the unfused sequence (new tiles, move,
 *               free, derive) instead of failing; when not even the new tiles fit: VERS_ERR_HIP, the OLD index stays intact and
 *               searchable.
 *   sharded   : purely local (list lengths are global already): no communicator, ranks call it or not independently.
 * Synchronous; holds the handle exclusively and waits for searches in flight, like vers_ivf_add_batch.  No centroids: VERS_OK, nothing to
 * do, both outputs 0.  A streamed upload in progress: VERS_ERR_EMPTY (as add / remove). */
int32_t vers_ivf_compact(vers_ivf_t* h, uint64_t* out_rows_before, uint64_t* out_rows_after);
/* The compact calls of this process by PHASE (host wall clock in ms, the stream synchronised at each phase's end).  out[8]: [0] calls,
 * [1] storage rows before, [2] storage rows after (summed over the calls), [3] planning + allocation, [4] the move (fused: with every
 * derived array), [5] derived arrays on the unfused path, [6] tables, [7] reserved.  reset != 0 zeroes them. */
int32_t vers_compact_phases(double* out8, int32_t reset);
/* Recluster (extension: the reference re-trains by building a new index, which renumbers every vector; defined on its five fields, like the
 * removal and the update).  With L = the ascending sequence of the vec ids that are in some list, m = |L| and X'[j] = values[L[j]]:
 *     (centroids', a') = IVFFlatIndex::build_index(num_clusters, num_attempts, max_iterations, &X')     -- ivfflat.rs:102-136, the handle's metric,
 *                        the draws of initialize_centroids injected as init_indices [num_attempts * num_clusters]: POSITIONS in L, 0 .. m-1,
 *                        exactly what gen_range(0..X'.len()) would draw
 *     if an attempt was kept { centroids = centroids';  for j: assignments[L[j]] = a'[j];  ids[c] = [ L[j] : a'[j] == c ], ascending }
 * values, assignments.len() (n of vers_ivf_info and the id the next add hands out) and the live count do not change; an id that is not in L
 * stays in no list and is never reused.  In one sentence: AFTER A RECLUSTER THE HANDLE IS, BIT FOR BIT IN EVERYTHING OBSERVABLE, A HANDLE
 * THAT RECEIVED vers_ivf_upload(values, centroids', assignments') FOLLOWED BY vers_ivf_remove_batch OF THE IDS THAT ARE IN NO LIST
 * (assignments' of such an id is 0; nothing observable depends on it).  The vec ids are kept: bitmap filters, the host's id mapping and
 * whatever an update call addresses stay valid.
 *   arithmetic   : the k-means is the build's own -- update_centroids sums a cluster's members in ascending position of X' (ascending vec
 *                  id), the cost fold runs in that order, the first best attempt wins: centroids, assignments, cost and iteration counts
 *                  are the bits vers_ivf_build gives on the rows values[L].
 *   num_clusters : may differ from the current k, larger or smaller; an empty cluster gets the zero centroid, as in the build.
 *   storage      : the plan of a fresh upload of the new lengths (len + max(8, len / 16) rounded up to 64 rows, lists ascending on tile
 *                  boundaries), whatever slack the old lists carried.
 *   derived      : both certificate maxima and the fp16 shadow's self-retirement state are recomputed over the rows the lists hold, as
 *                  after vers_ivf_compact; the int8 head, the shadow and the row-major copy follow the options as a build reads them.
 *   filters      : a prepared vers_filter_t stays a valid object (ids are kept) and rebuilds in full at its next use, also when k changed.
 *   outputs      : host memory, all nullable except out_kept.  out_centroids: num_clusters rows of pitch c_stride_bytes (>= 4 d);
 *                  out_assignments: [n] indexed by VEC ID, 0 for an id in no list; out_cost; out_iterations [num_attempts].
 *   ALL OR NOTHING -- every refusal leaves the index unchanged and searchable and the outputs untouched: a handle sharded by cluster
 *                  (world > 1: the build's exchanges are not wired in yet) -> VERS_ERR_INVALID; no centroids, no live row,
 *                  num_clusters == 0 or a streamed upload in progress -> VERS_ERR_EMPTY; an init index >= m -> VERS_ERR_INVALID; a NaN
 *                  distance with num_clusters >= 2 -> VERS_ERR_NAN (the k-means runs beside the index, not in it).  A NULL handle:
 *                  VERS_ERR_INVALID before anything else is looked at.
 *   nothing kept : num_attempts == 0, or no attempt's cost below +inf: VERS_OK, *out_kept = 0 (cost +inf, the iteration counts written),
 *                  the index UNCHANGED.  THIS DIFFERS FROM vers_ivf_build ON PURPOSE, which leaves an empty index: a maintenance call
 *                  does not destroy what it was asked to improve.
 *   memory       : beside the index the call holds X' (m rows at the row-major pitch) for the length of the k-means, and the new tiles
 *                  until they replace the old ones; the old shadow, head and row-major copy are released before the new tiles are
 *                  reserved.  When X' or the new tiles do not fit: VERS_ERR_HIP, the OLD index stays intact and searchable (the rule of
 *                  vers_ivf_compact).
 * Synchronous; holds the handle exclusively and waits for searches in flight, like vers_ivf_add_batch / vers_ivf_remove_batch /
 * vers_ivf_compact. */
int32_t vers_ivf_recluster(vers_ivf_t* h, uint64_t num_clusters, uint64_t num_attempts, uint64_t max_iterations, const uint64_t* init_indices,
                           float* out_centroids, uint64_t c_stride_bytes, uint64_t* out_assignments, float* out_cost, int32_t* out_kept,
                           uint64_t* out_iterations);
/* The recluster calls of this process by PHASE (host wall clock in ms, the stream synchronised at each phase's end; a refused call counts
 * nowhere).  out[8]: [0] calls, [1] live rows gathered, [2] the gather (rank table plus rows), [3] k-means, all attempts, [4] install
 * (grouping, reservation, placement, id relabel), [5] derived arrays, [6] tables (the storage plan), [7] reserved.  reset != 0 zeroes them. */
int32_t vers_recluster_phases(double* out8, int32_t reset);
/* Fetch (extension: the read side of the five fields -- the reference's callers read `values` and `assignments` directly).  For every i of
 * the call, with v = vec_ids[i]:
 *     if v is in some list                 -> out_rows[i] = values[v] (the stored bits, d floats);  out_clusters[i] = assignments[v];  out_status[i] = 0
 *     if v < n is in no list (removed)     -> the d floats of out_rows[i] = +0.0;  out_clusters[i] = UINT64_MAX;  out_status[i] = 2
 *                                             (2 is vers_ivf_update_batch's code for the same fact)
 * This is the call that makes the `values'` of the mutators' specifications observable: after any sequence of add_batch, remove_batch,
 * update_batch, compact and recluster, a fetch of every id returns the fields of the handle those sentences describe.
 *   vec_ids      : any order; repeats are allowed (the call is read-only) and every occurrence is answered.
 *   out_rows     : [n] rows, nullable; pitch as vers_ivf_add_batch: row_stride_bytes >= 4 d (a multiple of 4), resp. ld_floats >= d and a
 *                  multiple of 4.  Columns d .. pitch - 1 of an output row are NEVER written.
 *   out_clusters : [n] nullable.    out_status : [n] nullable (0 found, 2 in no list).    A call without rows is the membership query.
 *   out_counts   : [2] nullable, host memory in both calls: found | in no list.
 *   ALL OR NOTHING -- every id is checked before the first store: any id >= n of vers_ivf_info -> VERS_ERR_INVALID and no output byte is
 *                  written; no centroids, or a streamed upload in progress -> VERS_ERR_EMPTY; a handle sharded by cluster (world > 1) ->
 *                  VERS_ERR_INVALID (whether an id is live is known to its owner alone; not supported yet); more than 2^32 - 1 ids in one
 *                  _dev call -> VERS_ERR_INVALID.  n == 0: no-op, counts 0.  A NULL handle: VERS_ERR_INVALID before anything else is looked at.
 *   handle       : taken the way searches take it -- shared with searches and other fetches, excluded by the mutators.
 *   _dev         : vec_ids_dev and the three outputs are device memory.  The call queues on `stream` and WAITS for it, like
 *                  vers_ivf_range_search_dev: the host must learn the check's verdict before anything may be written.
 *   host call    : ids and rows are staged through bounded pinned buffers in chunks of option "add_batch_rows" ids (without out_rows:
 *                  "remove_batch_ids"); n rows are never held on the device.
 *   sources      : the row-major copy where the handle has one (a wave per row, whole sectors); otherwise the f32 tiles alone, the requests
 *                  ordered by storage row, one job per touched tile (option "fetch_lds_min": requests per tile from which the tile is
 *                  turned through LDS instead of read piece by piece).  Same bits either way.
 *   memory       : the first fetch allocates a vec id -> storage row map of 4 bytes per vec id on the handle (freed by vers_ivf_destroy).  It
 *                  is read-side state like a prepared filter: rebuilt after anything that moved rows, extended after an add into list slack,
 *                  valid as it is otherwise.  Optional memory: when it does not fit (or option "fetch_map" = 0) every call builds a
 *                  table of its own requests instead, with the same results. */
int32_t vers_ivf_fetch(vers_ivf_t* h, const uint64_t* vec_ids, uint64_t n, float* out_rows, uint64_t row_stride_bytes, uint64_t* out_clusters,
                       uint8_t* out_status, uint64_t* out_counts);
int32_t vers_ivf_fetch_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, uint64_t n, float* out_rows_dev, uint64_t ld_floats, uint64_t* out_clusters_dev,
                           uint8_t* out_status_dev, uint64_t* out_counts, void* stream);
/* The fetch calls of this process by PHASE (host wall clock in ms, the call's stream synchronised at each phase's end; a refused call counts
 * nowhere).  out[8]: [0] calls, [1] ids passed, [2] ids found, [3] staging of the ids, [4] map build or refresh (0 when the cached map was
 * valid), [5] check + gather, [6] copy out, [7] time inside the callbacks of vers_ivf_fetch_sharded_dev.  reset != 0 zeroes them. */
int32_t vers_fetch_phases(double* out8, int32_t reset);
/* Search by stored id ("more like this"; extension).  flags == 0: row q is, bit for bit, row q of vers_ivf_search[_dev] with
 * queries[q] = values[vec_ids[q]] at the same top_k and nprobe, the reference's mode nprobe == 0 included.  The queries never leave the
 * device: they are fetched into the call's workspace at the query pitch.
 *   VERS_BYID_EXCLUDE_SELF : row q is, bit for bit, that search on an index from which vec_ids[q] ALONE was removed.  In the order of
 *                  nprobe >= 1 -- one global stable order -- that is EXACTLY: SEARCH top_k + 1, DROP THE ENTRY WHOSE ID IS vec_ids[q] IF IT
 *                  IS THERE AND THE LAST ENTRY OTHERWISE, out_count[q] = min(count, top_k) of what is left.  It holds wherever the row's
 *                  own list ranks (after vers_ivf_upload with assignments of the caller's choice that need not be rank 0, nor within the
 *                  probe at all).  With nprobe == 0 the flag is refused: the reference's spill walk over per-list remainders has no such
 *                  identity.
 *   refusals     : all decided before anything is written -- VERS_ERR_INVALID for unknown flag bits, the flag with nprobe == 0, any
 *                  id >= n, any id that is in no list (vers_ivf_fetch tells which), a handle sharded by cluster; the search's own
 *                  refusals unchanged (no centroids: VERS_ERR_INSUFFICIENT).  A NULL handle: VERS_ERR_INVALID before anything else.
 *   _dev         : after the id check -- one status word read back, for which the call waits on `stream` -- the protocol of
 *                  vers_ivf_search_dev exactly: results after the stream's work, status through vers_ivf_poll.
 *   host call    : the ids go up, the results come down; reference mode retries deeper as vers_ivf_search does. */
#define VERS_BYID_EXCLUDE_SELF 1u
int32_t vers_ivf_search_by_id(vers_ivf_t* h, const uint64_t* vec_ids, uint32_t b, uint32_t top_k, uint32_t nprobe, uint32_t flags, uint64_t* out_ids,
                              float* out_dist, uint32_t* out_count);
int32_t vers_ivf_search_by_id_dev(vers_ivf_t* h, const uint64_t* vec_ids_dev, uint32_t b, uint32_t top_k, uint32_t nprobe, uint32_t flags,
                                  uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream);
/* Range search (extension; the reference has search_approximate only).  In the reference's terms: for query q, rank the lists as
 * search_approximate does (ivfflat.rs:155-161: first minimum, stable), take the P = min(nprobe, k) nearest, and return EVERY row of
 * `ids[c]` of those lists whose distance D(q, values[id]) -- the index's metric, the reference's bits: sequential f32, multiply and add
 * rounded separately -- is <= radius[q], a plain f32 comparison (so for squared L2 a negative radius selects nothing, +inf every row of the
 * probed lists).  No top_k: the result has whatever size the radius gives it.
 *   layout   : CSR.  Query q's results are out_ids / out_dist[out_lims[q] .. out_lims[q + 1]); out_lims[0] = 0, out_lims[b] = *out_total.
 *   order    : default = the nprobe mode's global stable order, ascending (distance, probe rank, position in the list): exactly the
 *              leading entries with distance <= radius[q] of vers_ivf_search(top_k = all rows of the probed lists, nprobe) -- ids,
 *              order and distance bits.  flags & VERS_RANGE_WALK_ORDER: walk order instead -- probe rank, then position in the list,
 *              the order search_approximate concatenates in; a stable sort of it by distance gives the default order.
 *   rows     : the lists as they are NOW: rows added since the build are in, removed rows are not, storage slack is never visited.
 *   protocol : synchronous (the host must learn the total before anything can be written), like add / remove / compact.  *out_total is
 *              always the full count.  *out_total > cap: VERS_OK, out_lims complete, out_ids / out_dist UNTOUCHED -- come back with
 *              arrays of *out_total entries.  cap == 0 with NULL out_ids / out_dist is the size query.
 *   handle   : taken the way searches take it -- shared with other searches, a workspace leased per stream, excluded by add / remove /
 *              compact.  _dev: every pointer but out_total is a device pointer, the work is queued on `stream` and the call waits for it.
 *   errors   : VERS_ERR_NAN a NaN distance on any scanned row (as every search), outputs untouched; VERS_ERR_INVALID a NaN radius,
 *              nprobe == 0 (the reference's spill walk is defined by top_k and has no range meaning), unknown flag bits, more than
 *              2^32 - 1 results in one call or 2^32 - 1 (query, probe, row segment) slots of the plan -- b x min(nprobe, k) x segments
 *              of the longest list -- (either way: split the batch), a handle sharded by cluster (world > 1: its range search needs a
 *              variable-size exchange -- vers_ivf_range_search_sharded_dev below); VERS_ERR_INSUFFICIENT no centroids (as search; a streamed upload in progress
 *              is seen as an empty index); VERS_ERR_HIP scratch for the result staging did not fit, outputs untouched.
 *   edges    : b == 0 is a no-op with *out_total = 0.  A probed list that is empty contributes nothing. */
#define VERS_RANGE_WALK_ORDER 1u
int32_t vers_ivf_range_search(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius /* [b] */,
                              uint32_t nprobe, uint32_t flags, uint64_t* out_lims /* [b+1] */, uint64_t* out_ids, float* out_dist,
                              uint64_t cap, uint64_t* out_total);
int32_t vers_ivf_range_search_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                  uint32_t nprobe, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                  uint64_t cap, uint64_t* out_total /* host */, void* stream);
/* The range calls of this process by PHASE (HIP events on the call's stream, ms).  out[8]: [0] calls, [1] queries, [2] results, [3] staging +
 * coarse quantiser + plan (the exhaustive calls below: the query staging alone), [4] count pass, [5] prefix scan + read-back of the total,
 * [6] fill pass, [7] sort + decode (0 in walk order).  Calls that end in an error are not counted.  reset != 0 zeroes them. */
int32_t vers_range_phases(double* out8, int32_t reset);
/* EXHAUSTIVE range search: the ground truth beside vers_ivf_range_search, as vers_flat_search / vers_ivf_search_exhaustive are beside the
 * approximate top-k search.  For query q: EVERY row whose distance D(q, row) -- `metric` as in vers_flat_search / vers_ivf_search_exhaustive,
 * the reference's bits: sequential f32, multiply and add rounded separately -- is <= radius[q], a plain f32 comparison (squared L2: a
 * negative radius selects nothing; +inf every row).
 *   rows     : flat handle: every uploaded row.  IVF handle: every row that is in a list NOW -- added rows are in, removed rows are out,
 *              storage slack is never a result.
 *   layout   : CSR, exactly as vers_ivf_range_search: out_lims[0] = 0, out_lims[b] = *out_total, query q owns [out_lims[q], out_lims[q+1]).
 *   order    : default = ascending (distance, vec id), utils::search_exhaustive's stable order (utils.rs:68-82, ties to the lower index):
 *              EXACTLY the leading entries with distance <= radius[q] of vers_flat_search / vers_ivf_search_exhaustive with top_k = all
 *              rows -- ids, order and distance bits.  flags & VERS_RANGE_WALK_ORDER: storage order, unsorted -- flat: ascending vec id;
 *              IVF: ascending cluster, then position in the list = vers_ivf_get_list(0), (1), ... concatenated and filtered by the
 *              radius.  A stable sort of the flat walk order by distance gives the default order.
 *   protocol : as vers_ivf_range_search -- synchronous; *out_total always the full count; *out_total > cap: VERS_OK, out_lims complete,
 *              out_ids / out_dist UNTOUCHED; cap == 0 with NULL arrays is the size query; b == 0: *out_total = 0.
 *   handle   : flat: under the handle's mutex, like vers_flat_search.  IVF: the way searches take it -- shared, a leased workspace --
 *              excluded by add / remove / compact.  _dev: every pointer but out_total is a device pointer, the work is queued on `stream`
 *              and the call waits for it.
 *   errors   : VERS_ERR_NAN a NaN distance on any scanned live row, outputs untouched; VERS_ERR_INVALID a NaN radius, unknown flag bits,
 *              metric > VERS_METRIC_COSDIST, more than 2^32 - 1 results or 2^32 - 1 (query, row segment) slots in one call (split the
 *              batch), IVF only: a handle sharded by cluster (world > 1: vers_ivf_range_search_exhaustive_sharded_dev); VERS_ERR_HIP scratch for
 *              the result staging did not fit, outputs untouched.
 *   NOT an error, total 0 and every limit 0 (what the exhaustive top-k search makes of it): an empty flat corpus, an IVF handle without
 *              centroids or with a streamed upload in progress.
 * vers_range_phases counts these calls too; its slot [3] is then the query staging alone (there is no coarse quantiser and no plan). */
int32_t vers_flat_range_search(vers_flat_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius /* [b] */,
                               uint32_t metric, uint32_t flags, uint64_t* out_lims /* [b+1] */, uint64_t* out_ids, float* out_dist,
                               uint64_t cap, uint64_t* out_total);
int32_t vers_flat_range_search_dev(vers_flat_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                   uint32_t metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                   uint64_t cap, uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_exhaustive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius /* [b] */,
                                         uint32_t metric, uint32_t flags, uint64_t* out_lims /* [b+1] */, uint64_t* out_ids, float* out_dist,
                                         uint64_t cap, uint64_t* out_total);
int32_t vers_ivf_range_search_exhaustive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                             uint32_t metric, uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                             float* out_dist_dev, uint64_t cap, uint64_t* out_total /* host */, void* stream);
/* FILTERED top-k search (extension; the reference has search_approximate only): the top_k nearest among the vec ids the caller is allowed
 * to see -- a tenant, a time window, an ACL, a category.  A filter is a VIRTUAL REMOVAL: with A the set of allowed vec ids, a filtered call
 * returns, bit for bit (ids, order, distance bits, out_count), what the unfiltered call of the same mode returns on an index from which every
 * vec id not in A has been removed by vers_ivf_remove_batch -- `ids[c].retain(|v| A.contains(v))` for the duration of the call.  The index
 * itself is not touched.
 *   bitmap   : allowed_bits holds u64 words, one bitmap per call, shared by the batch: bit (v & 63) of word (v >> 6) set = vec id v is
 *              allowed.  n_bits = the number of valid bits: ids >= n_bits are not allowed, bits of the last word at or beyond n_bits are
 *              ignored and may hold anything.  n_bits may be smaller or larger than n; bits of ids that were removed or are >= n select
 *              nothing.  n_bits == 0 (allowed_bits may then be NULL) is the empty filter.
 *   probed   : vers_ivf_search_filtered, nprobe >= 1.  The lists are ranked exactly as without a filter (the centroids do not depend on it;
 *              lists the filter empties still count as probed); results are the allowed rows of the min(nprobe, k) nearest lists in the one
 *              global stable order ascending (distance, probe rank, list position); out_count[q] = min(top_k, allowed rows in q's probed
 *              lists) -- it may be 0, which is not an error.
 *   exhaustive: vers_ivf_search_exhaustive_filtered.  The allowed rows that are in a list NOW, ascending (distance, vec id);
 *              out_count[q] = min(top_k, allowed live rows).  An index without centroids (a streamed upload in progress included): counts 0.
 *   layout   : out_ids / out_dist [b * top_k], out_count [b], as vers_ivf_search / vers_ivf_search_exhaustive; entries beyond a query's
 *              count are unspecified (host-pointer calls: zeros).  Any top_k and any nprobe >= 1; results beyond 64 ranks come 64 per pass.
 *   scan     : rows outside A are NOT SCANNED: the bitmap becomes one u64 per 64-row storage tile (one pass over the row ids, every call),
 *              and a tile without an allowed row is never loaded.  A NaN distance on a disallowed row is therefore not an error; on an
 *              allowed scanned row it is VERS_ERR_NAN, as in every search.  The scan is the exact ordered f32 chain over the f32 rows
 *              (like range search): no matrix-core / fp16-shadow pre-filter.
 *   handle   : the way searches take it -- shared, one leased workspace per stream, excluded by add / remove / compact.  _dev calls enqueue
 *              on `stream` and return without synchronising; errors found on the device latch for vers_ivf_poll, exactly as
 *              vers_ivf_search_dev.  The host-pointer calls stage the bitmap through the workspace and synchronise.  A filtered call neither
 *              consumes nor starts a vers_ivf_coarse_ahead_dev preparation.
 *   errors   : VERS_ERR_INVALID n_bits > 0 with a NULL bitmap; nprobe == 0 on the probed call (the reference's spill walk depends on the
 *              filtered list lengths: OUT OF SCOPE); metric > VERS_METRIC_COSDIST on the exhaustive call; a handle sharded by cluster
 *              (world > 1: OUT OF SCOPE).  VERS_ERR_INSUFFICIENT no centroids on the probed call, as in vers_ivf_search.
 *   out of scope: nprobe == 0, the flat corpus handle.  (A prepared, reusable filter object: DONE, vers_ivf_filter_prepare and
 *              vers_ivf_search_prepared_dev / _exhaustive_prepared_dev, further below.)  (Handles sharded by cluster: refused HERE;
 *              vers_ivf_search_filtered_sharded_dev / _partial_dev and their exhaustive twins, further below.  A filter per query: the _multi
 *              calls below.  A depth per query, for filters that leave nprobe lists short of top_k rows: the _adaptive calls below.)
 * vers_ivf_filter_stats (measurement hook; functions of the data and the plan alone): out4 = the most recent filtered call of the handle,
 * out4_total = over the handle's life; either may be NULL.  [0] tile visits the plan implied (64-row tiles of every work item, counted once
 * per item and scan pass), [1] tile visits actually loaded, [2] items skipped before their first load, [3] allowed storage rows (popcount
 * of the tile mask).  Bytes not read = ([0] - [1]) * 64 * ld * 4.  In the scan-timing ring (vers_ivf_scan_times) a filtered call leaves
 * the mask kernel's record, then one record per scan pass. */
int32_t vers_ivf_search_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                 const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
int32_t vers_ivf_search_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                     const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_ids_dev, float* out_dist_dev,
                                     uint32_t* out_count_dev, void* stream);
int32_t vers_ivf_search_exhaustive_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                                            uint32_t metric, const uint64_t* allowed_bits, uint64_t n_bits, uint64_t* out_ids, float* out_dist,
                                            uint32_t* out_count);
int32_t vers_ivf_search_exhaustive_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                                uint32_t metric, const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_ids_dev,
                                                float* out_dist_dev, uint32_t* out_count_dev, void* stream);
/* FILTERED top-k search with a FILTER PER QUERY: one batch whose queries belong to different allowed sets (tenants, ACLs, time windows).
 *   semantics: nothing new.  With filter_of[q] = f, row q of a _multi call is bit for bit (ids, order, distance bits, out_count[q]) row q of
 *              vers_ivf_search_filtered / vers_ivf_search_exhaustive_filtered made with bitmap f on the same handle, with the same queries,
 *              top_k and nprobe / metric.  The ranking of the lists, both result orders, counts of 0, any top_k and any nprobe >= 1, the
 *              output layout, the handle, lease and stream rules and vers_ivf_poll's latching on the _dev calls are the per-call ones, to
 *              the letter.
 *   filters  : n_filters bitmaps of u64 words, bitmap f at filters + f * filter_stride_words, filter_stride_words >= ceil(n_bits / 64).
 *              One n_bits serves all bitmaps with the meaning it has above: ids >= n_bits are not allowed, bits of a bitmap's last word at
 *              or beyond n_bits are ignored, bits of removed ids or ids >= n select nothing; n_bits == 0: every filter is empty, filters may
 *              be NULL.  Words between two bitmaps (a stride larger than needed) are never read as bits.
 *   filter_of: [b] u32, the bitmap query q uses.  At most VERS_FILTER_MAX distinct bitmaps per call: a batch with more distinct allowed
 *              sets is split by the caller.  A query that may see everything uses a bitmap of ones covering n.
 *   errors   : VERS_ERR_INVALID n_filters == 0 with b > 0; n_filters > VERS_FILTER_MAX; n_bits > 0 with NULL filters; NULL filter_of with
 *              b > 0; filter_stride_words < ceil(n_bits / 64); and the per-call ones (nprobe == 0, the metric, a handle sharded by cluster,
 *              the exhaustive call's batch too large).  VERS_ERR_INSUFFICIENT no centroids on the probed call.  Host-pointer calls: an entry
 *              of filter_of >= n_filters is VERS_ERR_INVALID.  _dev calls: filter_of is NOT read on the host; an entry >= n_filters selects
 *              the EMPTY filter (out_count[q] = 0) and never indexes outside the masks.  VERS_ERR_NAN counts a NaN distance only for a
 *              (query, row) pair whose row is allowed for THAT query and scanned: a NaN row allowed by a bitmap no query of the batch uses,
 *              or only for queries that do not probe its list, is not an error.
 *   scan     : the mask pass writes a u64 per storage row (bit f: bitmap f allows the row's vector) and one per 64-row tile (bit f: bitmap f
 *              allows some row of it); a tile is loaded for a group of queries when some query of the group is allowed a row of it, and each
 *              query takes only its own rows from it.  b == 0 is a no-op, top_k == 0 zeroes the counts.  The host-pointer calls stage the
 *              bitmaps and filter_of through the workspace.
 *   stats    : vers_ivf_filter_stats covers these calls: [0..2] as above (a tile counts as loaded when some live query of the work item is
 *              allowed a row of it); [3] = allowed (bitmap, storage row) pairs, summed over the call's n_filters bitmaps.  The scan-timing
 *              ring gets the mask kernel's record, then one per scan pass.
 *   out of scope (refused, not approximated): the flat corpus handle, nprobe == 0, more than VERS_FILTER_MAX
 *              bitmaps per call, a prepared (reusable) mask (DONE: vers_ivf_filter_prepare and the _prepared_dev calls, further below), re-grouping a list's queries by filter in the plan, any fp16 / matrix-core
 *              pre-filter.  (Sharded handles and partials: refused HERE; the _filtered_sharded_dev / _filtered_partial_dev calls further
 *              below, with a non-NULL filter_of_dev.  A filter per query on the range calls: the vers_ivf_range_search_*filtered_multi calls below.  A depth per
 *              query: vers_ivf_search_filtered_multi_adaptive below.) */
#define VERS_FILTER_MAX 64
int32_t vers_ivf_search_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                       const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                       const uint32_t* filter_of /* [b] */, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
int32_t vers_ivf_search_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe,
                                           const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                           const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                           void* stream);
int32_t vers_ivf_search_exhaustive_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                                                  uint32_t metric, const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters,
                                                  uint64_t n_bits, const uint32_t* filter_of /* [b] */, uint64_t* out_ids, float* out_dist,
                                                  uint32_t* out_count);
int32_t vers_ivf_search_exhaustive_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                                      uint32_t metric, const uint64_t* filters_dev, uint64_t filter_stride_words,
                                                      uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_ids_dev,
                                                      float* out_dist_dev, uint32_t* out_count_dev, void* stream);
int32_t vers_ivf_filter_stats(vers_ivf_t* h, uint64_t* out4, uint64_t* out4_total);
/* ADAPTIVE DEPTH for the probed filtered calls: every query of the batch probes lists until enough allowed rows are in reach, instead of one
 * nprobe sized for the batch's worst query.  Under a selective filter out_count[q] of the plain calls is often below top_k; the depth a query
 * needs depends on its list ranking and on the allowed rows per list only, and the device knows both before the scan starts.
 *   semantics: nothing new for the results.  For query q let L_0, L_1, ... be its lists in the order vers_ivf_search ranks them, a_j the number
 *              of live rows of L_j that q's bitmap allows, A_P = a_0 + ... + a_{P-1}, P_min = min(nprobe_min, k), P_max = min(nprobe_max, k).
 *              P_q is the smallest P in [P_min, P_max] with A_P >= min_allowed, or P_max if there is none (min_allowed == 0: P_q = P_min).
 *              Lists the filter empties, and empty lists, count as probed.  Row q of an adaptive call is bit for bit (ids, order, distance
 *              bits, out_count[q]) row q of vers_ivf_search_filtered -- of vers_ivf_search_filtered_multi for the _multi calls -- made with
 *              nprobe = P_q on the same handle, with the same queries, top_k and bitmap(s).  min_allowed = top_k asks for full results
 *              wherever nprobe_max lists hold them.
 *   out_nprobe: [b] u32, out_nprobe[q] = P_q; may be NULL.  The _dev calls take a device array.  top_k == 0: nothing is probed, zeros.
 *   rules    : the bitmap / filters, n_bits, filter_of and VERS_FILTER_MAX, the output layout, the handle, lease and stream rules,
 *              vers_ivf_poll's latching on the _dev calls, b == 0 (a no-op), top_k == 0 (zeroes the counts) and the staging of the
 *              host-pointer calls are those of the filtered calls above, to the letter.  On the _dev calls an entry of filter_of at or
 *              beyond n_filters selects the empty filter: every a_j is 0, so P_q = P_max and out_count[q] = 0.  VERS_ERR_NAN counts a NaN
 *              distance only on a (query, row) pair whose row is allowed for that query and lies in one of its P_q lists.
 *   errors   : VERS_ERR_INVALID nprobe_min == 0; nprobe_max < nprobe_min; and those of the filtered calls (a handle sharded by cluster
 *              included).  VERS_ERR_INSUFFICIENT no centroids.
 *   cost     : behind the mask pass one small kernel counts the allowed rows per list (per bitmap and list on the _multi calls), and the
 *              lists are ranked to P_max for every query.  The planning tables and the partial result slots are sized by b x P_max, as those
 *              of the plain call at nprobe = nprobe_max; the SCAN visits each query's P_q lists only.
 *   stats    : vers_ivf_filter_stats covers these calls as it covers the plain ones.  The scan-timing ring gets the mask kernel's record,
 *              then the allowed-count kernel's, then one per scan pass.
 *   out of scope (refused or absent, not approximated): the range calls (no top_k to aim for), the exhaustive calls (nothing to adapt),
 *              nprobe == 0.  (Sharded handles and partials: refused HERE; vers_ivf_search_filtered_sharded_dev / _partial_dev with a
 *              vers_adaptive_t, further below.) */
int32_t vers_ivf_search_filtered_adaptive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                                          uint32_t nprobe_min, uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* allowed_bits,
                                          uint64_t n_bits, uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint32_t* out_nprobe);
int32_t vers_ivf_search_filtered_adaptive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                              uint32_t nprobe_min, uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* allowed_bits_dev,
                                              uint64_t n_bits, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                              uint32_t* out_nprobe_dev, void* stream);
int32_t vers_ivf_search_filtered_multi_adaptive(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, uint32_t top_k,
                                                uint32_t nprobe_min, uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* filters,
                                                uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                const uint32_t* filter_of /* [b] */, uint64_t* out_ids, float* out_dist, uint32_t* out_count,
                                                uint32_t* out_nprobe);
int32_t vers_ivf_search_filtered_multi_adaptive_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                                    uint32_t nprobe_min, uint32_t nprobe_max, uint32_t min_allowed, const uint64_t* filters_dev,
                                                    uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                    const uint32_t* filter_of_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                                    uint32_t* out_count_dev, uint32_t* out_nprobe_dev, void* stream);
/* FILTERED RANGE search (extension): every ALLOWED vector within a radius -- dedup or threshold retrieval inside one tenant, a time window,
 * an ACL.  The composition of the range calls and the filtered top-k calls above, and nothing else:
 *   semantics: a filter is a VIRTUAL REMOVAL, exactly as in vers_ivf_search_filtered.  With A the set of allowed vec ids, a filtered range call
 *              returns, bit for bit (limits, ids, order, distance bits, *out_total), what the unfiltered range call of the same mode --
 *              vers_ivf_range_search / vers_ivf_range_search_exhaustive -- returns on an index from which every vec id not in A has been
 *              removed by vers_ivf_remove_batch.  The index itself is not touched.
 *   bitmap   : that of vers_ivf_search_filtered, to the letter: u64 words, one bitmap per call shared by the batch; n_bits valid bits, ids
 *              >= n_bits are not allowed, bits of the last word at or beyond n_bits are ignored; bits of removed ids or of ids >= n select
 *              nothing; n_bits == 0 (allowed_bits may then be NULL) is the empty filter: total 0, every limit 0.
 *   layout, order, radii, protocol: those of the range calls, to the letter.  CSR (out_lims [b + 1], out_lims[b] = *out_total); default order
 *              ascending (distance, probe rank, list position) on the probed call, ascending (distance, vec id) on the exhaustive call;
 *              flags & VERS_RANGE_WALK_ORDER: probe rank then list position / storage order, restricted to the allowed rows; radius[q] per
 *              query, a plain f32 `<=`.  Synchronous; *out_total is always the full count; *out_total > cap: VERS_OK, out_lims complete,
 *              out_ids / out_dist UNTOUCHED; cap == 0 with NULL arrays is the size query; b == 0 is a no-op with *out_total = 0.
 *   scan     : rows outside A are NOT SCANNED, in the count pass or in the fill pass: a 64-row storage tile without an allowed row is never
 *              loaded, a work item without one returns before its first load.  A NaN distance on a disallowed row is therefore not an
 *              error; on an ALLOWED scanned row it is VERS_ERR_NAN, outputs untouched.  The scan is the exact ordered f32 chain over the
 *              f32 rows.
 *   handle   : the way range searches take it -- shared, one leased workspace, excluded by add / remove / compact.  _dev: every pointer but
 *              out_total is a device pointer (the bitmap too), the work is queued on `stream` and the call waits for it.  The host-pointer
 *              calls stage the bitmap through the workspace.  A filtered range call neither consumes nor starts a vers_ivf_coarse_ahead_dev
 *              preparation.
 *   errors   : the union of the parents', checked before the device is touched where the parents do so.  VERS_ERR_INVALID a NaN radius,
 *              nprobe == 0, unknown flag bits, n_bits > 0 with a NULL bitmap, metric > VERS_METRIC_COSDIST on the exhaustive call, a handle
 *              sharded by cluster (world > 1: OUT OF SCOPE), more than 2^32 - 1 results or 2^32 - 1 slots in one call (split the batch).
 *              VERS_ERR_INSUFFICIENT no centroids on the probed call (a streamed upload in progress is seen as an empty index); the
 *              exhaustive call on such a handle: VERS_OK, total 0, every limit 0.  VERS_ERR_NAN as above.  VERS_ERR_HIP scratch for the
 *              result staging did not fit, outputs untouched.
 *   out of scope (refused, not approximated): the flat corpus handle, a prepared (reusable) filter object (DONE: vers_ivf_filter_prepare and the _prepared_dev calls, further below), any fp16 / matrix-core
 *              pre-filter.  (Sharded handles and partials: refused HERE; vers_ivf_range_search_filtered_sharded_dev / _partial_dev and
 *              their exhaustive twins, further below.  A filter per query: the _multi calls below.)
 * vers_ivf_filter_stats covers these calls: [3] comes from the mask kernel; [0..2] -- planned tile visits, loaded tile visits, items skipped
 * before their first load -- are counted in the COUNT pass only, so they do not depend on the radius: what the fill pass skips for lack of
 * hits is range search's own saving, not the filter's.  vers_range_phases counts these calls; its slot [3] then also covers the mask kernel.
 * In the scan-timing ring (vers_ivf_scan_times) a filtered range call leaves the mask kernel's record and none for the range passes. */
int32_t vers_ivf_range_search_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius /* [b] */,
                                       uint32_t nprobe, uint32_t flags, const uint64_t* allowed_bits, uint64_t n_bits,
                                       uint64_t* out_lims /* [b+1] */, uint64_t* out_ids, float* out_dist, uint64_t cap, uint64_t* out_total);
int32_t vers_ivf_range_search_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                           uint32_t nprobe, uint32_t flags, const uint64_t* allowed_bits_dev, uint64_t n_bits,
                                           uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                           uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_exhaustive_filtered(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b,
                                                  const float* radius /* [b] */, uint32_t metric, uint32_t flags, const uint64_t* allowed_bits,
                                                  uint64_t n_bits, uint64_t* out_lims /* [b+1] */, uint64_t* out_ids, float* out_dist,
                                                  uint64_t cap, uint64_t* out_total);
int32_t vers_ivf_range_search_exhaustive_filtered_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                      const float* radius_dev, uint32_t metric, uint32_t flags,
                                                      const uint64_t* allowed_bits_dev, uint64_t n_bits, uint64_t* out_lims_dev,
                                                      uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                                      uint64_t* out_total /* host */, void* stream);
/* FILTERED RANGE search with a FILTER PER QUERY: one batch whose queries belong to different allowed sets, everything within a radius.  The
 * composition of the filtered range calls and the top-k _multi calls above, and nothing else:
 *   semantics: nothing new.  With filter_of[q] = f, query q's CSR segment of a _multi call holds, bit for bit (count, ids, order, distance
 *              bits), query q's segment of vers_ivf_range_search_filtered / vers_ivf_range_search_exhaustive_filtered made with bitmap f on
 *              the same handle, with the same queries, radii, nprobe / metric and flags.  out_lims is the running sum, *out_total the full
 *              count.
 *   filters, filter_stride_words, n_filters, n_bits, filter_of: those of vers_ivf_search_filtered_multi, to the letter (n_bits == 0 with NULL
 *              filters included: every filter is empty, total 0, every limit 0).
 *   layout, order, radii, protocol, handle: those of the filtered range calls, to the letter.  *out_total > cap: VERS_OK, out_lims complete,
 *              out_ids / out_dist UNTOUCHED; cap == 0 with NULL arrays is the size query; b == 0 is a no-op with *out_total = 0.  _dev: every
 *              pointer but out_total is a device pointer (the bitmaps and filter_of too).  The host-pointer calls stage the bitmaps (packed
 *              to ceil(n_bits / 64) words each) and filter_of through the workspace.
 *   scan     : the mask pass of the top-k _multi calls, once per call and before the count pass.  A tile is loaded for a group of queries when
 *              some query of the group is allowed a row of it, in the count pass and in the fill pass alike, and each query takes only its
 *              own rows from it.  VERS_ERR_NAN counts a NaN distance only for a (query, row) pair whose row is allowed for THAT query and
 *              scanned; outputs untouched.
 *   errors   : the union of the parents', checked before the device is touched where the parents do so.  VERS_ERR_INVALID a NaN radius,
 *              nprobe == 0, unknown flag bits, n_filters == 0 with b > 0, n_filters > VERS_FILTER_MAX, n_bits > 0 with NULL filters, NULL
 *              filter_of with b > 0, filter_stride_words < ceil(n_bits / 64), metric > VERS_METRIC_COSDIST on the exhaustive call, a handle
 *              sharded by cluster, more than 2^32 - 1 results or 2^32 - 1 slots in one call.  VERS_ERR_INSUFFICIENT no centroids on the probed
 *              call; the exhaustive call on such a handle: VERS_OK, total 0, every limit 0.  Host-pointer calls: an entry of filter_of >=
 *              n_filters is VERS_ERR_INVALID.  _dev calls: filter_of is NOT read on the host; an entry >= n_filters selects the EMPTY filter
 *              (query q's segment is empty) and never indexes outside the masks.
 *   stats    : vers_ivf_filter_stats covers these calls: [0..2] from the COUNT pass only (a tile counts as loaded when some live query of the
 *              work item is allowed a row of it), [3] = allowed (bitmap, storage row) pairs from the mask kernel.  vers_range_phases counts
 *              these calls, its slot [3] covering the mask kernel; the scan-timing ring gets the mask kernel's record and none for the range
 *              passes.
 *   out of scope (refused, not approximated): the flat corpus handle, nprobe == 0, more than VERS_FILTER_MAX
 *              bitmaps per call, a prepared (reusable) mask (DONE: vers_ivf_filter_prepare and the _prepared_dev calls, further below), re-grouping a list's queries by filter in the plan, any fp16 / matrix-core
 *              pre-filter.  (Sharded handles and partials: refused HERE; the range _filtered_sharded_dev / _filtered_partial_dev calls
 *              further below, with a non-NULL filter_of_dev.) */
int32_t vers_ivf_range_search_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b, const float* radius /* [b] */,
                                             uint32_t nprobe, uint32_t flags, const uint64_t* filters, uint64_t filter_stride_words,
                                             uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of /* [b] */,
                                             uint64_t* out_lims /* [b+1] */, uint64_t* out_ids, float* out_dist, uint64_t cap, uint64_t* out_total);
int32_t vers_ivf_range_search_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                                 uint32_t nprobe, uint32_t flags, const uint64_t* filters_dev, uint64_t filter_stride_words,
                                                 uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_lims_dev,
                                                 uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total /* host */,
                                                 void* stream);
int32_t vers_ivf_range_search_exhaustive_filtered_multi(vers_ivf_t* h, const float* queries, uint64_t q_stride_bytes, uint32_t b,
                                                        const float* radius /* [b] */, uint32_t metric, uint32_t flags, const uint64_t* filters,
                                                        uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                        const uint32_t* filter_of /* [b] */, uint64_t* out_lims /* [b+1] */, uint64_t* out_ids,
                                                        float* out_dist, uint64_t cap, uint64_t* out_total);
int32_t vers_ivf_range_search_exhaustive_filtered_multi_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                            const float* radius_dev, uint32_t metric, uint32_t flags, const uint64_t* filters_dev,
                                                            uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                            const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                                            float* out_dist_dev, uint64_t cap, uint64_t* out_total /* host */, void* stream);
/* SHARDED range search: the range calls on handles sharded by cluster (vers_ivf_set_shard / vers_ivf_build_sharded_dev), where the calls
 * above return VERS_ERR_INVALID.  The result is the unsharded index's, bit for bit -- limits, ids, order, distance bits.  Three layers:
 *
 * 1. A rank's PARTIAL: vers_ivf_range_search_partial_dev / vers_ivf_range_search_exhaustive_partial_dev run the count pass, prefix scan and
 *    fill pass over the lists (probed call) or rows (exhaustive call) THIS handle stores and return CSR of (key, id) pairs instead of
 *    (id, distance): out_keys_dev / out_ids_dev[out_lims_dev[q] .. out_lims_dev[q + 1]).
 *      keys     : probed call: (order bits of the distance) << 32 | the row's sequence number in the query's probe order, counted over the
 *                 GLOBAL list lengths -- the same number on every rank.  Exhaustive call: (order bits) << 32 | vec id.  Either way the keys
 *                 of one query are unique across ranks and ascend in the unsharded call's default order.
 *      order    : default = each query's run ascending by key.  VERS_RANGE_WALK_ORDER, probed call: this rank's walk order = ascending
 *                 sequence number (the key's low word).  Exhaustive call: VERS_ERR_INVALID -- storage order across ranks has no key the
 *                 ranks share; a walk order of the exhaustive search on sharded handles is out of scope.
 *      protocol : that of vers_ivf_range_search_dev on the LOCAL count: *out_total = this rank's count; > cap: VERS_OK, out_lims complete,
 *                 the arrays untouched; cap == 0 with NULL arrays is the size query.  Synchronous.
 *      handles  : sharded or not (world == 1: the whole result as keys).  Errors as the unsharded calls; the 2^32 - 1 limits apply to the
 *                 local counts.
 *
 * 2. The MERGE: vers_range_merge_dev turns `world` partials into the result, on `stream`, without a handle and without synchronising.
 *      input    : rank r's run for query q is keys_dev[r * rank_stride + rank_lims_dev[r * (b + 1) + q] ..), ids_dev the same way;
 *                 rank_lims_dev = every rank's out_lims, [world][b + 1] u64.  One gathered [world][2][T_max] buffer serves both arrays with
 *                 ids_dev = keys_dev + T_max and rank_stride = 2 * T_max.  Elements behind a rank's total (padding) are never read.
 *      output   : out_lims_dev[q] = SUM_r rank_lims[r][q] (q = 0 .. b; the last one the global total); out_ids_dev / out_dist_dev must hold
 *                 that many entries; the distance is decoded from the key's high word.  flags & VERS_RANGE_WALK_ORDER: the runs ascend by
 *                 the key's low word and are merged by it (partials made with the same flag).
 *      how      : one thread per gathered entry: its position is out_lims[q] + its index in its own run + the number of smaller keys in
 *                 every other rank's run (a bisection each).  No atomics: the same bytes on every run.
 *      errors   : VERS_ERR_INVALID, before anything touches a device: world == 0 (or > 65535), unknown flag bits, b > 0 with NULL
 *                 rank_lims_dev / out_lims_dev, rank_stride > 0 with a NULL array.  b == 0: no-op.  rank_stride == 0: the limits alone.
 *
 * 3. END TO END: vers_ivf_range_search_sharded_dev / vers_ivf_range_search_exhaustive_sharded_dev.  EVERY rank calls, with the same queries,
 *    radii, nprobe / metric, flags and THE SAME cap (the decision to exchange results depends on it).  comm: the callbacks of
 *    vers_ivf_build_sharded_dev, of which all_gather alone is used (synchronous, as in vers_ivf_remove_batch_dev); NULL on an unsharded
 *    handle (world 1: no exchange).
 *      exchange 1 : [b + 1] u64 per rank -- this rank's per-query counts and its local status word.  Afterwards every rank knows the global
 *                   limits and total, every rank's total and the worst status.  This is the AGREEMENT round: if any rank failed locally (a
 *                   NaN distance, a NaN radius, scratch that did not fit; option "test_fail_sharded" injects one), every rank returns the
 *                   first failing rank's status, outputs untouched, and nobody enters exchange 2.
 *      exchange 2 : only if 0 < total <= cap: ONE all_gather of 2 * 8 * max_r T_r bytes per rank (keys | ids, padded to the largest rank's
 *                   count T_r), then the merge.
 *      result     : *out_total = the GLOBAL total and out_lims_dev complete whenever the call returns VERS_OK; > cap: ids / distances
 *                   untouched, as in the unsharded protocol; the 2^32 - 1 limit applies to the global total (VERS_ERR_INVALID everywhere).
 *      errors     : before any exchange (so every rank must pass arguments that fail alike): a comm whose rank / world disagree with the
 *                   handle's, nprobe == 0, unknown flag bits, VERS_RANGE_WALK_ORDER on the exhaustive call, bad pointers, no centroids
 *                   (probed call).  After the agreement round a local failure (the gather buffers did not fit, VERS_ERR_COMM from a
 *                   callback) has no round left to be told in: the host aborts the group on a non-zero return, as for the sharded build.
 *    Synchronous, like every range call.  vers_range_phases counts the local part of these calls. */
int32_t vers_ivf_range_search_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                          uint32_t nprobe, uint32_t flags, uint64_t* out_lims_dev /* [b+1] */, uint64_t* out_keys_dev,
                                          uint64_t* out_ids_dev, uint64_t cap, uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_exhaustive_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                     const float* radius_dev, uint32_t metric, uint32_t flags, uint64_t* out_lims_dev,
                                                     uint64_t* out_keys_dev, uint64_t* out_ids_dev, uint64_t cap,
                                                     uint64_t* out_total /* host */, void* stream);
int32_t vers_range_merge_dev(const uint64_t* keys_dev, const uint64_t* ids_dev, uint64_t rank_stride /* elements */,
                             const uint64_t* rank_lims_dev /* [world][b+1] */, uint32_t world, uint32_t b, uint32_t flags,
                             uint64_t* out_lims_dev /* [b+1] */, uint64_t* out_ids_dev, float* out_dist_dev, void* stream);
int32_t vers_ivf_range_search_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm /* NULL = world 1 */, const float* queries_dev,
                                          uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe, uint32_t flags,
                                          uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                          uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_exhaustive_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm /* NULL = world 1 */, const float* queries_dev,
                                                     uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t metric,
                                                     uint32_t flags, uint64_t* out_lims_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                                     uint64_t cap, uint64_t* out_total /* host */, void* stream);
/* Process-wide switches: every one is a named option set here (or, for a process one does not control from inside, through the ONE
 * environment variable VERS_OPTIONS="name=value,name=value", read once; besides it the library reads only VERS_SHADOW and
 * VERS_ROWMAJOR, the two memory switches of INTEGRATION.md = options "shadow" / "rowmajor", and VERS_PRE_PRUNE = option "pre_prune").  Unknown name: VERS_ERR_INVALID.
 * Results are bit-identical under every setting: the switches choose between exact paths and pre-filters behind exact finishes.
 *  Memory:
 *   "shadow" (1)        indexes built / uploaded from now on keep an fp16 shadow of their rows for the list scans
 *                       (vers_ivf_shadow_state); 0 = none, and searches on existing handles read their f32 rows until it is 1 again.
 *   "rowmajor" (-1)     the row-major f32 copy the exact finish gathers from: -1 = kept while the rows take <= 1/4 of the device
 *                       (and "memory" is 0), 0 never, 1 always.
 *   "memory" (0)        0 = speed: f32 tiles + fp16 shadow + row-major f32 copy (2.7 x the f32 rows at d = 768); 1 = compact: ONE f32
 *                       copy -- tiles + shadow, 1.7 x --, the exact finish gathers its survivors from the tiles (16-byte pieces).
 *                       Read when an index is built / uploaded.
 *  Serving:
 *   "single_shadow" (1) a single query (b == 1, nprobe >= 1) streams the fp16 shadow and is finished exactly like a batch;
 *                       0 = the ordered-chain scan of the f32 rows.
 *   "host_spin" (1)     a host-pointer single-query call waits by spinning on the pinned status word (<= 2 ms); 0 = hipStreamSynchronize.
 *   "pre_min_batch" (4) the smallest batch whose list scan runs on the matrix cores when its lists are shared by fewer than two
 *                       queries on average; smaller batches run as consecutive single queries.
 *   "scan_reserve_cus" (-1 = auto: 64 while another batch of the handle is in flight on another stream, else 0) compute units the
 *                       persistent matrix-core list scan leaves free for the other batches' latency-bound kernels and the exchange.
 *   "pre_prune" (1)     the batched list scan (fp16 shadow, hi-only query blocks, squared L2) stops reading a 64-row tile once the
 *                       columns read so far prove that none of its rows can pass any of its queries' thresholds; 0 = every tile is
 *                       read whole.  Not on sharded handles (measured: only cost there).  "pre_prune_first" (2): the first 64-column
 *                       step boundary at which a wave tests.
 *   "pre_hot_single" (1) where tiles are abandoned early, the scan's blocks take the quads of the hot lists (some query's nearest:
 *                       the first of the work order) one at a time, so that thresholds are tight before the bulk is read; 0 = guided
 *                       runs of up to 8 quads from the first quad on.
 *   "pre_head" (1)      an int8 copy of the first "pre_head_cols" (384; multiples of 64 in 256 .. 512, clipped to the row length - 64)
 *                       columns of every stored row, built with the index (+ that many bytes per storage row; optional memory like the
 *                       shadow) -- where tiles are abandoned early the list scan then runs as three launches: the hot lists, a filter
 *                       that rules whole cold quads out from the int8 head (half the bytes of the fp16 prefix), the cold quads it left.
 *                       Results are bit-identical.  Read when the index is built / uploaded / compacted (whether there is a head) and
 *                       per search (whether it is used); add, add_batch and remove_batch invalidate the head until the next
 *                       vers_ivf_compact (vers_ivf_head_state).  0 = no head, one launch.  "pre_head_backoff" (1): after a scan in which
 *                       fewer than 1/8 of the quads the filter tested were ruled out (rows without cluster contrast) the handle's
 *                       next 64 batches run as one launch, then the filter is tried again; 0 = never back off.
 *   "pre_ball" (1)      sub-cluster balls per list, derived with the int8 head (up to 32 fp16 centres per list, a radius and the smallest
 *                       |x|^2 each; at most 64 x the row length bytes per list): inside the three-launch scan a pass in front of the
 *                       head's filter rules cold quads out from the centres alone, and the filter reads the heads of the quads that
 *                       are left.  Results are bit-identical.  Read when the index is built / uploaded / compacted and per search;
 *                       invalidated with the head (vers_ivf_ball_state).  "pre_ball_cut" (900): the farthest-point cut of the derive
 *                       pass in thousandths of sqrt(max |x|^2); a list that needs more than 32 sub-clusters at the cut gets none.
 *                       "pre_ball_min_quads" (0 = twice the compute units the scan uses): cold quads below which the pass stands aside.
 *   "scan_events" (2)   HIP event records around list-scan launches (vers_ivf_last_scan / vers_ivf_scan_times): 1 always, 0 never,
 *                       2 for batches only (the two records cost a single-query call 5.5-6 us).
 *  A/B and forced paths (tests, measurements):
 *   "gemm_x3" (3)       bit 0 the k-means assign contraction, bit 1 the coarse quantiser's contraction as three bf16 MFMA products of
 *                       hi/lo-split operands instead of the f32 MFMA kernel.
 *   "prescan" (1)       0 = ordered chains for batches too, 2 = every list-scan certificate fails (the exact re-scan runs).
 *   "coarse" (0)        1 = the batched coarse quantiser always exact, 2 = every coarse certificate fails.
 *   "assign" (0)        k-means assign: 1 = never on the matrix cores, 2 = always (default: from 1e11 flop per pass).
 *   "assign_terms" (0)  the assign contraction's first filter: 1 = ONE product of fp16 operands (a third of the MFMAs; the points it leaves
 *                       open go to the tile-limited exact re-scan), 3 = all three products of the bf16 hi/lo split, 0 = probe per build.
 *   "assign_glds" (-1)  the one-product filter with both operands fp16 in memory, staged by LDS-DMA in whole cache lines: 1 = always, 0 = never
 *                       (the register-staged kernel that converts the f32 batch while it stages it), -1 = from 4096 centroids on.
 *   "pre_narrow" (0), "pre_wide" (1), "pre_hi_only" (0)   the list scan's query-block width (16 / 64 queries) and fp16 hi-only query blocks.
 *   "wide_k" (1)        results of 49 .. 200 keys (batches, nprobe >= 1) stay on the matrix-core list scan with candidate lists four keys
 *                       per lane wide; 0 = the ordered chains, 64 ranks per pass.
 *   "coarse1" (1), "scan1t" (1), "ref_as_nprobe1" (1), "assign_tiles" (1), "assign_tiles_min" (64), "seg_rows" (0), "pre_slack" (0),
 *   "upload_stage_mb" (256), "add_batch_rows" (131072), "remove_batch_ids" (1048576), "compact_fused" (1)   kernel-choice and sizing knobs of
 *                       DESIGN.md section 5.  "seg_rows", when non-zero, also fixes the row-segment length of the two exhaustive range
 *                       scans (vers_flat_range_search, vers_ivf_range_search_exhaustive), rounded up to 64 and capped at what one buffer
 *                       descriptor addresses; vers_flat_search and vers_ivf_search_exhaustive keep their own sizing.
 *   "fetch_lds_min" (64; never for rows of more than 256 columns) requests for one 64-row tile from which vers_ivf_fetch's tile gather
 *                       turns the whole tile through LDS instead of reading the wanted rows' 16-byte pieces directly (1 = always, above 64 = never).  "fetch_map" (1): 0 = no vec id ->
 *                       storage row map on the handle, every fetch builds a table of its own requests (what a failed allocation does).
 *   "scan_debug" (0), "poison_alloc" (-1), "poison_slack_bits" (-1), "test_fail_sharded" (0)   diagnosis: phase stamps / skipped
 *                       phases, new device buffers filled with a byte, slack rows filled with an f32 bit pattern, the next n sharded
 *                       searches fail locally. */
int32_t vers_set_option(const char* name, int64_t value);
/* Device memory the library holds in this process right now (rows, ids, scratch of every handle) and its high-water
 * mark since the last reset -- lets a test assert that no rank of a sharded build ever allocated the whole corpus. */
int32_t vers_mem_stats(uint64_t* out_bytes_now, uint64_t* out_bytes_peak, int32_t reset_peak);
/* Local part of search_approximate: out_keys/out_ids [b*top_k], kKeyMax (all ones) padded. */
int32_t vers_ivf_search_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                    uint32_t top_k, uint32_t nprobe, uint64_t* out_keys_dev,
                                    uint64_t* out_ids_dev, void* stream);
/* Local part of utils::search_exhaustive (utils.rs:68-82) over the rows this rank stores: keys = (order-preserving
 * distance bits << 32) | vec_id -- the reference's stable order, ties to the lower index -- so the same all-gather +
 * vers_topk_merge_dev (any nprobe >= 1: global top-k by key) yields the brute-force result of the whole corpus. */
int32_t vers_ivf_search_exhaustive_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                               uint32_t top_k, uint32_t metric, uint64_t* out_keys_dev,
                                               uint64_t* out_ids_dev, void* stream);
/* Merge of the gathered partials into final results: rank r's keys at keys_dev + r*rank_stride
 * ([b][top_k], rank_stride in elements), ids likewise -- so one all-gathered [world][2][b][top_k]
 * buffer serves both with rank_stride = 2*b*top_k. */
int32_t vers_topk_merge_dev(const uint64_t* keys_dev, const uint64_t* ids_dev, uint64_t rank_stride, uint32_t world,
                            uint32_t b, uint32_t top_k, uint32_t nprobe, uint64_t* out_ids_dev,
                            float* out_dist_dev, uint32_t* out_count_dev, void* stream);

/* Bytes of the three copies of the stored rows this handle holds: the f32 tiles (always), the fp16 shadow the batched
 * list scan streams (vers_ivf_shadow_state), the row-major f32 copy the exact finish gathers from (kept whenever the rows
 * take at most a quarter of the device's memory; VERS_ROWMAJOR=0 switches it off).  0 = that copy does not exist. */
int32_t vers_ivf_layout_bytes(vers_ivf_t* h, uint64_t* out_rows, uint64_t* out_shadow, uint64_t* out_rowmajor);

/* ---- sharded search WITHOUT the host in the loop ----------------------------------------------------------------
 * The ONE exchange of a sharded search (all-gather of the per-rank partial top-k) as a stream-ordered
 * callback: all_gather_async queues, on `stream`, an all-gather of `bytes` bytes per rank from send_dev into recv_dev
 * ([world][bytes], rank order) and returns without synchronising.  include/vers_comm_rccl.h fills one from an
 * ncclComm_t (ncclAllGather on the batch's stream: RCCL over xGMI); tests put gloo behind the same signature. */
typedef struct vers_gather {
  void* ctx;
  uint32_t rank, world;
  int32_t (*all_gather_async)(void* ctx, const void* send_dev, void* recv_dev, uint64_t bytes, void* stream);
} vers_gather_t;
/* search_approximate over lists sharded by cluster (vers_ivf_set_shard / vers_ivf_build_sharded_dev), end to end on
 * `stream`: local partial search -> g->all_gather_async of [2][b][top_k] u64 (keys | ids) -> merge of the world's
 * partials (vers_topk_merge_dev) into out_*_dev.  Nothing synchronises; the gather buffers belong to the workspace the
 * call leases (one per stream in flight), so batches kept in flight on several streams overlap.  Every rank must issue
 * its calls in the same order.  g == NULL: a single process, no exchange (same as vers_ivf_search_dev).  Results are bit-identical to the
 * unsharded index; statuses latch per stream (vers_ivf_poll). */
int32_t vers_ivf_search_sharded_dev(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev, uint64_t ldq_floats,
                                    uint32_t b, uint32_t top_k, uint32_t nprobe, uint64_t* out_ids_dev,
                                    float* out_dist_dev, uint32_t* out_count_dev, void* stream);
/* utils::search_exhaustive (utils.rs:68-82) over the rows sharded across the ranks, the same way. */
int32_t vers_ivf_search_exhaustive_sharded_dev(vers_ivf_t* h, const vers_gather_t* g, const float* queries_dev,
                                               uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t metric,
                                               uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                               void* stream);

/* ---- UPDATE, FETCH and SEARCH BY ID on handles SHARDED BY CLUSTER ---------------------------------------------------------------------
 * vers_ivf_update_batch[_dev], vers_ivf_fetch[_dev] and vers_ivf_search_by_id[_dev] refuse a sharded handle (world > 1); these three take
 * one.  They have no semantics of their own: EVERY rank calls with the same ids (and, for the update, the same rows), exactly as the sharded
 * vers_ivf_add_batch and vers_ivf_remove_batch_dev are called, and every rank receives, bit for bit, what the matching _dev call returns on
 * the UNSHARDED index holding the same five fields -- but out_counts[3] of the update: storage re-layouts are this rank's own, 0 or 1.
 * comm == NULL (and g == NULL) on an unsharded handle: the call IS the existing _dev call.
 *   the "where" round : whether an id is live, and in which list, is known to the list's owner alone.  ONE comm->all_gather of 4 * (n + 1)
 *              bytes per rank, shared by the three calls: word i = the cluster (< k) of vec_ids[i] if this rank stores it in a list, else
 *              0xFFFFFFFF; word n = this rank's local status (0, or the VERS_ERR_* of a local failure such as scratch that did not fit;
 *              option "test_fail_sharded" injects one).  It is the agreement round, as in vers_ivf_range_search_sharded_dev: if any rank's
 *              status word is non-zero every rank returns the first failing rank's status, nothing written, no further exchange.  An id
 *              claimed by two ranks, or by a rank that does not own the claimed list: VERS_ERR_HIP (inconsistent index), nothing written.
 *   before any exchange, the same on every rank, 0 callbacks, outputs and index untouched: every refusal of the unsharded call that
 *              follows from the arguments, the centroids or n (an id >= n, a duplicate id or a NaN distance of the update, no centroids, a
 *              streamed upload in progress, unknown flags, VERS_BYID_EXCLUDE_SELF with nprobe == 0), a comm / g whose rank or world
 *              disagree with the handle, world > 1 with a NULL comm.
 *   fetch    : after the where round every rank knows each request's cluster, status and owner; a call without out_rows_dev ends there
 *              (1 callback).  Rows travel in chunks of option "add_batch_rows" requests: for chunk j every rank sends the rows it found
 *              among requests [jR, (j+1)R), packed in request order at a pitch of exactly d floats and padded to the largest rank's count
 *              of that chunk -- ONE all_gather per chunk, a chunk in which no rank found anything is skipped: 1 + (non-empty chunks)
 *              callbacks per call.  A device kernel places the rows; a request in no list gets d zeros; columns d .. ld_floats - 1 are
 *              never written.  Synchronous like vers_ivf_fetch_dev; takes the handle shared.  vers_fetch_phases [7] = time in callbacks.
 *              A failure of this rank AFTER the where round (scratch for a chunk that does not fit) has no round left to be told in:
 *              the peers are inside their callback and the host aborts the group, as for the sharded mutators.
 *   update   : mark, assign, the local pass over the stored rows, the where round, then a resolve pass over the gathered table, from
 *              which every rank derives the same status per row (stayed: old cluster == new; moved; skipped: no claimer) and the same
 *              per-list out / in counts, hence the same new GLOBAL lengths.  The owner of a row that stays overwrites it in place; the
 *              owner of a list that loses rows compacts it; the owner of a list that gains rows merges the movers in from the CALL's
 *              rows at their sorted places (every rank is handed the rows anyway: no row crosses ranks) and, when an owned list outgrows
 *              its capacity, re-lays out its own storage.  Afterwards every handle is what vers_ivf_set_shard + vers_ivf_upload of the
 *              updated fields + removal of the ids in no list would hold.  The first byte of the index is written after the agreement:
 *              ONE callback per call.  A failure after it has no round left to be told in: the host aborts the group, as for the other
 *              sharded mutators.  Synchronous; holds the handle exclusively.  The exchange is counted in vers_update_phases [6].  Prepared
 *              filters and fetch maps refresh on EVERY rank when anything moved anywhere.
 *   search by id : the where round over the b ids (an id in no list on any rank: VERS_ERR_INVALID on every rank after that one callback,
 *              nothing written), one row round that puts the query block into the call's workspace on every rank, then
 *              vers_ivf_search_sharded_dev unchanged (for VERS_BYID_EXCLUDE_SELF at top_k + 1, the own id dropped behind it): from there
 *              on results after the stream's work, status through vers_ivf_poll.  The call gives the handle back between the row round
 *              and the search: a mutator that was waiting runs in that gap, and the search then sees the index AFTER it (with the flag, a
 *              query id removed in the gap is no longer there and the last entry goes in its place).  Ranks issue their calls in one
 *              order, so every rank sees the same; a host that needs the search on the index the rows were read from does not mutate
 *              concurrently. */
int32_t vers_ivf_fetch_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm /* NULL = world 1 */, const uint64_t* vec_ids_dev, uint64_t n,
                                   float* out_rows_dev, uint64_t ld_floats, uint64_t* out_clusters_dev, uint8_t* out_status_dev,
                                   uint64_t* out_counts /* host [2] */, void* stream);
int32_t vers_ivf_update_batch_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm /* NULL = world 1 */, const uint64_t* vec_ids_dev,
                                          const float* rows_dev, uint64_t n, uint64_t ld_floats, uint64_t* out_clusters_dev,
                                          uint8_t* out_status_dev, uint64_t* out_counts /* host [4] */);
int32_t vers_ivf_search_by_id_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm, const vers_gather_t* g /* both NULL = world 1 */,
                                          const uint64_t* vec_ids_dev, uint32_t b, uint32_t top_k, uint32_t nprobe, uint32_t flags,
                                          uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev, void* stream);

/* ---- FILTERED search on handles SHARDED BY CLUSTER: partials, the merges' input, and the calls end to end ---------------------------
 * The filtered calls above refuse a sharded handle (world > 1); these nine take one.
 *   semantics: none of their own.  Call R the result of the matching existing filtered call on the UNSHARDED index -- the same data, lists,
 *              queries and bitmaps.  Every rank's partial, laid out as the all-gather lays it out and fed UNCHANGED into vers_topk_merge_dev
 *              (any nprobe >= 1) / vers_range_merge_dev, gives R bit for bit: ids, order, distance bits, counts, limits.  The _sharded_dev
 *              calls do that end to end and every rank gets R; with `adaptive`, out_nprobe is the unsharded adaptive call's on every rank.
 *   filters  : always in the _multi form -- filters_dev, filter_stride_words, n_filters, n_bits with the meaning they have above, indexed by
 *              GLOBAL vec id; every rank passes the same bits.  filter_of_dev == NULL: ONE bitmap for the whole batch, n_filters must be 1,
 *              the per-call kernels run and the rules are those of vers_ivf_search_filtered / vers_ivf_range_search_filtered, to the
 *              letter.  filter_of_dev != NULL: a bitmap per query, the per-query kernels, the rules of the _multi calls (an entry at or
 *              beyond n_filters selects the empty filter).
 *   partials : top-k: out_keys_dev / out_ids_dev [b * top_k], kKeyMax (all ones) padded, with the keys of vers_ivf_search_partial_dev
 *              (probed: order bits of the distance << 32 | the row's sequence number in the query's probe order over the GLOBAL list
 *              lengths) and vers_ivf_search_exhaustive_partial_dev (order bits << 32 | vec id); top_k >= 1; stream-ordered, nothing
 *              synchronises.  Range: CSR of (key, id) with the keys, the walk-order rule and the cap protocol (on the LOCAL count) of
 *              vers_ivf_range_search_*partial_dev; synchronous.  Handles sharded or not: at world 1 the partial is the whole result as keys.
 *   adaptive : NULL = plain depth; else `nprobe` is nprobe_max.  A query's depth depends on the allowed rows of EVERY list and a rank can
 *              count only the lists it stores.  vers_ivf_filter_allowed_len_dev: the mask pass + the count, out_len_dev[f * k + L] = the
 *              rows of list L bitmap f allows if this rank stores L, else 0 -- on an unsharded handle the true counts; every list has one
 *              owner, so the ranks' arrays ADD UP to the global counts.  A partial call takes those global counts (allowed_len_dev, required
 *              [n_filters][k]; filter_of_dev == NULL: [k]); a _sharded_dev call takes NULL and exchanges them itself.  Depth, sequence
 *              numbers and out_nprobe come from the global lengths and counts: identical on every rank.
 *   exchanges: the top-k _sharded_dev calls follow vers_ivf_search_sharded_dev: stream-ordered through g->all_gather_async, never
 *              synchronising, one gather per call, a rank that fails locally joining it with a poisoned partial (peers latch VERS_ERR_COMM
 *              at vers_ivf_poll).  An ADAPTIVE call gathers TWICE on the stream: n_filters * k u32 of local allowed counts (summed over the
 *              ranks on the device, then the plan), then the partials; a rank that fails locally joins both -- zeros in the first, the
 *              poisoned partial in the second.  The range _sharded_dev calls follow vers_ivf_range_search_sharded_dev: its agreement round
 *              (a local failure -- option "test_fail_sharded" injects one -- is every rank's status, outputs untouched), the same cap on
 *              every rank, synchronous comm->all_gather, 2 callbacks per call, 1 for the size query / a total beyond cap / a batch without
 *              a hit, 0 for a call refused from its arguments.  g / comm == NULL on an unsharded handle: the existing filtered call.
 *   errors   : the union of the filtered and the sharded calls'.  VERS_ERR_INVALID nprobe == 0 (OUT OF SCOPE); n_filters == 0 with b > 0;
 *              n_filters > VERS_FILTER_MAX; a NULL filter_of_dev with n_filters != 1; filter_stride_words < ceil(n_bits / 64); n_bits > 0
 *              with NULL filters; top_k == 0 (top-k calls); VERS_RANGE_WALK_ORDER on an exhaustive range partial or sharded call; a g /
 *              comm whose rank or world disagree with the handle; adaptive with nprobe_min == 0 or nprobe < nprobe_min; a NULL
 *              allowed_len_dev on an adaptive partial, a non-NULL one on a sharded call.  VERS_ERR_INSUFFICIENT no centroids on the probed
 *              calls.  VERS_ERR_NAN only for a (query, row) pair that is allowed, scanned and stored on THIS rank.
 *   stats    : vers_ivf_filter_stats covers the local part of every one of these calls.  An adaptive partial leaves no allowed-count record in
 *              the scan-timing ring (it counts nothing).
 *   out of scope: nprobe == 0, the flat corpus handle, a prepared (reusable) mask (DONE: vers_ivf_filter_prepare and the _prepared_dev calls, further below), a walk order of the exhaustive range search across ranks. */
typedef struct vers_adaptive { /* NULL = plain depth */
  uint32_t nprobe_min, min_allowed;
  const uint32_t* allowed_len_dev; /* partial call: GLOBAL counts [n_filters][k], required; sharded call: must be NULL */
  uint32_t* out_nprobe_dev;        /* nullable, [b] */
} vers_adaptive_t;
int32_t vers_ivf_filter_allowed_len_dev(vers_ivf_t* h, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                        uint64_t n_bits, uint32_t* out_len_dev /* [n_filters][k] */, void* stream);
int32_t vers_ivf_search_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                             uint32_t nprobe /* nprobe_max if adaptive */, const uint64_t* filters_dev,
                                             uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev,
                                             const vers_adaptive_t* adaptive, uint64_t* out_keys_dev, uint64_t* out_ids_dev, void* stream);
int32_t vers_ivf_search_exhaustive_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                        uint32_t top_k, uint32_t metric, const uint64_t* filters_dev,
                                                        uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                        const uint32_t* filter_of_dev, uint64_t* out_keys_dev, uint64_t* out_ids_dev,
                                                        void* stream);
int32_t vers_ivf_search_filtered_sharded_dev(vers_ivf_t* h, const vers_gather_t* g /* NULL = world 1 */, const float* queries_dev,
                                             uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t nprobe, const uint64_t* filters_dev,
                                             uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits, const uint32_t* filter_of_dev,
                                             const vers_adaptive_t* adaptive, uint64_t* out_ids_dev, float* out_dist_dev,
                                             uint32_t* out_count_dev, void* stream);
int32_t vers_ivf_search_exhaustive_filtered_sharded_dev(vers_ivf_t* h, const vers_gather_t* g /* NULL = world 1 */, const float* queries_dev,
                                                        uint64_t ldq_floats, uint32_t b, uint32_t top_k, uint32_t metric,
                                                        const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                                        uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_ids_dev,
                                                        float* out_dist_dev, uint32_t* out_count_dev, void* stream);
int32_t vers_ivf_range_search_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                   const float* radius_dev, uint32_t nprobe, uint32_t flags, const uint64_t* filters_dev,
                                                   uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                                   const uint32_t* filter_of_dev, uint64_t* out_lims_dev /* [b+1] */, uint64_t* out_keys_dev,
                                                   uint64_t* out_ids_dev, uint64_t cap, uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_exhaustive_filtered_partial_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                              const float* radius_dev, uint32_t metric, uint32_t flags,
                                                              const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                                              uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_lims_dev,
                                                              uint64_t* out_keys_dev, uint64_t* out_ids_dev, uint64_t cap,
                                                              uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_filtered_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm /* NULL = world 1 */, const float* queries_dev,
                                                   uint64_t ldq_floats, uint32_t b, const float* radius_dev, uint32_t nprobe, uint32_t flags,
                                                   const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                                   uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_lims_dev,
                                                   uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap, uint64_t* out_total /* host */,
                                                   void* stream);
int32_t vers_ivf_range_search_exhaustive_filtered_sharded_dev(vers_ivf_t* h, const vers_comm_t* comm /* NULL = world 1 */,
                                                              const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                              const float* radius_dev, uint32_t metric, uint32_t flags,
                                                              const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                                              uint64_t n_bits, const uint32_t* filter_of_dev, uint64_t* out_lims_dev,
                                                              uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                                              uint64_t* out_total /* host */, void* stream);

/* ---- PREPARED filters: masks kept across calls, refreshed when rows move ------------------------------------------------------------
 * Every filtered call above rebuilds its masks from the bitmaps: a pass over every storage row, per call.  A tenant or an access-control
 * set stays the same over thousands of queries; a vers_filter_t keeps its masks in an object the index handle owns.
 *   object   : vers_ivf_filter_prepare(_dev) COPIES the bitmaps -- the _multi form and meaning: n_filters <= VERS_FILTER_MAX bitmaps
 *              filter_stride_words apart, one n_bits for all, ids at or beyond n_bits not allowed -- and builds the masks for the index as it
 *              stands, synchronously, holding the handle shared like a search.  The caller's array may be freed or changed afterwards.  On a
 *              handle without an index (no centroids, or a streamed upload in progress) the masks are empty.  No update call: to change the
 *              bits, destroy the object and prepare a new one.  The handle keeps a registry: vers_ivf_destroy frees the objects still alive;
 *              an object of another handle is VERS_ERR_INVALID everywhere.  Its device bytes count in vers_mem_stats.
 *   holds    : what the per-call path leaves in its workspace, with the same content -- the per-call tile mask (needed when a search passes no
 *              filter_of), the per-query row / tile sets (needed when it passes one), allowed_len[n_filters][k] and the allowed total that
 *              feeds vers_ivf_filter_stats.  Each mask form is built at first need and then kept (prepare builds the per-call form of a
 *              one-bitmap object, the per-query form otherwise).
 *   searches : the four _prepared_dev calls are the _filtered_sharded_dev calls without g / comm and with `f` in the bitmaps' place.  No
 *              semantics of their own: each returns, bit for bit, what the matching vers_ivf_*_filtered_sharded_dev call with g / comm = NULL
 *              returns on the same handle in its current state, given the bitmaps f was prepared from -- ids, order, distance bits, counts /
 *              limits / total, out_nprobe, the latched status, the capacity protocol, all four slots of vers_ivf_filter_stats.
 *              (tiles_loaded / items_skipped of a PROBED batch with a filter per query are not reproducible between two runs of the same
 *              call, prepared or not: the plan deals a list's queries into work items in the order of an atomic counter, and an item's
 *              union of filters decides which tiles it loads.  tiles_planned, rows_allowed and every result are reproducible.)
 *              filter_of_dev == NULL needs an object of ONE bitmap (the per-call kernels); else the per-query kernels and the _multi rules
 *              (an entry at or beyond n_filters selects the empty filter).  adaptive->allowed_len_dev must be NULL: the object has the counts.
 *   staleness: at the start of a prepared search, or of vers_ivf_filter_refresh (on `stream`), the object is compared with the handle.  Rows
 *              MOVED since (build, upload, set_shard, a remove_batch that removed something, compact, an add / add_batch that re-laid-out
 *              storage): a full rebuild on the call's stream.  Rows only APPENDED in place (an add / add_batch into list slack): a tail
 *              refresh over the appended rows alone -- and nothing at all when every id handed out since is at or beyond n_bits.  Neither:
 *              nothing; the call launches no mask and no count kernel and leaves no mask record in vers_ivf_scan_times (a call that rebuilds
 *              or tail-refreshes leaves one).  A rebuild queued on one stream is waited for ON THE DEVICE by searches on other streams; no host
 *              synchronisation is added to the query path.
 *   threads  : prepared searches on one object may run from several threads and streams.  vers_ivf_filter_destroy (and vers_ivf_destroy)
 *              must NOT run while another thread is inside a call that uses the object: the caller orders them, as for the handle itself.
 *              A one-bitmap object that builds its second mask form after in-place adds it has not yet seen rebuilds and recounts in full.
 *   info     : out8 = n_filters | n_bits | device bytes held | full builds so far (prepare's and every form's first build included) | tail
 *              refreshes | searches served with no mask work at all | 1 if fresh against the handle now, else 0 | 0.
 *   errors   : those of the _filtered_sharded_dev calls, and VERS_ERR_INVALID for a NULL f, an f of another handle (or destroyed), a handle
 *              sharded by cluster (world > 1: OUT OF SCOPE), n_filters == 0 or > VERS_FILTER_MAX or a too small filter_stride_words at prepare.
 *   out of scope: handles sharded by cluster, nprobe == 0, the flat corpus handle, updating an object's bits in place, an incremental refresh
 *              after remove_batch / compact (a removal compacts every touched list from its first removed row on), host-pointer searches. */
typedef struct vers_filter vers_filter_t;
int32_t vers_ivf_filter_prepare(vers_ivf_t* h, const uint64_t* filters, uint64_t filter_stride_words, uint32_t n_filters, uint64_t n_bits,
                                vers_filter_t** out);
int32_t vers_ivf_filter_prepare_dev(vers_ivf_t* h, const uint64_t* filters_dev, uint64_t filter_stride_words, uint32_t n_filters,
                                    uint64_t n_bits, vers_filter_t** out);
int32_t vers_ivf_filter_refresh(vers_ivf_t* h, vers_filter_t* f, void* stream);
int32_t vers_ivf_filter_info(vers_ivf_t* h, const vers_filter_t* f, uint64_t* out8);
int32_t vers_ivf_filter_destroy(vers_ivf_t* h, vers_filter_t* f);
int32_t vers_ivf_search_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                     uint32_t nprobe /* nprobe_max if adaptive */, const vers_filter_t* f, const uint32_t* filter_of_dev,
                                     const vers_adaptive_t* adaptive, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_count_dev,
                                     void* stream);
int32_t vers_ivf_search_exhaustive_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, uint32_t top_k,
                                                uint32_t metric, const vers_filter_t* f, const uint32_t* filter_of_dev, uint64_t* out_ids_dev,
                                                float* out_dist_dev, uint32_t* out_count_dev, void* stream);
int32_t vers_ivf_range_search_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b, const float* radius_dev,
                                           uint32_t nprobe, uint32_t flags, const vers_filter_t* f, const uint32_t* filter_of_dev,
                                           uint64_t* out_lims_dev /* [b+1] */, uint64_t* out_ids_dev, float* out_dist_dev, uint64_t cap,
                                           uint64_t* out_total /* host */, void* stream);
int32_t vers_ivf_range_search_exhaustive_prepared_dev(vers_ivf_t* h, const float* queries_dev, uint64_t ldq_floats, uint32_t b,
                                                      const float* radius_dev, uint32_t metric, uint32_t flags, const vers_filter_t* f,
                                                      const uint32_t* filter_of_dev, uint64_t* out_lims_dev, uint64_t* out_ids_dev,
                                                      float* out_dist_dev, uint64_t cap, uint64_t* out_total /* host */, void* stream);

/* Measurement hook: durations (HIP events on the search's stream) of the two kernels of the most recent batched
 * coarse quantiser -- the queries x centroids contraction on the f32 matrix cores (2*b*k*d flop) and the selection /
 * exact re-score / certificate kernel behind it. */
int32_t vers_ivf_last_coarse_ms(vers_ivf_t* h, float* out_gemm_ms, float* out_select_ms);
/* Measurement hook: duration (HIP events on the search's stream) of the exact finish -- ivf_rescore_kernel: merge of the
 * partial candidate lists, certificate, exact re-score of the survivors, emit -- of the most recent matrix-core batch. */
int32_t vers_ivf_last_finish_ms(vers_ivf_t* h, float* out_ms);
/* Batched coarse quantiser statistics: batches that went through the MFMA pre-selection (f32 matrix cores +
 * exact re-score + certificate, csrc/gemm.hip.h) and queries whose certificate failed and were re-done exactly. */
int32_t vers_ivf_coarse_stats(vers_ivf_t* h, uint64_t* out_mfma_batches, uint64_t* out_fallback_queries);
/* Batched list scan statistics (nprobe mode): batches whose list scan ran on the matrix cores (pre-selection +
 * exact re-score + certificate, csrc/prescan.hip.h) and queries whose certificate failed and were re-scanned
 * exactly.  Results are bit-identical either way; option "prescan" = 0 keeps the ordered-chain scan for every batch. */
int32_t vers_ivf_prescan_stats(vers_ivf_t* h, uint64_t* out_batches, uint64_t* out_fallback_queries);
/* Early abandon of the batched list scan (option "pre_prune"): 64-column steps whose math ran | steps of abandoned tiles that ran no
 * math (one of them per abandoned tile was still read: it was in flight) | tiles abandoned -- [3] of the most recent matrix-core
 * scan (zeros when it ran with the switch off or on a path the switch does not cover) and [3] summed over the handle's life.  Either
 * pointer may be NULL.  HBM bytes not read = (steps - tiles) x 8 KiB.  A tile the int8 head's filter ruled out (option "pre_head") counts
 * as abandoned before its first step: all its steps without math, none of them in flight (vers_ivf_head_state has the filter's own
 * counters and what it read instead). */
int32_t vers_ivf_prune_stats(vers_ivf_t* h, uint64_t* out_last, uint64_t* out_total);
/* The int8 head of the stored rows (option "pre_head"): whether the handle holds a VALID one (built by build / upload / compact;
 * invalidated by add, add_batch, remove_batch), its bytes and its columns per row, and the filter's counters -- quads tested | quads
 * ruled out | 64-column head steps (4 KiB each) read -- [3] of the most recent list scan (zeros when that scan was a single launch)
 * and [3] over the handle's life.  Any pointer may be NULL. */
int32_t vers_ivf_head_state(vers_ivf_t* h, int32_t* out_valid, uint64_t* out_bytes, uint32_t* out_cols, uint64_t* out_last, uint64_t* out_total);
/* The sub-cluster balls of the lists (option "pre_ball"): whether the handle holds VALID ones (derived and invalidated where the int8
 * head is), their bytes, the lists that got balls and the sub-clusters over all lists, and the ball filter's counters -- units (list,
 * query group) tested | units ruled out -- [2] of the most recent list scan (zeros when the pass was not launched or did not engage)
 * and [2] over the handle's life.  The quads of a unit ruled out count in vers_ivf_head_state's quads tested | ruled out as well.
 * Any pointer may be NULL. */
int32_t vers_ivf_ball_state(vers_ivf_t* h, int32_t* out_valid, uint64_t* out_bytes, uint32_t* out_lists_with_balls, uint64_t* out_subclusters,
                            uint64_t* out_last, uint64_t* out_total);
/* An fp16 shadow copy of the stored rows (+50 % corpus memory) feeds the matrix-core pre-selection of batched searches:
 * half the HBM bytes per list scan, a ~2x wider certificate window, the same exact f32 finish -- results stay
 * bit-identical.  On by default (VERS_SHADOW=0 or vers_set_option("shadow", 0) before build / upload: f32 rows feed the
 * scan); skipped when its allocation fails; switched off for the handle when more than 1/8 of the queries failed the
 * certificate (data with many near-ties, or elements outside fp16's range).  out_active: 1 = in use. */
int32_t vers_ivf_shadow_state(vers_ivf_t* h, int32_t* out_active, uint64_t* out_bytes);
/* Durations (ms) of the most recent list-scan launches, oldest first (ring of 64); reset != 0
 * empties the ring.  Lets bench.py time every launch of the timed region without stalling it. */
int32_t vers_ivf_scan_times(vers_ivf_t* h, float* out_ms, uint32_t cap, uint32_t* out_n, int32_t reset);
/* Reads inverted list `cluster` back to the host in list order: rows (pitch row_stride_bytes) and
 * vec ids; out_rows / out_ids may be NULL to query the length only.  (ids[c] and values of the
 * reference, for host-side serde and for the CPU baseline of bench.py.) */
int32_t vers_ivf_get_list(vers_ivf_t* h, uint64_t cluster, float* out_rows, uint64_t row_stride_bytes,
                          uint64_t* out_ids, uint64_t cap_rows, uint64_t* out_len);
int32_t vers_ivf_get_centroids(vers_ivf_t* h, float* out_centroids, uint64_t c_stride_bytes);

/* ------------------------------------------------------------------------ *
 * Measurement tooling (bench.py): deterministic synthetic vectors written   *
 * straight into HBM; bit-identical to tests/datagen.py on the host.          *
 * kind 0 = uniform on the sphere, kind 1 = clustered (n_modes centres drawn  *
 * as kind 0 from seed_centres, row = normalize(centre[row % n_modes] +       *
 * sigma * noise)).  Rows start_row .. start_row+n-1 of the stream `seed`.    *
 * ------------------------------------------------------------------------ */
int32_t vers_gen_rows_dev(float* out_dev, uint64_t n, uint32_t d, uint64_t ld_floats, uint32_t kind,
                          uint64_t seed, uint64_t seed_centres, uint32_t n_modes, float sigma,
                          uint64_t start_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VERS_HIP_H */
