/*
 * sqgr.h — C ABI of libsqgr.so, the MI355X (gfx950) implementation of Squidpy's `sq.gr`
 * spatial-statistics hot path.
 *
 * The reference (scverse/squidpy) has no FFI on this path: its kernels are numba-JIT Python
 * (SURVEY.md §8b).  Each entry point below therefore replaces a *Python-level* reference
 * function, cited as file:line under /root/reference/src/squidpy; INTEGRATION.md shows the
 * ctypes binding a Squidpy maintainer would add at those call sites.
 *
 * Conventions
 *   - plain C, every function returns 0 (SQGR_OK) or a negative sqgr_status; never throws.
 *     `sqgr_last_error()` returns a thread-local human-readable message for the last failure.
 *   - all array arguments are caller-owned HOST pointers (C-contiguous), copied in/out by the
 *     library and never retained after return, except inside explicit handles
 *     (sqgr_graph, sqgr_nhood, sqgr_points, sqgr_autocorr), which keep DEVICE copies.
 *   - a context owns one device and one HIP stream; a context is not thread-safe, distinct
 *     contexts may be used from distinct threads (one process per GPU is the intended use).
 *   - calls are synchronous on return unless documented otherwise.
 *   - there is NO CPU fallback anywhere in this library: without a usable HIP device
 *     `sqgr_ctx_create` fails.
 */
#ifndef SQGR_H
#define SQGR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQGR_ABI_VERSION 7

typedef enum sqgr_status {
    SQGR_OK = 0,
    SQGR_ERR_INVALID = -1,     /* bad argument (null pointer, out-of-range label, K <= 1, ...) */
    SQGR_ERR_HIP = -2,         /* a HIP runtime call failed; message has the hipError string   */
    SQGR_ERR_NOMEM = -3,       /* device or host allocation failed                               */
    SQGR_ERR_UNSUPPORTED = -4, /* valid request outside what the kernels implement               */
    SQGR_ERR_NODEVICE = -5     /* no HIP device / device index out of range                      */
} sqgr_status;

typedef struct sqgr_ctx sqgr_ctx;
typedef struct sqgr_graph sqgr_graph;
typedef struct sqgr_nhood sqgr_nhood;
typedef struct sqgr_points sqgr_points;
typedef struct sqgr_autocorr sqgr_autocorr;

/* ------------------------------------------------------------------ library / context */
int sqgr_abi_version(void);
const char* sqgr_last_error(void);
int sqgr_device_count(int* out_count);
int sqgr_ctx_create(int device, sqgr_ctx** out_ctx);
int sqgr_ctx_destroy(sqgr_ctx* ctx);
int sqgr_ctx_sync(sqgr_ctx* ctx);
/* Device buffers of 64 MB and more are parked per device when their owner lets go of them and reused by the next request of
 * about that size (bounded by SQGR_POOL_GB, default a quarter of the device memory — the oldest parked buffers go first; other HIP users of the process see parked memory as taken).
 * sqgr_ctx_trim synchronises the device and returns parked buffers of ctx's device to the driver until at most keep_bytes
 * stay parked (0: everything). */
int sqgr_ctx_trim(sqgr_ctx* ctx, int64_t keep_bytes);
/* What the library asked of the HIP allocator since it was loaded (process-wide, all devices): out[0..count) <-
 * {hipMalloc calls, bytes of the successful ones, ns spent inside hipMalloc, hipFree calls, ns spent inside hipFree, requests
 * served by a parked buffer, buffers parked, pool flushes}; slots past 8 read 0.  bench.py prints the differences over its timed
 * regions next to the kernel times, and `a second call allocates nothing` is a test (tests/test_autocorr_gpu.py). */
int sqgr_debug_counters(int64_t* out, int32_t count);
/* name[0..len) <- device name, *cu_count <- compute units, *hbm_bytes <- total device memory */
int sqgr_ctx_device_info(sqgr_ctx* ctx, char* name, int len, int* cu_count, int64_t* hbm_bytes);

/* Per-kernel HIP-event timing on the context's own stream (used by bench.py for the roofline
 * figure).  While enabled every kernel launch is bracketed by hipEventRecord on ctx's stream.
 * sqgr_timer_get sums elapsed ms and launches of all kernels whose name starts with `prefix`. */
int sqgr_timer_enable(sqgr_ctx* ctx, int enable);
int sqgr_timer_reset(sqgr_ctx* ctx);
int sqgr_timer_get(sqgr_ctx* ctx, const char* prefix, double* total_ms, int64_t* launches);
/* writes a ';'-separated list "name:launches:ms" of everything timed so far */
int sqgr_timer_report(sqgr_ctx* ctx, char* buf, int len);

/* ------------------------------------------------------------------ multi-GPU: RCCL communicator
 * One process per GPU.  The path shards by permutation range / row tiles / feature blocks and has ONE exchange: an
 * all-reduce(sum) of exact 64-bit integer accumulators (`Σcount`, `Σcount²`: replaces the reduction the reference's
 * joblib fan-out does by concatenating per-job chunks, gr/_nhood.py:215-231, _utils.py:223-231).  The library binds
 * RCCL itself (librccl.so.1, at the first sqgr_comm_* call); the caller only moves rank 0's unique id to the other
 * ranks (any side channel) — no torch.distributed in the data path.
 *   sqgr_comm_unique_id : rank 0 fills out_id[SQGR_UNIQUE_ID_BYTES] (ncclGetUniqueId)
 *   sqgr_comm_create    : collective over all `world` ranks (ncclCommInitRank) on ctx's device
 *   sqgr_comm_allreduce_i64 : in-place all-reduce of a HOST buffer int64[count] (staged through the device; uint64
 *                             data may be passed through its int64 view for SQGR_OP_SUM: addition modulo 2^64)
 *   sqgr_nhood_set_comm : attaches the communicator to a plan — sqgr_nhood_run then all-reduces the moments ON THE
 *                         DEVICE before its one 2*K*K*8-byte copy-out (every rank returns the global sums), and
 *                         sqgr_nhood_run_pcg64_stats all-gathers the per-permutation counts of the ranks' ranges. */
#define SQGR_UNIQUE_ID_BYTES 128
#define SQGR_OP_SUM 0
#define SQGR_OP_MAX 1
typedef struct sqgr_comm sqgr_comm;
int sqgr_comm_unique_id(uint8_t* out_id);
int sqgr_comm_create(sqgr_ctx* ctx, const uint8_t* unique_id, int32_t rank, int32_t world, sqgr_comm** out_comm);
int sqgr_comm_destroy(sqgr_comm* comm);
int sqgr_comm_info(const sqgr_comm* comm, int32_t* rank, int32_t* world);
int sqgr_comm_allreduce_i64(sqgr_comm* comm, int64_t* buf, int64_t count, int32_t op);
int sqgr_comm_barrier(sqgr_comm* comm);

/* ------------------------------------------------------------------ spatial graph (CSR)
 * Device-resident copy of `adata.obsp[<key>_connectivities]` (scipy CSR): what
 * gr/_nhood.py:194,205 and gr/_ppatterns.py:212 read.  `data` may be NULL (binarised use).
 * indptr: int64[n+1]; indices: int32[nnz]; data: float32[nnz] (sqgr_graph_create) or float64[nnz] (…_f64). */
int sqgr_graph_create(sqgr_ctx* ctx, int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                      const float* data, sqgr_graph** out_graph);
/* The same with float64 weights (a float64 `obsp` matrix, or one row-normalised in float64 as gr/_ppatterns.py:212-214
 * does): the device keeps and uses float64 weights in either case — float32 input is widened exactly. */
int sqgr_graph_create_f64(sqgr_ctx* ctx, int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                          const double* data, sqgr_graph** out_graph);
int sqgr_graph_destroy(sqgr_graph* g);
/* Observations in no spatial order cost the permutation test's count kernel up to 8x: it gathers the label rows of an edge's two
 * endpoints (no counterpart in the reference, whose loop does not care).  `sqgr_graph_renumbered` builds the twin P A P^T of a graph
 * (structure only, canonical CSR) on the device for `order[new] = old`; `sqgr_spatial_order` computes such an order from coordinates
 * xy float64[n][2] (Z-order curve).  A plan created on the twin with the labels in twin order and `sqgr_nhood_set_spot_map(plan,
 * order)` returns exactly the moments of the plan on the caller's own graph (sqgr_nhood_run; ABI v7). */
int sqgr_graph_renumbered(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* order, sqgr_graph** out_graph);
int sqgr_spatial_order(sqgr_ctx* ctx, const double* xy, int64_t n, int32_t* out_order);
/* The segment list of a structurally symmetric graph without self loops (lattices in scan order: the count kernel of the permutation
 * test walks 16 consecutive rows with one column offset as one entry; SQGR_COUNT_SEGMENTS, ABI v7), built on first use; for tests.
 *   out_info: int64[5] = {1 built | 0 not applicable (sqgr_last_error names the reason; the call still returns SQGR_OK), entries,
 *             entries with the zero-mask padding, residual half edges, half edges}
 *   out_seg:  int32[padded entries][3] = (r0, d, mask) or NULL — bit j of mask <=> half edge (r0 + j, r0 + j + d); ordered by (r0, d)
 *   out_res:  int32[residual][2] = (r, c) or NULL — the half edges of the entries with fewer than 8 edges. */
int sqgr_graph_segments(const sqgr_graph* g, int64_t* out_info, int32_t* out_seg, int32_t* out_res);

/* ------------------------------------------------------------------ nhood_enrichment
 * replaces the generated numba kernel `_nenrich_{K}_{parallel}` (gr/_nhood.py:54-141):
 *   out[a*K+b] = sum_{i: lab_i=a} #{j in N(i): lab_j=b}      (uint32, edges binarised)
 * labels: int32[n] in [0,K).  2 <= K <= 256. */
int sqgr_nhood_counts(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, uint32_t* out_counts);

/* Injected permutations: the body of `_nhood_enrichment_helper` (gr/_nhood.py:530-539) with the
 * shuffled label vectors supplied by the caller (e.g. numpy's PCG64 shuffles, for exact parity):
 *   labels: uint8[n_perms][n];  out_counts: uint32[n_perms][K][K]. */
int sqgr_nhood_counts_batch(sqgr_ctx* ctx, const sqgr_graph* g, const uint8_t* labels, int64_t n_perms, int32_t K,
                            uint32_t* out_counts);

/* A resident permutation-test problem: graph + base labels (+ optional libraries) on the device.
 * lib_ids: int32[n] in [0,n_libs) or NULL (gr/_utils.py:185-213 `_shuffle_group` semantics:
 * labels are shuffled independently inside each library). */
int sqgr_nhood_create(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, const int32_t* lib_ids,
                      int32_t n_libs, sqgr_nhood** out_plan);
int sqgr_nhood_destroy(sqgr_nhood* plan);

/* Runs permutations [perm_begin, perm_end) of the test entirely on the device: replaces
 * `parallelize(_nhood_enrichment_helper, ...)` (gr/_nhood.py:215-230).  Label shuffles are generated
 * on the GPU by a counter-based generator keyed by (seed, global permutation index, library):
 * Philox4x32-10 round keys + 8-round Feistel bijection with cycle walking (csrc/sqgr_rng.h,
 * restated in oracle/devrng.py), so results do not depend on how a permutation range is split
 * across calls, devices or ranks.
 *   shift:      int64[K*K] or NULL(=0): d = count - shift is what gets accumulated (exact integers)
 *   out_sum:    int64[K*K]   sum_p d           out_sumsq: uint64[K*K]  sum_p d*d
 *   out_perms:  uint32[(perm_end-perm_begin)*K*K] or NULL — the per-permutation counts. */
int sqgr_nhood_run(sqgr_nhood* plan, uint64_t seed, int64_t perm_begin, int64_t perm_end, const int64_t* shift,
                   int64_t* out_sum, uint64_t* out_sumsq, uint32_t* out_perms);

/* The same test with numpy's OWN random streams reproduced bit for bit on the device: permutation p is
 * shuffled by numpy's algorithm (PCG64 + Generator.shuffle's reverse Fisher-Yates with masked rejection; with libraries the
 * per-library sub-shuffles of `_shuffle_group`, gr/_utils.py:185-213) starting from generator state
 *   pcg_states[4*p .. 4*p+3] = {state_hi, state_lo, inc_hi, inc_lo}
 * = `np.random.PCG64(SeedSequence(seed).spawn(n_perms)[p]).state["state"]`, i.e. the state of `generators[p]` of
 * `spawn_generators` (_utils.py:240-241).  Outputs as sqgr_nhood_run; with out_perms the caller can apply the reference's
 * float64 `perms.mean/std` (gr/_nhood.py:231) and obtain Squidpy's z-scores for that seed exactly. */
int sqgr_nhood_run_pcg64(sqgr_nhood* plan, const uint64_t* pcg_states, int64_t n_perms, const int64_t* shift, int64_t* out_sum,
                         uint64_t* out_sumsq, uint32_t* out_perms);
/* The numpy-stream test reduced the way the reference reduces it (gr/_nhood.py:231): out_mean / out_std float64[K*K] are
 * `perms.mean(axis=0)` and `perms.std(axis=0)` of the (n_perms, K, K) float64 count array, bit for bit (sequential
 * float64 accumulation in permutation order, as numpy does over a leading axis), so that
 * `(count - mean) / std` is Squidpy's z-score for the seed — without moving the n_perms*K*K counts to the host. */
int sqgr_nhood_run_pcg64_stats(sqgr_nhood* plan, const uint64_t* pcg_states, int64_t n_perms, double* out_mean, double* out_std);

/* Launch geometry of a plan, int64[12]: {width of the label slab's rows (16|32 permutations), batches per launch group,
 * edge chunks (count blocks) per batch, edges of the list the count kernel walks (the half list r < c + self loops on a structurally
 * symmetric graph, else nnz), 0 full list | 1 half list | 2 half list with self loops, accumulator slots per batch (K*K x row
 * width), self loops, permutations per group of the label generator, permutations per PASS over the edge list (16 | 8 | 4 | 2 | 1;
 * 32 for 32-wide rows; 0: device-scope counters), row halves per pass (2: 203 <= K <= 256 with 32-bit counters), counter mode
 * (0: 32-bit counters on K*K pairs; 1: 16-bit on K*K pairs; 2: 16-bit on the K (K + 1) / 2 unordered pairs of a symmetric
 * graph), bytes of one chunk's partial histograms}.  bench.py derives its per-kernel ceilings from these. */
int sqgr_nhood_info(sqgr_nhood* plan, int64_t* out_info);

/* Attaches (comm != NULL) or detaches an RCCL communicator: see "multi-GPU" above. */
int sqgr_nhood_set_comm(sqgr_nhood* plan, sqgr_comm* comm);
/* The plan lives on a renumbered twin of the caller's graph (sqgr_graph_renumbered): spot_of int32[n], slab row i belongs to the
 * caller's observation spot_of[i] — the device generator permutes THAT observation's rank, so sqgr_nhood_run returns the moments of
 * the plan on the caller's own graph, bit for bit.  No libraries, at most 256 clusters; the numpy-stream and injected-label entry
 * points refuse such a plan (they permute positions).  NULL removes the map. */
int sqgr_nhood_set_spot_map(sqgr_nhood* plan, const int32_t* spot_of);

/* numpy's `Generator.permutation(n)` for n_perms generator states (layout as above), on the device:
 * out_idx int32[n_perms][n] — the row permutations of `_score_helper` (gr/_ppatterns.py:269-271). */
int sqgr_pcg64_permutations(sqgr_ctx* ctx, int64_t n, const uint64_t* pcg_states, int64_t n_perms, int32_t* out_idx);

/* Debug/parity hook: the shuffled label vector of one global permutation index, uint8[n]. */
int sqgr_nhood_shuffled_labels(sqgr_nhood* plan, uint64_t seed, int64_t perm, uint8_t* out_labels);

/* tuning knobs (0 = library default): perms per CSR pass (16|32 = width of the label slab; 8|4|2|1 = cap of the LDS pass width
 * of a 16-wide slab — what 51 <= K <= 202 clusters select by themselves), count blocks (edge chunks) per batch, batches per launch */
int sqgr_nhood_tune(sqgr_nhood* plan, int32_t perms_per_pass, int32_t blocks_per_batch, int32_t batches_per_launch);

/* weighted K x K edge sums: `_interaction_matrix` (gr/_nhood.py:412-429); out: float64[K*K].
 * weights != 0 uses graph data (must have been uploaded), else 1 per stored edge. */
int sqgr_interaction_matrix(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int32_t weights,
                            double* out);

/* ------------------------------------------------------------------ co_occurrence
 * replaces the numba kernel `_occur_count` (gr/_ppatterns.py:283-310):
 *   out[(a*K+b)*L + r] = #{ i != j : lab_i=a, lab_j=b, d2_ij <= thr2[r] },  d2 = dx*dx + dy*dy in float32
 * x, y: float32[n]; labels: int32[n] in [0,K); thr2: float32[L] squared thresholds (any order).
 * fma = 0: products and sum rounded separately (numpy / literal-source semantics, the oracle of record);
 * fma = 1: d2 = fma(dx,dx,dy*dy) (what LLVM may emit for numba's fastmath=True on an FMA host).
 * Only row tiles t with t % shard_count == shard_index are swept (each unordered tile pair once, credited to
 * both (a,b) and (b,a)); summing the outputs of all shards gives the full counts (multi-GPU: all-reduce). */
int sqgr_cooccur_counts(sqgr_ctx* ctx, const float* x, const float* y, const int32_t* labels, int64_t n, int32_t K,
                        const float* thr2, int32_t L, int32_t fma, int32_t shard_index, int32_t shard_count,
                        int64_t* out_counts);

/* ------------------------------------------------------------------ spatial_autocorr (Moran's I / Geary's C)
 * A resident block of features on one graph: vals float64[G][n] (gene-major, the reference's `vals`,
 * gr/_ppatterns.py:154-185).  The graph must carry its weights (row-normalised by the caller when
 * `transformation=True`, gr/_ppatterns.py:212-214).  mode: 0 = Moran's I, 1 = Geary's C. */
int sqgr_autocorr_create(sqgr_ctx* ctx, const sqgr_graph* g, const double* vals, int64_t G, sqgr_autocorr** out);
/* Same block handed over cell-major: vals float64[n][G] — the layout of `adata.X[:, genes]` before the reference
 * transposes it (gr/_ppatterns.py:168) — so the host never has to materialise the transpose (a strided 8-byte gather,
 * ~0.1 GB/s in numpy: 13 s for 1e5 cells x 2048 genes).  Results are bit-identical to sqgr_autocorr_create. */
int sqgr_autocorr_create_cm(sqgr_ctx* ctx, const sqgr_graph* g, const double* vals, int64_t G, sqgr_autocorr** out);
/* The whole expression matrix resident on the device: x float64[n_rows][n_cols] row-major (`adata.X` as it lies in
 * memory), uploaded once; feature blocks are then columns [col0, col0 + G) of it — no host-side slicing or transposing
 * per block at all (gr/_ppatterns.py:154-185 builds `vals = adata[:, genes].X.T` on the host). */
typedef struct sqgr_matrix sqgr_matrix;
int sqgr_matrix_create(sqgr_ctx* ctx, const double* x, int64_t n_rows, int64_t n_cols, sqgr_matrix** out);
/* The same for float32 (AnnData's usual dtype; widened to float64 on the device, exactly) and / or a column range of a
 * wider host matrix: x points at the first wanted element, rows are `ld` elements apart (ld >= n_cols); value_bytes 4 | 8. */
int sqgr_matrix_create_dense(sqgr_ctx* ctx, const void* x, int32_t value_bytes, int64_t n_rows, int64_t n_cols, int64_t ld,
                             sqgr_matrix** out);
/* The same matrix filled while its first feature blocks are being worked on (ABI v6): `sqgr_matrix_alloc_dense` reserves the
 * device array; `sqgr_matrix_upload_columns(m, x, ld, col0, n_cols)` copies columns [col0, col0 + n_cols) — x points at the first
 * row's element of column col0 of the host matrix, rows `ld` elements apart — on the context's COPY stream and waits for that
 * stream only, so it may run on another host thread than the statistics (config 3: 16 GB cross PCIe in 0.29 s, hidden behind the
 * 0.58 s of the ten feature blocks).  A column range must be uploaded before sqgr_autocorr_create_cols reads it: the caller's
 * business (squidpy_amd: DeviceMatrix.wait_columns). */
int sqgr_matrix_alloc_dense(sqgr_ctx* ctx, int32_t value_bytes, int64_t n_rows, int64_t n_cols, sqgr_matrix** out);
int sqgr_matrix_upload_columns(sqgr_matrix* m, const void* x, int64_t ld, int64_t col0, int64_t n_cols);
/* Sparse expression as scipy holds it — the input every real Visium / Xenium object has (`adata.X` CSR float32; the
 * reference densifies `vals` feature block by feature block on the host, gr/_ppatterns.py:154-185 + scanpy's metrics):
 * CSR (rows = cells: indptr[n_rows + 1], indices = columns) or CSC (columns = features: indptr[n_cols + 1], indices = rows),
 * index arrays int32 or int64 (index_bytes 4 | 8, both arrays alike as in scipy), values float32 or float64
 * (value_bytes 4 | 8), in scipy's canonical format: indices ascending inside every row / column, no repeated entries
 * (checked on the device; SQGR_ERR_INVALID names which — `sort_indices()` / `sum_duplicates()` fix it).  Feature blocks are expanded to dense float64 ON THE DEVICE by sqgr_autocorr_create_cols: the
 * results are bit-identical to uploading `toarray().astype(float64)`. */
int sqgr_matrix_create_csr(sqgr_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, const void* indices,
                           int32_t index_bytes, const void* values, int32_t value_bytes, sqgr_matrix** out);
int sqgr_matrix_create_csc(sqgr_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, const void* indices,
                           int32_t index_bytes, const void* values, int32_t value_bytes, sqgr_matrix** out);
int sqgr_matrix_destroy(sqgr_matrix* m);
int sqgr_autocorr_create_cols(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_matrix* m, int64_t col0, int64_t G, sqgr_autocorr** out);
/* Features = the columns cols[0 .. G) of the resident matrix, in that order (any subset, any order): the reference's default —
 * the highly variable genes — and explicit `genes` lists select columns with `adata[:, genes].X` on the host
 * (gr/_ppatterns.py:156-166), an O(nnz) copy that costs more than the whole statistic at 1e5 cells; here the matrix is uploaded
 * once as it is and the selection happens on the device (a CSR matrix gets a by-column twin there the first time). */
int sqgr_autocorr_create_colidx(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_matrix* m, const int32_t* cols, int64_t G,
                                sqgr_autocorr** out);
int sqgr_autocorr_destroy(sqgr_autocorr* h);
/* observed statistic: replaces `score = func(g, vals)` (gr/_ppatterns.py:216; scanpy.metrics.morans_i/gearys_c);
 * constant features -> NaN.  out_scores: float64[G]. */
int sqgr_autocorr_scores(sqgr_autocorr* h, int32_t mode, double* out_scores);
/* permutation scores: replaces `parallelize(_score_helper, ...)` (gr/_ppatterns.py:225-232, 258-280):
 *   out_sims[p][g] = func(g[idx_p, :], vals)[g]        (rows of the graph permuted, values fixed)
 * perm_idx: int32[P][n] caller-supplied permutations (e.g. numpy's `rng.permutation(n)` streams) or NULL to
 * generate permutations [perm_begin, perm_end) on the device (csrc/sqgr_rng.h, keyed by seed and the global
 * permutation index => the PERMUTATIONS are independent of how the range is split).  out_sims: float64[P][G],
 * P = perm_end-perm_begin.  The scores' last bits also depend on which of the three summation kernels runs, and that is
 * chosen from the length of THIS call's range (fewer than 40 permutations, 40-511, 512 and more — for >= 256 features and
 * >= 4096 spots; the gather kernel otherwise): a caller that cuts one test into several calls and wants bit-identical scores
 * keeps every piece on one side of these thresholds (or sets SQGR_AUTOCORR_KERNEL).  The front end never cuts permutation
 * ranges — ranks own feature blocks — so its frames do not depend on the number of ranks. */
int sqgr_autocorr_perms(sqgr_autocorr* h, int32_t mode, const int32_t* perm_idx, uint64_t seed, int64_t perm_begin,
                        int64_t perm_end, double* out_sims);
/* sqgr_autocorr_perms with the reference's own numpy streams generated ON THE DEVICE: pcg_states holds n_perms rows
 * [state_hi, state_lo, inc_hi, inc_lo] of `spawn_generators(seed, n_perms)` (_utils.py:240-241); permutation p of the
 * rows is bit for bit `generators[p].permutation(n)` (gr/_ppatterns.py:270-271).  Nothing but 32 bytes per permutation
 * crosses PCIe (injecting the same permutations through sqgr_autocorr_perms costs 4*n bytes each, per feature block). */
int sqgr_autocorr_perms_pcg64(sqgr_autocorr* h, int32_t mode, const uint64_t* pcg_states, int64_t n_perms, double* out_sims);

/* The permutation test REDUCED on the device: runs the permutations exactly like sqgr_autocorr_perms (perm_idx != NULL:
 * injected; pcg_states != NULL: numpy streams as sqgr_autocorr_perms_pcg64, one row per permutation of the range; both
 * NULL: the device generator for [perm_begin, perm_end)) but keeps the (P, G) scores on the device and returns, per
 * feature, what `_p_value_calc` (gr/_ppatterns.py:474-492) takes out of them — so G x 4 numbers cross PCIe instead of
 * P x G (160 MB at 20 000 features x 1000 permutations):
 *   out_ge[g]  = #{p : sims[p][g] >= score[g]}       `(sims >= score).sum(axis=0)`            int64[G]
 *   out_sum[g] = `sims.sum(axis=0)[g]`    out_std[g] = `sims.std(axis=0)[g]`    out_var[g] = `np.var(sims, axis=0)[g]`
 * each in numpy's own evaluation order (sequential over the permutation axis, mean = sum / P, then the squared
 * deviations summed the same way): bit-identical to numpy on the same scores.  score: float64[G], the observed statistic.
 * only_feature != 0 (G must be 1): this block is the ONLY feature of the call — the reference's (P, 1) array is contiguous
 * along the permutation axis as well and numpy reduces it in its other order (pairwise sums of 8192-element runs); set it
 * when the call scores a single feature, never for a one-feature block of a larger call. */
int sqgr_autocorr_perm_stats(sqgr_autocorr* h, int32_t mode, const int32_t* perm_idx, const uint64_t* pcg_states, uint64_t seed,
                             int64_t perm_begin, int64_t perm_end, const double* score, int64_t* out_ge, double* out_sum,
                             double* out_std, double* out_var, int32_t only_feature);

/* parity hook: the device generator's permutations, int32[perm_end-perm_begin][n] (<= 32768 per call) */
int sqgr_autocorr_perm_indices(sqgr_ctx* ctx, int64_t n, uint64_t seed, int64_t perm_begin, int64_t perm_end,
                               int32_t* out_idx);

/* ------------------------------------------------------------------ ripley (K/L pair counts, F/G kNN distances)
 * metric: 0 euclidean, 1 manhattan, 2 chebyshev (sklearn KDTree arithmetic: per-coordinate accumulation, no FMA); the
 * nearest-neighbour entry points also take 3 canberra (sklearn's BallTree metric without parameters; brute-force sweep,
 * no cell list) — sqgr_pair_counts does not: KDTree.valid_metrics ends at chebyshev (gr/_ripley.py:213).
 *
 * sqgr_pair_counts replaces `KDTree(points).two_point_correlation(points, support, dualtree=True) - m`
 * (gr/_ripley.py:220-222): out[s] = #{ordered i != j : dist_ij <= r_s}.  xy: float64[m][2]; thr: float64[S]
 * ascending.  For metric 0 the comparison is done on the squared distance: pass thr[s] = the largest float64 t with
 * fl(sqrt(t)) <= r_s (so that `d2 <= t` == `sqrt(d2) <= r_s` bit for bit); for metrics 1/2 pass the radii. */
int sqgr_pair_counts(sqgr_ctx* ctx, const double* xy, int64_t m, const double* thr, int32_t S, int32_t metric,
                     int64_t* out_counts);
/* The same for n_sets point sets in ONE launch (Ripley's L evaluates one set per cluster and one per simulation,
 * gr/_ripley.py:152,171): set z = points xy[offsets[z] .. offsets[z+1]), out_counts int64[n_sets][S].  n_sets <= 65535. */
int sqgr_pair_counts_batch(sqgr_ctx* ctx, const double* xy, const int64_t* offsets, int32_t n_sets, const double* thr, int32_t S,
                           int32_t metric, int64_t* out_counts);
/* sqgr_knn_dist replaces `NearestNeighbors(n_neighbors=k).fit(ref).kneighbors(query)[0]` (gr/_ripley.py:144-150,
 * 163-169): out float64[nq][k] ascending; for metric 0 the SQUARED distances (caller applies sqrt). 1 <= k <= 16. */
int sqgr_knn_dist(sqgr_ctx* ctx, const double* query, int64_t nq, const double* ref, int64_t nr, int32_t k, int32_t metric,
                  double* out);
/* Ripley's G keeps its (large) query set on the device: sqgr_points holds coordinates (+ an int32 label per point);
 * sqgr_knn_hist finds, for every query point whose label differs from `exclude_label` (-1: all points), the k nearest of
 * the `ref` points and returns `np.histogram(distances, bins=edges)[0]` (int64[S-1]) of all those distances — what
 * gr/_ripley.py:163-169 + `_f_g_function` :206-209 compute with sklearn and numpy, without moving the distances. */
typedef struct sqgr_points sqgr_points;
int sqgr_points_create(sqgr_ctx* ctx, const double* xy, const int32_t* labels, int64_t n, sqgr_points** out);
int sqgr_points_destroy(sqgr_points* p);
int sqgr_knn_hist(sqgr_ctx* ctx, const sqgr_points* queries, int32_t exclude_label, const double* ref, int64_t nr, int32_t k,
                  int32_t metric, const double* edges, int32_t S, int64_t* out_counts);

/* ------------------------------------------------------------------ spatial graph construction
 * Exact 2-D neighbour search on a device cell list; xy: float64[n][2].
 *
 * sqgr_knn_self replaces `NearestNeighbors(n_neighbors=k, metric="euclidean").fit(xy).kneighbors()`
 * (gr/neighbors.py:196-199, 402-405): for every sample its k nearest OTHER samples (self excluded by index),
 * ascending; ties broken by the smaller index.  out_idx int32[n][k]; out_d2 float64[n][k] SQUARED distances
 * (per-coordinate accumulation, no FMA; the caller applies sqrt).  1 <= k <= min(64, n-1). */
int sqgr_knn_self(sqgr_ctx* ctx, const double* xy, int64_t n, int32_t k, int32_t* out_idx, double* out_d2);
/* sqgr_radius_self replaces `NearestNeighbors(radius=r).fit(xy).radius_neighbors()` (gr/neighbors.py:252-255): all
 * other samples with squared distance <= r*r, as CSR.  Call once with out_idx = out_d2 = NULL to obtain
 * out_indptr int64[n+1], allocate out_indptr[n] entries, call again (capacity = allocated entries). */
int sqgr_radius_self(sqgr_ctx* ctx, const double* xy, int64_t n, double radius, int64_t* out_indptr, int32_t* out_idx,
                     double* out_d2, int64_t capacity);
/* The same two searches on 3-D coordinates, xyz: float64[n][3] row-major (stacked sections, volumetric data): squared
 * distances (dx*dx + dy*dy) + dz*dz, unfused, in coordinate order — sklearn's for coordinates of width 3.  Contracts,
 * error codes and messages are those of sqgr_knn_self / sqgr_radius_self; a point set that is flat in one or two axes,
 * or all at one site, is valid input. */
int sqgr_knn_self3(sqgr_ctx* ctx, const double* xyz, int64_t n, int32_t k, int32_t* out_idx, double* out_d2);
int sqgr_radius_self3(sqgr_ctx* ctx, const double* xyz, int64_t n, double radius, int64_t* out_indptr, int32_t* out_idx,
                      double* out_d2, int64_t capacity);

/* ---- ligand-receptor permutation test -------------------------------------------------------------------------------
 * sqgr_ligrec_counts replaces the numba kernel `_score_permutations` (gr/_ligrec.py:616-673) that `_analysis`
 * (gr/_ligrec.py:677-775) calls once for all permutations:
 *     for every permutation p in [perm_begin, perm_end):
 *         perm        = shuffle(clustering)
 *         groups[k,g] = (sum over cells with perm[cell] == k of data[cell,g], cells in index order) * inv_counts[k]
 *         out_counts[i,j] += valid[i,j] && groups[a_j,rec_i] + groups[b_j,lig_i] > obs[i,j]
 * with (rec_i, lig_i) = interactions[i], (a_j, b_j) = cpairs[j] and obs[i,j] = mean_obs[a_j,rec_i] + mean_obs[b_j,lig_i]
 * (formed by the caller in float64, the same IEEE addition the reference performs per comparison).
 *   data: the (n_cells x n_genes) float64 matrix as CSC columns of its stored entries (colptr int64[n_genes+1],
 *         rowidx int32 ascending inside a column, values) — zeros need not be stored, they do not change a sum.
 *   clustering int32[n_cells] in [0,K), 2 <= K <= 65535 (more than 256 clusters run in cluster tiles of 255 on 16-bit labels); inv_counts float64[K].
 *   pcg_states == NULL: device generator keyed by (seed, global permutation index) — the result for a permutation
 *         range does not depend on how ranges are split over calls or GPUs.
 *   pcg_states != NULL: numpy streams; (perm_end-perm_begin) rows [state_hi,state_lo,inc_hi,inc_lo] of the PCG64
 *         generators `spawn_generators(seed, n_perms)[perm_begin:perm_end]` (_utils.py:240-241); permutation p is then
 *         bit-for-bit `generators[p].shuffle(clustering.copy())`; `seed` is ignored.
 *   out_counts int64[n_inter*n_cp] (row-major, overwritten).  out_means_perm0 (may be NULL): float64[K*n_genes], the
 *         `groups` matrix of the first permutation of the range (for parity checks).
 * Group sums are accumulated in the reference's order (cell index), so they are bit-identical to the CPU loop. */
int sqgr_ligrec_counts(sqgr_ctx* ctx, int64_t n_cells, int32_t n_genes, int32_t K, const int64_t* colptr, const int32_t* rowidx,
                       const double* values, const int32_t* clustering, const double* inv_counts, const int32_t* interactions,
                       int64_t n_inter, const int32_t* cpairs, int32_t n_cp, const double* obs, const uint8_t* valid,
                       uint64_t seed, const uint64_t* pcg_states, int64_t perm_begin, int64_t perm_end, int64_t* out_counts,
                       double* out_means_perm0);

/* ---- sepal: diffusion-time scores of spatially variable genes --------------------------------------------------------
 * Replaces `_diffusion_genes` / `_diffusion` (gr/_sepal.py:165-251); the host builds the lattice of `_compute_idxs` (:308-363).
 *   sat int32[n_sat]: the saturated spots (exactly max_neighs stored neighbours), nbr int32[n_sat][max_neighs] their neighbours in
 *   the order the graph stores them (also the order of the neighbour sum); unsat int32[n_unsat] the other spots and src[q] the
 *   POSITION in sat[] of unsat[q]'s nearest saturated spot.  n_sat + n_unsat == n, every spot exactly once; max_neighs 4 (square
 *   grid, d2 = nbrs - 4c) or 6 (hex grid, d2 = (2 nbrs - 12c) / 3).
 * sqgr_sepal_run: genes = columns cols[0 .. G) of m (n rows); out_iter[g] = the first sweep i with |ent_i - ent_{i-1}| <= thresh
 *   (the reference's score is dt * i), -1 when no sweep within n_iter qualifies (NaN).  The concentrations follow numpy's bit for
 *   bit; the entropy is a fixed-order float64 reduction, so a gene's result depends on that gene alone.
 * sqgr_sepal_trace (parity hook): exactly n_steps sweeps of column col without a stop test; out_conc float64[n] the vector after
 *   them, out_ent float64[n_steps] ent_i of every sweep; either may be NULL. */
typedef struct sqgr_sepal sqgr_sepal;
int sqgr_sepal_create(sqgr_ctx* ctx, int64_t n, int32_t max_neighs, const int32_t* sat, int64_t n_sat, const int32_t* nbr,
                      const int32_t* unsat, const int32_t* src, int64_t n_unsat, sqgr_sepal** out);
int sqgr_sepal_run(sqgr_sepal* h, const sqgr_matrix* m, const int32_t* cols, int64_t G, int32_t n_iter, double dt, double thresh,
                   int32_t* out_iter);
int sqgr_sepal_trace(sqgr_sepal* h, const sqgr_matrix* m, int32_t col, int32_t n_steps, double dt, double* out_conc, double* out_ent);
int sqgr_sepal_destroy(sqgr_sepal* h);

/* ---- centrality_scores: the integers behind group closeness, group degree and local clustering -------------------------------
 * Replaces what `centrality_scores` (gr/_nhood.py:245-345) asks of rustworkx and of its numba kernel.  Both entry points take the
 * graph `_build_graph` (gr/_nhood.py:432-454) builds on the host — A + A^T, diagonal and stored zeros removed, rows sorted: an
 * undirected simple graph — and return SQGR_ERR_INVALID (sqgr_last_error names which) for a graph that is not structurally
 * symmetric, has a self loop, or a row that is not strictly increasing (checked on the device).  All results are exact integers;
 * the caller forms the floats.
 * sqgr_graph_triangles: out_two_tri int64[n], two_tri[v] = sum over u in N(v) of |N(v) n N(u)| = twice the triangles through v
 *   (`_local_clustering`, :457-491: cc[v] = two_tri[v] / (k_v (k_v - 1)) for k_v >= 2).
 * sqgr_group_bfs: one multi-source BFS per group g = {i : labels[i] == g}, 64 groups per sweep of the graph; labels int32[n] in
 *   [-1, K), -1 = member of no group (the node stays in the graph).  K >= 1.  With d(g, v) the hop distance from the group's
 *   nearest member to a node v outside the group:
 *     out_adjacent[g] = #{v : d = 1}                   (group degree centrality = adjacent / (n - |g|))
 *     out_dist_sum[g] = sum of d over the reached v    (group closeness centrality = (n - |g|) / dist_sum)
 *     out_reached[g]  = #{v : d finite}                 each int64[K]; an empty group reaches nothing
 *     *out_levels     = the largest finite d of the call (0: no group reached anything). */
int sqgr_graph_triangles(sqgr_ctx* ctx, const sqgr_graph* g, int64_t* out_two_tri);
int sqgr_group_bfs(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int64_t* out_adjacent, int64_t* out_dist_sum,
                   int64_t* out_reached, int64_t* out_levels);
/* sqgr_group_bfs_hook (parity hook): the same with the grid of the level kernel given: grid_blocks >= 1 replaces 8 x compute units as the
 * cap on its blocks (a block then strides over the nodes in more trips), 0 = the default.  The integers do not depend on it. */
int sqgr_group_bfs_hook(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int64_t* out_adjacent, int64_t* out_dist_sum,
                        int64_t* out_reached, int64_t* out_levels, int32_t grid_blocks);

/* ---- calculate_niche_cellcharter: a full-covariance Gaussian mixture fitted by EM in float64 -----------------------------------
 * Replaces `GaussianMixture(n_components, random_state, init_params="random_from_data").fit(embedding).predict(embedding)`
 * (gr/_niche.py:1474-1480) and follows scikit-learn 1.7's fit step for step (n_init = 1, covariance_type = "full").
 * X: n x d row-major float64, finite (the caller checks).  init_rows int64[k]: row init_rows[c] starts as component c with
 * responsibility 1 — the caller draws `np.random.RandomState(random_state).choice(n, size=k, replace=False)`.
 * At most max_iter (>= 1) EM steps; a step converges when |lower bound - previous lower bound| < tol and its parameters are kept.
 * out_weights float64[k], out_means [k x d], out_covariances [k x d x d]: the parameters after the last M-step.
 * out_lower_bounds float64[max_iter]: one value per step taken, the first *out_n_iter are written; *out_converged 0 | 1.
 * out_labels int32[n]: argmax over the components of the weighted log-density under the final parameters, first maximum wins.
 * Two calls with the same arguments return the same bytes: every sum over rows has a fixed order that depends on (n, d, k) alone.
 * Every device buffer is taken before the first step; a step reads back 16 bytes.  Device memory: (n d + n k) doubles + O(k d^2).
 * SQGR_ERR_UNSUPPORTED for d > 64, k > 64 or n >= 2^31; SQGR_ERR_INVALID for k > n, an init row outside [0, n), and when a
 * covariance is not positive definite ("ill-defined empirical covariance": sklearn's ValueError). */
int sqgr_gmm_fit(sqgr_ctx* ctx, const double* X, int64_t n, int32_t d, int32_t k, const int64_t* init_rows, double reg_covar, double tol,
                 int32_t max_iter, double* out_weights, double* out_means, double* out_covariances, double* out_lower_bounds,
                 int32_t* out_n_iter, int32_t* out_converged, int32_t* out_labels);
/* sqgr_gmm_geometry: the launch geometry sqgr_gmm_fit derives from (n, d, k), from the function the fit itself calls.  Needs no device.
 *   out int64[20] = {columns of P padded to a strip, E-step tiles per block, E-step blocks, rows of a chunk of the covariance sums, rows
 *   of a chunk of the weighted sums, covariance chunks, weighted-sum chunks, rows staged at a time by the weighted sums, the same by
 *   the covariance sums, LDS bytes of the E-step, of the weighted sums, of the covariance sums; then the constants these are formed
 *   from: rows of an E-step tile, most E-step blocks, most chunks x components of the covariance grid, fewest rows of a chunk, most
 *   chunks of the weighted sums, columns of a strip of P, bytes of a stage, bytes of the group reduction}.
 *   SQGR_ERR_INVALID outside 1 <= d, k <= 64, 1 <= n < 2^31. */
int sqgr_gmm_geometry(int64_t n, int32_t d, int32_t k, int64_t* out);

/* ---- niche feature matrices: stage 1 of the three niche flavours, everything in front of scanpy (gr/_niche.py) -------------------
 * Float64 throughout; every sum over a row's stored entries runs in ascending column order with separately rounded products and
 * sums (no FMA); two calls with the same arguments return the same bytes.  Graphs must be in canonical CSR form (rows strictly
 * increasing) where a row is walked as a set (sqgr_shells_create checks on the device).
 *
 * sqgr_niche_info: out_info int64[4] = {on-chip capacity of the shell builder: the largest expansion — sum of the lengths of the
 *   rows of A that a row of hop_{k-1} walks — that stays in LDS, rows above it take the global-memory path; the path count limit
 *   2^24; columns of X per aggregation block; largest distance}.
 *
 * sqgr_shells_create: the hop shells of `_CellcharterEmbedder.get_embedding` (:1336-1355, `_setdiag` / `_hop` :1002-1027) as sorted
 *   CSR on the device, structure of g only (the caller has checked that every stored value is 1):
 *     vis_1 = A with its diagonal, every count 1;  hop_1 = A without its diagonal
 *     P_k = hop_{k-1} @ A (integer path counts, self loops of A take part);  hop_k = P_k > vis_{k-1} (absent = 0);
 *     vis_k = vis_{k-1} + hop_k                                                for k = 2 .. distance
 *   Not a BFS: a visited node re-enters shell k whenever more paths reach it than it has been visited.  count_limit: 0, or a lower
 *   limit than 2^24 (tests); SQGR_ERR_UNSUPPORTED when a path count reaches the limit, and for n >= 2^31 - 1.
 * sqgr_shells_info: out_info int64[5] = {n, nnz of hop_k, nnz of vis_k, rows of shell k built on the global-memory path, rows whose
 *   expansion was exactly the on-chip capacity}, 1 <= k <= distance.
 * sqgr_shells_read: hop_k and vis_k with its visit counts; indptr int64[n + 1], indices / counts int32[nnz]. */
typedef struct sqgr_shells sqgr_shells;
int sqgr_niche_info(int64_t* out_info);
int sqgr_shells_create(sqgr_ctx* ctx, const sqgr_graph* g, int32_t distance, int32_t count_limit, sqgr_shells** out);
int sqgr_shells_info(const sqgr_shells* h, int32_t k, int64_t* out_info);
int sqgr_shells_read(const sqgr_shells* h, int32_t k, int64_t* hop_indptr, int32_t* hop_indices, int64_t* vis_indptr, int32_t* vis_indices,
                     int32_t* vis_counts);
int sqgr_shells_destroy(sqgr_shells* h);
/* sqgr_niche_aggregate: out[i * ld_out + j] for every column j of the resident matrix m (dense / CSR / CSC, float32 / float64,
 *   densified on the device one block of columns at a time), out a HOST array of n rows, ld_out >= n_cols doubles apart.  Exactly
 *   one of g and shells is given:
 *     shells, k = 0:      X itself (block 0 of :1345)
 *     shells, k >= 1:     `_aggregate(adata, _normalize(hop_k), ...)` (:1030-1054): with d = 1 / (stored entries of the row), 1 / 0 -> 0,
 *                         m1 = sum_j d * x_j; variance != 0: m2 = sum_j d * (x_j * x_j) and m2 - m1 * m1
 *     g (k, variance 0):  `normalize(A, norm="l1", axis=1) @ X` (:1259-1260): sum_j (a_ij / sum_j |a_ij|) * x_j, a row of norm 0 keeps
 *                         its entries; a graph created without weights counts 1 per entry. */
int sqgr_niche_aggregate(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_shells* shells, int32_t k, const sqgr_matrix* m, int32_t variance,
                         double* out, int64_t ld_out);
/* sqgr_niche_label_hops: the hop profiles of `_NhoodProfileEmbedder` (:1117-1209) for hops 1 .. distance in one call:
 *   out float64[distance][n][K], out[h - 1] = A^h onehot(labels) formed as A (A^(h-1) onehot) — A^h itself is never built.
 *   labels int32[n], a label outside [0, K) belongs to no category.  weighted != 0: the graph's weights (it must carry them), else 1
 *   per stored entry.  normalise != 0: every row of every hop is then divided by its sum over the categories (ascending), 0 / 0 -> 0
 *   (`abs_nhood=False`, :1163-1167). */
int sqgr_niche_label_hops(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int32_t distance, int32_t weighted,
                          int32_t normalise, double* out);

/* ---- PCA of a dense matrix resident on the device: the parts of scanpy's default `sc.tl.pca` that grow with n ---------------------
 * (sklearn's `PCA(n_components, svd_solver="arpack")`, what the reference's utag and cellcharter flavours call next: gr/_niche.py
 * :1262, :1357.)  The handle owns F, float64[n][D] row-major, on the device.  The caller diagonalises the D x D scatter matrix on
 * the host between sqgr_pca_moments and sqgr_pca_project.  Float64 throughout, no float atomics, no FMA; every order of summation
 * depends on (n, D) alone, so two calls return the same bytes.
 *
 * sqgr_pca_info: out_info int64[4] = {rows of a chunk of the row sums (chunks hold a multiple of it), largest D, largest c, columns
 *   of a scatter tile}.  Needs no device.
 * sqgr_pca_create: F zeroed.  SQGR_ERR_UNSUPPORTED unless 2 <= n < 2^31 and 2 <= D <= 4096.
 * sqgr_pca_upload: F[:, col0 : col0 + n_cols] = x, a HOST row-major matrix of n rows, ld values apart, of value_bytes 8 (float64)
 *   or 4 (float32, widened exactly).
 * sqgr_pca_fill_aggregate: the block sqgr_niche_aggregate(ctx, g, shells, k, m, variance, ...) returns — same arguments, kernels and
 *   arithmetic — written to F[:, col0 : col0 + m.n_cols] on the device instead of a host array.
 * sqgr_pca_moments: out_mean float64[D], mean_j = (sum_i F[i][j]) / n, a fixed-order sum and one division;  out_scatter
 *   float64[D][D], S[a][b] = sum_i (F[i][a] - mean_a) * (F[i][b] - mean_b): the mean is subtracted before the product, the sum is
 *   not divided, and S is exactly symmetric.
 * sqgr_pca_project: out float64[n][c] (HOST), out[i][r] = sum_j (F[i][j] - mean_j) * components[r][j] with j ascending and the mean
 *   of the last sqgr_pca_moments (SQGR_ERR_INVALID when F was written since); components float64[c][D] on the host.
 *   SQGR_ERR_UNSUPPORTED unless 1 <= c <= 64 and c < min(n, D). */
typedef struct sqgr_pca sqgr_pca;
int sqgr_pca_info(int64_t* out_info);
int sqgr_pca_create(sqgr_ctx* ctx, int64_t n, int32_t D, sqgr_pca** out);
int sqgr_pca_upload(sqgr_pca* h, const void* x, int32_t value_bytes, int64_t ld, int32_t col0, int32_t n_cols);
int sqgr_pca_fill_aggregate(sqgr_pca* h, int32_t col0, const sqgr_graph* g, const sqgr_shells* shells, int32_t k, const sqgr_matrix* m,
                            int32_t variance);
int sqgr_pca_moments(sqgr_pca* h, double* out_mean, double* out_scatter);
int sqgr_pca_project(sqgr_pca* h, const double* components, int32_t c, double* out);
int sqgr_pca_destroy(sqgr_pca* h);
/* sqgr_pca_geometry: the launch geometry sqgr_pca_moments derives from (n, D), from the function it calls itself.  Needs no device.
 *   out int64[10] = {column tiles, tile pairs of the upper triangle, rows of a chunk of the column sums, rows of a chunk of the scatter,
 *   chunks of the column sums, chunks of the scatter; then the constants these are formed from: the chunk unit, most chunks, the target
 *   of tile pairs x chunks, columns of a tile}.  SQGR_ERR_INVALID outside 2 <= n < 2^31, 2 <= D <= 4096. */
int sqgr_pca_geometry(int64_t n, int32_t D, int64_t* out);

/* ---- exact kNN in feature space and UMAP's fuzzy kNN weights: the parts of `sc.pp.neighbors(adata, n_neighbors, use_rep="X")` that
 * grow with n (gr/_niche.py:1417, in front of `sc.tl.leiden`).  Float64 throughout, no float atomics, no FMA.
 *
 * sqgr_knn_nd_info: out_info int64[4] = {query rows of a block, candidate rows of a tile, largest D, largest k}.  Needs no device.
 * sqgr_knn_nd: x a HOST row-major matrix of n rows and D columns, ld values apart, of value_bytes 8 (float64) or 4 (float32, widened
 *   exactly).  For every row its k nearest OTHER rows (self excluded by index), ascending by (d2, index): ties go to the smaller
 *   index.  out_idx int32[n][k], out_d2 float64[n][k] (HOST), out_d2[i][r] = sum_j (x[i][j] - x[c][j])^2 with j ascending and every
 *   difference, product and sum rounded on its own — sklearn's KD-tree `rdist`; the caller takes the square root.  All pairs are
 *   computed (3 D float64 operations per ordered pair).  The result does not depend on the launch geometry; two calls return the
 *   same bytes.  SQGR_ERR_UNSUPPORTED unless 1 <= D <= 256, 1 <= k <= min(64, n - 1) and n < 2^31.
 * sqgr_fuzzy_knn: UMAP's `smooth_knn_dist` and `compute_membership_strengths` for local_connectivity = 1, one lane per row.
 *   dist float64[n][k] (HOST): the true distances of a row's k neighbours, ascending; the row's own zero is the implicit column 0 of
 *   scanpy's m = k + 1 neighbours.  rho_i = the first dist[i][j] > 0, else 0.  sigma_i: bisection from lo = 0, hi = inf, mid = 1, at
 *   most 64 sweeps of psum = sum_j (dist[i][j] - rho_i > 0 ? exp(-((dist[i][j] - rho_i) / mid)) : 1), j ascending, until
 *   |psum - log2(m)| < 1e-5; psum > log2(m): hi = mid, mid = (lo + hi) / 2; else lo = mid, mid = hi == inf ? 2 mid : (lo + hi) / 2.
 *   Then sigma_i = max(sigma_i, 1e-3 * (sum_j dist[i][j], ascending) / m) when rho_i > 0, else max(sigma_i, 1e-3 * mean_all), with
 *   mean_all = dist.sum() / (n m) from the caller.  out_iters[i] int32: the index of the last sweep, 0 .. 63.  out_vals
 *   float64[n][k] = (dist[i][j] - rho_i <= 0 or sigma_i == 0) ? 1 : exp(-((dist[i][j] - rho_i) / sigma_i)).
 *   SQGR_ERR_UNSUPPORTED unless 1 <= k <= 64 and n < 2^31. */
int sqgr_knn_nd_info(int64_t* out_info);
int sqgr_knn_nd(sqgr_ctx* ctx, const void* x, int32_t value_bytes, int64_t n, int32_t D, int64_t ld, int32_t k, int32_t* out_idx,
                double* out_d2);
int sqgr_fuzzy_knn(sqgr_ctx* ctx, const double* dist, int64_t n, int32_t k, double mean_all, double* out_rho, double* out_sigma,
                   int32_t* out_iters, double* out_vals);

/* ---- Leiden communities of a symmetric weighted graph: `sc.tl.leiden(adata, resolution)` of the `neighborhood` and `utag` flavours
 * (gr/_niche.py:1428; leidenalg's RBConfigurationVertexPartition, Q = sum_c (in_c / 2m - gamma (tot_c / 2m)^2)) as a deterministic
 * synchronous variant on exact integers.  leidenalg itself is randomised; parity with it is not claimed.
 *
 * sqgr_leiden_info: out_info int64[6] = {weight scale bits (the caller quantises q = max(1, rint(w / w_max * 2^24)), int32), sweep cap
 *   of one local moving or refinement phase, iteration cap for n_iterations < 0, on-chip capacity: the stored entries of a row up to
 *   which its neighbour communities are tabulated in LDS (longer rows take the global-memory path), slots of that table, entries of
 *   out_stats}.  Needs no device.
 * sqgr_leiden: HOST arrays in canonical CSR: indptr int64[n + 1], indices int32[nnz] strictly increasing in a row, no self loop, every
 *   entry mirrored with an equal weight, weights int32[nnz] >= 1 — checked on the device, SQGR_ERR_INVALID names the property that
 *   failed.  resolution finite and > 0; n_iterations > 0, or < 0 for "until an iteration changes nothing" (at most the iteration cap).
 *   SQGR_ERR_UNSUPPORTED when the sum of all weights 2m reaches 2^62 or n >= 2^31 - 1.
 *   Arithmetic: every k_v, k_{v,c}, tot_c, in_c and 2m is an exact int64 on every level.  The one floating-point expression is
 *     gain(v, c) = (double)k_vc - gamma * (double)k_v * (double)(tot_c - [c == comm(v)] k_v) / (double)two_m
 *   evaluated left to right, every operation rounded on its own.  Candidates: (gain descending, community id ascending); a move needs
 *   gain(v, c) > gain(v, comm(v)) strictly; a self loop of a coarse node counts in k_v, not in k_vc.
 *   Per iteration and level: (1) local moving in synchronous sweeps s = 0, 1, ..: every vertex picks its best target among its
 *   neighbours' communities on the state the sweep began with; of the vertices that want to move, one moves when
 *   (hash(vertex, s), vertex) is smaller than that of every neighbour that wants to move too, hash(v, s): x = v * 0x9E3779B1 + s *
 *   0x85EBCA77; x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16 (uint32).  Against overshoot, of all the
 *   vertices that want into one community c (W_c the sum of their k) the one of smallest (hash, vertex) is exempt; any other moves
 *   only if (double)k_vc - gamma * (double)k_v * (double)(tot_c + W_c - k_v) / two_m > gain(v, comm(v)).  Ends at a sweep without a move,
 *   or after the sweep cap with the assignment of largest Q among the start and every sweep (the first such), Q = (double)sum_in /
 *   (double)two_m - gamma * ((double)sum_c tot_c^2 / ((double)two_m * (double)two_m)) from the exact integers.  (2) Refinement from
 *   singletons, the same sweeps with targets inside the vertex's community: only a vertex still alone moves, and only when
 *   (double)k_{v, C - v} >= gamma * (double)k_v * (double)(tot_C - k_v) / two_m; a target S needs the same of k_{S, C - S} and tot_S;
 *   gain(v, S) = k_vS - gamma k_v tot_S / 2m must be > 0.  (3) Aggregation: refined communities numbered ascending by their id
 *   become nodes, parallel edges summed, inner weight on a self loop; a node starts in the community of its members.  The levels
 *   end when local moving leaves every node alone or refinement merges nothing; the last level's nodes are the communities.  An
 *   iteration starts at the input graph from the previous labels.
 *   out_labels int32[n] in [0, K): communities numbered by size descending, ties by smallest member.  out_stats int64[8] = {K,
 *   iterations run, levels, sweeps, sum_c in_c of the result, 2m, local moving phases that ended at the sweep cap, 1 when the last
 *   iteration changed nothing}.  A graph without entries: every vertex alone, all other stats 0.
 *   The result does not depend on the launch geometry; two calls return the same bytes. */
int sqgr_leiden_info(int64_t* out_info);
int sqgr_leiden(sqgr_ctx* ctx, int64_t n, const int64_t* indptr, const int32_t* indices, const int32_t* weights, double resolution,
                int32_t n_iterations, int32_t* out_labels, int64_t* out_stats);
/* sqgr_leiden_hook (parity hook): the same with the grid of the grid-stride kernels given: grid_blocks >= 1 replaces 8 x compute units
 * (the kernels then cover the rows and entries in more trips), 0 = the default.  Labels and stats do not depend on it. */
int sqgr_leiden_hook(sqgr_ctx* ctx, int64_t n, const int64_t* indptr, const int32_t* indices, const int32_t* weights, double resolution,
                     int32_t n_iterations, int32_t* out_labels, int64_t* out_stats, int32_t grid_blocks);

/* ---- Multiplex Leiden on two layers over the same vertices: what `calculate_niche_spatialleiden` (gr/_niche.py:466-620) gets from
 * spatialleiden, i.e. leidenalg's optimise_partition_multiplex over one RBConfigurationVertexPartition per layer with layer_weights
 * [1, layer_ratio].  Layer 0 is the latent graph, layer 1 the spatial graph.  The objective is unnormalised,
 *     Q = sum_l a_l sum_c (in^l_c - gamma_l (tot^l_c)^2 / 2m_l),  a_0 = 1, a_1 = layer_ratio,
 * so a layer counts in proportion to its total weight; the caller quantises both layers with ONE common scale.  Parity with
 * spatialleiden / leidenalg is not claimed.  The contract is sqgr_leiden's with the changes below and nothing else.
 *
 * sqgr_leiden_multiplex_info: out_info int64[7] = the six entries of sqgr_leiden_info (entries of out_stats: 10), then the number of
 *   layers (2).  Needs no device.
 * sqgr_leiden_multiplex: per layer l HOST arrays as for sqgr_leiden (canonical symmetric CSR, no self loop, int32 weights >= 1); a
 *   layer may be empty (indptr all zero; indices / weights may then be null).  Checked on the device; SQGR_ERR_INVALID names the layer
 *   ("layer 0" / "layer 1") and the property that failed.  resolution0, resolution1 and layer_ratio finite and > 0; n_iterations as for
 *   sqgr_leiden.  SQGR_ERR_UNSUPPORTED when either 2m_l reaches 2^62 or n >= 2^31 - 1.
 *   Integers: every k^l_v, k^l_{v,c}, tot^l_c, in^l_c, 2m_l and W^l_c is an exact int64, per layer and on every level.
 *   Gain: per layer g_l(v, c) = (double)k^l_vc - gamma_l * (double)k^l_v * (double)(tot^l_c - [c == comm(v)] k^l_v) / (double)two_m_l,
 *   left to right, every operation rounded on its own; g_l is exactly +0.0 for a layer with 2m_l = 0.  gain(v, c) = g_0 + layer_ratio *
 *   g_1: the product is rounded, then the sum, no FMA.  Every floating-point test below mixes its two per-layer terms t_0, t_1 the same
 *   way, t_0 + layer_ratio * t_1, a term being +0.0 for a layer with 2m_l = 0.
 *   Candidates: the communities of v's neighbours in either layer, plus its own; one candidate per community (its k^0_vc and k^1_vc
 *   belong to the same candidate).  Order (gain descending, community id ascending) and the strict-improvement rule as in sqgr_leiden.
 *   Independent set: a vertex that wants to move yields to a neighbour IN EITHER LAYER that wants to move too and has the smaller
 *   (hash(vertex, s), vertex).  Overshoot rule: W^l_c, the sum of k^l_v over the vertices that want into c, is kept per layer; a vertex
 *   that is not the first of them moves only if t_l = (double)k^l_vc - gamma_l * (double)k^l_v * (double)(tot^l_c + W^l_c - k^l_v) /
 *   two_m_l mixed as above is > gain(v, comm(v)).
 *   Quality at the sweep cap: Q = (double)two_m_0 * q_0 + layer_ratio * ((double)two_m_1 * q_1), q_l the single-layer expression of
 *   sqgr_leiden formed from layer l's exact integers, 0 for a layer with 2m_l = 0.
 *   Refinement: a vertex is well connected when (x_0 - p_0) + layer_ratio * (x_1 - p_1) >= 0 with x_l = (double)k^l_{v, C - v} and p_l =
 *   gamma_l * (double)k^l_v * (double)(tot^l_C - k^l_v) / two_m_l; a target S needs the same of k^l_{S, C - S} and tot^l_S; S must be
 *   adjacent to v in at least one layer and gain(v, S) (g_l = k^l_vS - gamma_l k^l_v tot^l_S / 2m_l) must be > 0.
 *   Aggregation: one coarse CSR per layer over the same numbering of the refined communities; the self loop of a coarse node in
 *   layer l carries in^l_c.  Levels, iterations and the canonical labelling as in sqgr_leiden.
 *   out_labels int32[n]; out_stats int64[10] = {K, iterations run, levels, sweeps, sum_c in^0_c, 2m_0, sum_c in^1_c, 2m_1, local moving
 *   phases that ended at the sweep cap, 1 when the last iteration changed nothing}.  Both layers empty: every vertex alone, all other
 *   stats 0.  On-chip path: a row whose stored entries in layer 0 plus those in layer 1 are <= the capacity; otherwise the
 *   global-memory path.  The result does not depend on the path or the launch geometry; two calls return the same bytes. */
int sqgr_leiden_multiplex_info(int64_t* out_info);
int sqgr_leiden_multiplex(sqgr_ctx* ctx, int64_t n, const int64_t* indptr0, const int32_t* indices0, const int32_t* weights0,
                          const int64_t* indptr1, const int32_t* indices1, const int32_t* weights1, double resolution0, double resolution1,
                          double layer_ratio, int32_t n_iterations, int32_t* out_labels, int64_t* out_stats);
/* sqgr_leiden_multiplex_hook (parity hook): grid_blocks as for sqgr_leiden_hook. */
int sqgr_leiden_multiplex_hook(sqgr_ctx* ctx, int64_t n, const int64_t* indptr0, const int32_t* indices0, const int32_t* weights0,
                               const int64_t* indptr1, const int32_t* indices1, const int32_t* weights1, double resolution0, double resolution1,
                               double layer_ratio, int32_t n_iterations, int32_t* out_labels, int64_t* out_stats, int32_t grid_blocks);

/* ---- mask_graph: `LineString([a_k, b_k]).within(polygon_mask)` for every edge of a spatial graph (gr/_build.py:852-954), as the numpy
 * restatement squidpy_amd/gr/_mask.py evaluates it: plain float64 cross products, divisions and comparisons, every operation rounded
 * on its own (no FMA), IEEE division — the device returns that code's booleans bit for bit.
 *
 * sqgr_mask_info: out_info int64[2] = {cut parameters of one segment held on chip (0 and 1 included), (point or segment, ring edge)
 *   pairs of one kernel launch}.  Needs no device.
 * sqgr_segments_within: HOST arrays.  a_xy, b_xy float64[E][2]: the segments' ends.  ring_xy float64[P][2]: all rings concatenated as
 *   closed coordinate lists (first point == last point, at least 4 stored points each); ring_offsets int64[n_rings + 1]: ring r is
 *   points [ring_offsets[r], ring_offsets[r + 1]), ring_offsets[0] = 0; ring_polygon int32[n_rings]: the polygon of every ring,
 *   counting up from 0, a polygon's rings contiguous and its first ring the shell, the others holes.  Crossing parity is kept per
 *   ring: a point is in a hole when it is inside ANY hole of the polygon.  SQGR_ERR_INVALID for a ring that is not closed or shorter,
 *   ids out of order, E or the number of ring edges R >= 2^31, or a coordinate that is not finite.  E = 0 is valid.
 *   out_within uint8[E]: 0, 1, or 2 = overflow: the segment is cut (touches a ring, neither end outside) and would produce more cut
 *   parameters — 0, 1, one per crossing, two per collinear ring edge — than the first entry of sqgr_mask_info; the caller recomputes
 *   such a row on the host.  out_stats int64[4] = {touched segments, cut segments (overflowed ones included), overflow, launches of
 *   the kernels that walk the ring edges}.  Brute force over the ring edges: E R pair tests and 3 E R point-edge tests, cut into
 *   launches of at most the second entry of sqgr_mask_info pairs.  Two calls return the same bytes.
 * sqgr_segments_within_hook (parity hook): the same with pairs_per_launch (0 = the default) and, when out_classes is not NULL,
 *   out_classes uint8[3][E] = the classes of a, b and 0.5 (a + b): 0 outside, 1 on a boundary, 2 inside (`_classify`). */
int sqgr_mask_info(int64_t* out_info);
int sqgr_segments_within(sqgr_ctx* ctx, const double* a_xy, const double* b_xy, int64_t E, const double* ring_xy, const int64_t* ring_offsets,
                         const int32_t* ring_polygon, int64_t n_rings, uint8_t* out_within, int64_t* out_stats);
int sqgr_segments_within_hook(sqgr_ctx* ctx, const double* a_xy, const double* b_xy, int64_t E, const double* ring_xy,
                              const int64_t* ring_offsets, const int32_t* ring_polygon, int64_t n_rings, uint8_t* out_within, int64_t* out_stats,
                              int64_t pairs_per_launch, uint8_t* out_classes);

/* ---- var_by_distance: the distance from every observation to the nearest member of each anchor set (tl/_var_by_distance.py:129-134,
 * one sklearn KDTree per (anchor, slide) queried with every observation of the slide) — all anchors and all slides in one call.
 * Float64, no FMA, sklearn's order of operations: euclidean sqrt(min((dx*dx + dy*dy) + dz*dz)) with one correctly rounded square
 * root at the end, manhattan min((|dx| + |dy|) + |dz|), chebyshev min(max |d|) — KDTree.query's distances bit for bit.
 *
 * sqgr_anchor_dist_info: out_info int64[5] = {points below which a set is one cell (swept whole), target points per cell, largest
 *   dim, most anchor columns of a call, threads of a query block}.  Needs no device.
 * sqgr_anchor_dist: HOST arrays.  q float64[nq][dim] row-major, dim 2 or 3; q_slide int32[nq]: the slide of every query, -1 = no
 *   result; r float64[nr][dim]: the reference points of all sets, in any order; r_set int32[nr]: the set of each; set_of
 *   int32[n_anchors][n_slides]: the set that anchor column a searches for a query of slide s, or -1; set ids are
 *   0 .. n_anchors * n_slides - 1 and a set may serve several pairs.  metric: 0 euclidean, 1 manhattan, 2 chebyshev.
 *   out float64[n_anchors][nq]: out[a][i] = min over j with r_set[j] == set_of[a][q_slide[i]] of the metric distance; NaN when the
 *   query has no slide, the pair has no set, or the set has no point.  Every set gets a uniform cell grid built on the device; one
 *   launch of the query kernel serves all (query, anchor column) pairs.  out_stats int64[4] = {cells of all grids, sets with more
 *   than one cell, launches of the query kernel, reference points}.  Two calls return the same bytes.  SQGR_ERR_INVALID for a
 *   coordinate that is not finite, dim other than 2 or 3, a slide or set id out of range, nq or nr >= 2^31 - 1, nq < 1, more than the
 *   fourth entry of sqgr_anchor_dist_info anchor columns.
 * sqgr_anchor_dist_hook (parity hook, tuning): the same with the one-cell threshold and the target points per cell given (0 = the
 *   defaults). */
int sqgr_anchor_dist_info(int64_t* out_info);
int sqgr_anchor_dist(sqgr_ctx* ctx, int32_t dim, const double* q, const int32_t* q_slide, int64_t nq, const double* r, const int32_t* r_set,
                     int64_t nr, const int32_t* set_of, int32_t n_anchors, int32_t n_slides, int32_t metric, double* out, int64_t* out_stats);
int sqgr_anchor_dist_hook(sqgr_ctx* ctx, int32_t dim, const double* q, const int32_t* q_slide, int64_t nq, const double* r, const int32_t* r_set,
                          int64_t nr, const int32_t* set_of, int32_t n_anchors, int32_t n_slides, int32_t metric, double* out, int64_t* out_stats,
                          int64_t brute_below, double target_per_cell);

#ifdef __cplusplus
}
#endif
#endif /* SQGR_H */
