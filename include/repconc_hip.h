/*
 * repconc_hip.h — C ABI of librepconc_hip.so, the MI355X (gfx950) implementation of the
 * RepCONC product-quantisation hot path.
 *
 * The reference (jingtaozhan/RepCONC) is pure Python: the "plugin interface" of this path is
 * the Python surface of `repconc.models.repconc`.  This header is the C-level
 * boundary a maintainer binds with ctypes from those Python functions (INTEGRATION.md shows the
 * stubs).  Each entry point names the reference lines it replaces; paths are relative to
 * /root/reference/src/repconc/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the handle's HIP device unless suffixed `_host`;
 *   - the caller allocates every buffer (sizes given below / by the *_bytes helpers);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); functions only
 *     ENQUEUE work on it and return, they never synchronise;
 *   - return value: RC_OK (0) or a negative RC_E* code, never throws; rc_error_string() decodes;
 *   - no global mutable state outside the handle; handles are independent and re-entrant;
 *   - K (centroids per sub-quantiser) must be 256 (evaluate_repconc.py:80, run_warmup.py:90);
 *     M may be any divisor of D (modeling_repconc.py:41): dsub = D/M in {8,12,16,24,32,48,64,96} (the recipes' widths)
 *     runs on specialised kernels, any other width on run-time-width kernels with the same arithmetic — the fp32
 *     summation order of the torch-CPU oracle, SURVEY.md §8 a-1, pinned for all 18 divisors of 768;
 *     search: rc_index_search, rc_adc_search_exact and the Python boundary serve ANY M (round 5); the raw screening
 *     entries rc_adc_search / _img / _q have kernels for M in {8,12,16,24,32,48,64,96} and return RC_ESHAPE for any other M
 *     BEFORE anything is enqueued — the caller's route is then rc_adc_search_exact (same results, exact scan with a
 *     run-time width), which is what rc_index_search does itself; the list-centric IVF entries need M in {16,32,48,64,96};
 *   - fp32 arithmetic follows the reference bit for bit (no FMA contraction, IEEE division);
 *     the fp64 Sinkhorn stage is evaluated with potentials and is specified
 *     on its OUTPUT, the codes.
 */
#ifndef REPCONC_HIP_H
#define REPCONC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_OK 0
#define RC_EINVAL (-1)     /* bad argument (null pointer, negative size, …)            */
#define RC_ESHAPE (-2)     /* unsupported K / dsub / M                                 */
#define RC_EHIP (-3)       /* a HIP runtime call failed (see rc_last_hip_error)        */
#define RC_EWORKSPACE (-4) /* workspace smaller than the matching *_ws_bytes()         */
#define RC_ECOMM (-5)      /* RCCL unavailable or a collective call failed             */
#define RC_ESELECT (-6)    /* ADC candidate selection did not converge (thousands of identical codes) */

#define RC_CODE_U8 0
#define RC_CODE_I64 1

/* bits of the `flags` word written by the Sinkhorn entry points */
#define RC_FLAG_NONFINITE 1 /* a row/column sum became 0, inf or NaN — the reference's   */
                            /* "Sinkhorn Algorithm returns nan/inf values" warning,      */
                            /* models/repconc/modeling_repconc.py:64-65                  */
#define RC_FLAG_COMM 4      /* IPC transport: a peer's signal did not arrive within RC_IPC_TIMEOUT_MS (default 600000): */
                            /* the wait gave up instead of hanging the GPU; the codes of this call are garbage       */
#define RC_FLAG_RANGE 2     /* |(L + f) N/ln2| left the range the sweep's integer split  */
                            /* covers: eps < ~3e-4 on centred distances — or, at any eps, a row potential that is already NaN,   */
                            /* then together with RC_FLAG_NONFINITE.                                                           */
/* The band in eps (tests/test_sinkhorn_strain.py).  Exact parity with the reference's codes is promised for     */
/* eps >= 0.003.  The reference's plan starts as exp(-d/eps)/tot with centred distances reaching +-1, so its smallest entries     */
/* are subnormal or zero once 2/eps + ln(B K) > ~708 (eps < ~0.00288 at B K = 2^18; its exp(1/eps) overflows only at eps <       */
/* 1.4e-3): below that its codes depend on its own underflow.  There this library returns the codes of the same iteration in      */
/* potentials (log) form, which loses no single entry, with flags 0 — unless a whole COLUMN underflows (every exp(L + f) of a row  */
/* of x is 0: max_k (L + f) < -745, e.g. one far outlier row at eps < ~0.0027), which is the reference's NaN warning case and is  */
/* reported as RC_FLAG_NONFINITE (| RC_FLAG_RANGE from the next sweep on); the codes are then in range and repeatable, no more.  */

typedef struct rc_handle_s* rc_handle_t;
typedef void* rc_stream_t;
typedef struct rc_index_s* rc_index_t;   /* stateful PQ index, see rc_index_* below */

int rc_version(void);
const char* rc_error_string(int code);
int rc_create(rc_handle_t* out, int device);
int rc_destroy(rc_handle_t h);
int rc_last_hip_error(rc_handle_t h); /* hipError_t of the last RC_EHIP on this handle */
int rc_num_cus(rc_handle_t h);

/* ------------------------------------------------------------------ measurement hook
 * With profiling enabled every launch of a hot kernel is bracketed by a pair of hipEvents recorded
 * on the launch stream.  rc_profile_collect() waits for the recorded events of one kernel class,
 * returns the number of launches and the summed device time in milliseconds, and clears them.
 * Classes: 0 = Sinkhorn sweep (sk_sweep_kernel, t >= 1), 1 = ADC filter scan, 2 = nearest assignment,
 * 3 = distance table.  bench.py's `roofline.achieved` comes from this.
 * on = 1: one event pair per launch (the Sinkhorn solve then runs its eager launch loop).  on = 2 ("bracket"): ONE pair
 * around the whole run of sweeps t >= 2 of a solve — eager or replayed from the captured hipGraph — counted as that
 * many launches: two event records per solve, the inter-launch gaps (~1.5 us each) are inside the measured time. */
int rc_profile_enable(rc_handle_t h, int on);
int rc_profile_collect(rc_handle_t h, int kernel_class, int* launches, double* total_ms);

/* ------------------------------------------------------------------ a-1 / a-5
 * Nearest-centroid codes (index build).  Replaces RepCONC.quantize with use_constraint=False,
 * models/repconc/modeling_repconc.py:49-52,66: code[b,m] = argmin_k sum_j (x[b,m*dsub+j]-C[m,k,j])^2,
 * first minimum wins.  x: [B, ldx>=D] fp32 row-major; C: [M,K,dsub] fp32.
 * Either output may be NULL: codes_u8 [B,M] (what evaluate_repconc.py:69 casts to) and
 * codes_i64 [B,M] (what quantize returns). */
int rc_pq_assign_nearest(rc_handle_t h, const float* x, int64_t ldx, const float* C, int64_t B,
                         int D, int M, int K, uint8_t* codes_u8, int64_t* codes_i64,
                         rc_stream_t stream);

/* Same codes, bit for bit, ~5.7x faster: the bf16 matrix cores (v_mfma_f32_32x32x16_bf16 on operands split into two
 * bf16 pieces, three products) screen with the GEMM form ||c||^2 - 2<c,x>; every (row, m) whose best/second-best gap is
 * inside the rounding bound of that form is recomputed with the reference's exact arithmetic and first-minimum rule
 * (csrc/pq_assign_mfma.hip).  x must be 16-byte aligned with ldx % 4 == 0 and B*M < 2^32.
 * ws: rc_pq_assign_nearest_fast_ws_bytes(B, M) bytes (one doubt-list slot per pair: the list cannot overflow; plus the
 * staged bf16 image of the centroids, written once per call by assign_prep_kernel and fetched by every block).
 * Asynchronous and complete — no follow-up call is needed.  rc_pq_assign_nearest_fast_overflow (synchronises) only
 * reports the number of doubtful pairs in *doubtful and returns 0.
 * The rounding bound: a pair is doubtful unless its best screened value leads the second best by more than
 * margin * (||x_m||^2 + max_k ||c_mk||^2), margin = 2 E = 2 [3.63e-5 + (3 KP + 7) 3.6e-7 + (2 dsub + 4) 1.2e-7], KP = dsub
 * rounded up to 16 (1.21e-4 at dsub 16; the terms are derived in the header of csrc/pq_assign_mfma.hip).
 * rc_pq_assign_nearest_fast_margin(dsub) returns the compiled margin, negative for a width without a screen; no GPU. */
size_t rc_pq_assign_nearest_fast_ws_bytes(int64_t B, int M);
float rc_pq_assign_nearest_fast_margin(int dsub);
int rc_pq_assign_nearest_fast(rc_handle_t h, const float* x, int64_t ldx, const float* C, int64_t B,
                              int D, int M, int K, uint8_t* codes_u8, int64_t* codes_i64, void* ws,
                              size_t ws_bytes, rc_stream_t stream);
int rc_pq_assign_nearest_fast_overflow(rc_handle_t h, const void* ws, int64_t B, int M, int* doubtful);

/* ------------------------------------------------------------------ a-1
 * Distance table d[M,B,K] fp32 (modeling_repconc.py:50) and, if minmax != NULL, the per-m
 * maximum (minmax[0..M)) and minimum (minmax[M..2M)) over (b,k) (:76-77).
 * ws: rc_pq_dist_table_ws_bytes(B, M) bytes of scratch (block partials).  x must be 16-byte aligned with ldx % 4 == 0
 * (the same holds for the assign_sinkhorn entry points, which start with this table). */
size_t rc_pq_dist_table_ws_bytes(int64_t B, int M);
int rc_pq_dist_table(rc_handle_t h, const float* x, int64_t ldx, const float* C, int64_t B, int D,
                     int M, int K, float* d, float* minmax, void* ws, size_t ws_bytes,
                     rc_stream_t stream);

/* ------------------------------------------------------------------ a-2
 * In place (d - mid)/amp with mid=(mx+mn)/2, amp=(mx-mid)+1e-5f per m
 * (RepCONC.center_distance_for_constraint, modeling_repconc.py:81-84).  `minmax` holds the
 * values AFTER the cross-rank all_reduce(MAX/MIN) of :78-80, which the host performs. */
int rc_pq_centre(rc_handle_t h, float* d, const float* minmax, int64_t B, int M, int K,
                 rc_stream_t stream);

/* ------------------------------------------------------------------ a-3 / a-4, staged form
 * Sinkhorn-Knopp of sinkhorn_algorithm (modeling_repconc.py:137-165) on L = -d/eps, evaluated with
 * potentials f[M,K], g[M,B] (fp64) instead of the in-place matrix Q.  One launch per sweep over d:
 *
 *   rc_sk_sweep(t = 0):   rows[m,k] = sum_b exp(L[m,b,k])                                  (:141,:155)
 *   rc_sk_sweep(t >= 1):  f -= log(sum_r rows_prev[r])   (f = 0 before t = 1)              (:157-158)
 *                         g -= log(colsum of sweep t-1)  (g = 0 in sweep 1)                (:162)
 *                         w = exp(L + f_k + g_b); colsum_b = sum_k w; rows[m,k] = sum_b w/colsum_b
 *   rc_sk_argmax(t = T):  f -= log(sum_r rows_prev[r]);  code[b,m] = argmax_k (L + f), first max (:63,:66)
 *
 * T = sinkhorn_iterations is: sweeps t = 0 … T-1, then rc_sk_argmax(t = T) — T+1 reads of d.  Between two
 * sweeps the host all-gathers `rows_out` of every rank into `rows_prev` [G,M,K] (rank-major; the rank sum of
 * :157 is taken inside the next launch in rank order; on one rank pass rows_out itself, G = 1).  The
 * constants /K, /B, the global normalisation of :152 and the last column normalisation cancel in the argmax.
 *
 * f2:       [2,M,K] fp64, potentials double-buffered by sweep parity (owned by the solve, no init needed)
 * g,colsum: [M,B] fp64-sized scratch each (no init needed).  The column potentials never reach the result (w/colsum and
 *           the argmax are independent of g), so the default sweep keeps them as int32 column exponents inside `g` and
 *           leaves `colsum` untouched; the round-1 sweep (RC_SK_V1=1) stores fp64 g and colsum.  d must be a CENTRED
 *           table (|d| <= 1, rc_pq_centre) — a wider table is rescaled together with eps by a power of two first.
 * rows_out: [M,K] fp64, this rank's row sums of the sweep
 * ws:       rc_sk_ws_bytes(B, M, K) bytes (block partials + arrival counters; sweep 0 resets the counters)
 * flags:    one int, OR-ed with RC_FLAG_* (caller zeroes it before sweep 0)
 */
size_t rc_sk_ws_bytes(int64_t B, int M, int K);
int rc_sk_sweep(rc_handle_t h, const float* d, const double* rows_prev, int G, double* f2, double* g,
                double* colsum, double* rows_out, int64_t B, int M, int K, double eps, int t, int* flags,
                void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_sk_argmax(rc_handle_t h, const float* d, const double* rows_prev, int G, const double* f2, int64_t B,
                 int M, int K, double eps, int t, uint8_t* codes_u8, int64_t* codes_i64, int* flags,
                 rc_stream_t stream);

/* ------------------------------------------------------------------ a-3 for ANY fp64 cost tensor (module boundary)
 * `sinkhorn_algorithm(out, epsilon, sinkhorn_iterations, use_distrib_train)` (modeling_repconc.py:137-165) takes any fp64
 * tensor out[M,K,B]; RepCONC.quantize passes the negated centred fp32 table, which the streaming sweep above serves.  A
 * tensor that is NOT exactly representable in fp32 is served by these two entries on the caller's fp64 data (log-domain
 * potentials, every log-sum-exp max-subtracted; deterministic; not a hot path):
 *   rc_sk64_rows: lse[m,k] = log sum_b exp(out[m,k,b]/eps + g[m,b])      (g = NULL: zeros)            (:155)
 *   rc_sk64_cols: f[m,k] = -log sum_r exp(lse_gathered[r,m,k])  (ranks in order: the all-reduce of :157),
 *                 g_out[m,b] = -log sum_k exp(out[m,k,b]/eps + f[m,k])  (NULL: potentials only)        (:158-163)
 * T iterations = rows, (cols, rows) x (T-1), cols(g_out = NULL); the plan is Q[:,:,b] = softmax_k(out/eps + f).
 * out: [M,K,B] fp64 contiguous (this rank's columns), lse / f: [M,K] fp64, g: [M,B] fp64, lse_gathered: [G,M,K] fp64. */
int rc_sk64_rows(rc_handle_t h, const double* out, const double* g, int64_t B, int M, int K, double eps, double* lse,
                 rc_stream_t stream);
int rc_sk64_cols(rc_handle_t h, const double* out, const double* lse_gathered, int G, int64_t B, int M, int K, double eps,
                 double* f_out, double* g_out, rc_stream_t stream);

/* ------------------------------------------------------------------ a-1 … a-4, one call
 * RepCONC.quantize with use_constraint=True on ONE rank (modeling_repconc.py:47-67,
 * dist.is_initialized()==False): distance table -> centring -> `iters` Sinkhorn iterations ->
 * argmax.  ws: rc_pq_assign_sinkhorn_ws_bytes(B, M, K) bytes. */
size_t rc_pq_assign_sinkhorn_ws_bytes(int64_t B, int M, int K);
int rc_pq_assign_sinkhorn(rc_handle_t h, const float* x, int64_t ldx, const float* C, int64_t B,
                          int D, int M, int K, double eps, int iters, uint8_t* codes_u8,
                          int64_t* codes_i64, int* flags, void* ws, size_t ws_bytes,
                          rc_stream_t stream);

/* ------------------------------------------------------------------ a-1 … a-4, one call, N ranks
 * RepCONC.quantize with use_constraint=True in the dist.is_initialized() branch (modeling_repconc.py:47-67 with
 * :78-80 and :149-157): every rank passes its equal row block of the batch and receives the codes of its rows; the
 * uniform-assignment constraint is over the global batch.  The exchanges (MAX/MIN of the distance range once, one
 * all-gather of the [M,256] fp64 row sums per iteration) run inside the call on the transport the handle was given:
 * IPC peer stores (below; the default of the Python boundary) — ONE chain of all M sub-quantisers, the exchange fused
 * into the sweep kernel — or RCCL (rc_comm_init), where the sub-quantisers are solved as TWO independent chains on two
 * streams so that one chain's all-gather overlaps the other's sweep (comm.hip; RC_DIST_SPLIT=0/1 overrides the rule,
 * rc_solve_num_chains_on says what a call will use).
 *
 * rc_comm_unique_ids: fill ids_host[2*128] on ONE rank (ncclGetUniqueId x2); the caller broadcasts the 256 bytes.
 * rc_comm_init: every rank, same ids; creates two communicators on the handle's device.  RC_ECOMM if RCCL
 * (librccl.so.1, resolved with dlopen at run time) is missing.
 * ws: rc_pq_assign_sinkhorn_dist_ws_bytes(B_local, M, K, world) bytes. */
int rc_comm_unique_ids(void* ids_host);
int rc_comm_init(rc_handle_t h, const void* ids_host, int rank, int world);
int rc_comm_destroy(rc_handle_t h);
int rc_comm_world(rc_handle_t h);

/* IPC transport (round 3; default of the Python boundary, RC_COMM=rccl selects RCCL): the same exchange steps — the
 * dist.all_reduce calls of modeling_repconc.py:78-80,149-157 — as hand-written peer stores.  Every rank owns one receive
 * buffer in device memory, exports it with hipIpcGetMemHandle and maps the other ranks' buffers (ranks may be processes
 * on ONE GPU — what a one-GPU box can test — or one process per GPU of a node, where the stores travel over xGMI; the
 * code is the same).  An all-gather is ONE kernel that stores this rank's slice into slot `rank` of every peer's buffer
 * and bumps the peer's arrival counter (system-scope release), followed by a one-thread kernel that waits for the local
 * counter and re-arms it: no library call, no communicator, capturable in a hipGraph like any kernel; buffers and
 * counters alternate between two parities so consecutive exchanges need no further handshake.  The wait gives up after
 * RC_IPC_TIMEOUT_MS (default 600000; flags |= RC_FLAG_COMM) instead of hanging the device when a peer has died.
 * Round 5: inside rc_pq_assign_sinkhorn_dist the per-iteration exchange (modeling_repconc.py:155-157) is part of the
 * sweep kernel itself — the block that finishes a sub-quantiser's row sums stores them and a sequence-numbered flag at
 * every peer, the next sweep's blocks of that sub-quantiser wait for the peers' flags in their prologue (after their
 * long-latency loads are on their way; a flag-wait kernel instead when ranks share a device): ONE launch per Sinkhorn
 * iteration on N ranks, one chain of all M sub-quantisers (RC_IPC_XSWEEP=0: the push + wait kernels of rounds 3-4).
 * One chain moves [M, 256] fp64 through a 256 KiB slot: M <= 128 on this transport (RC_ESHAPE before anything is
 * enqueued; RC_COMM=rccl has no limit).
 *
 * rc_comm_ipc_export: allocate this rank's buffer, write its RC_IPC_BLOB_BYTES-byte descriptor (IPC handle, device
 *   identity) to blob_host.  The caller gathers the descriptors of all ranks, rank order, through any channel
 *   (torch.distributed, a file, a pipe) and hands them to
 * rc_comm_ipc_connect: map the peers.  After it rc_pq_assign_sinkhorn_dist / rc_comm_allgather use the IPC transport.
 * rc_comm_allgather: generic all-gather of `bytes` bytes per rank into dst [world][bytes] on `stream` (either
 *   transport; per-shard k-means statistics run_warmup.py:102-113, row-sharded search results).  Every rank must call
 *   it with the same `bytes`, in the same order relative to its other collectives.
 * rc_comm_kind: 0 none, 1 RCCL, 2 IPC.  rc_comm_destroy releases either; the caller makes sure (barrier) that no peer
 *   still stores into this rank's buffer. */
#define RC_IPC_BLOB_BYTES 128
#define RC_IPC_MAX_WORLD 16
int rc_comm_ipc_export(rc_handle_t h, int rank, int world, void* blob_host);
int rc_comm_ipc_connect(rc_handle_t h, const void* blobs_host);
int rc_comm_allgather(rc_handle_t h, const void* src, void* dst, size_t bytes, int* flags, rc_stream_t stream);
int rc_comm_kind(rc_handle_t h);
int rc_comm_status(rc_handle_t h); /* IPC transport: RC_FLAG_COMM once a wait has timed out (synchronises the device) */
int rc_solve_num_chains(int world, int M); /* 1 or 2: launches per sweep (measurement bookkeeping; RCCL transport) */
int rc_solve_num_chains_on(rc_handle_t h, int world, int M); /* ... on h's transport (IPC, fused exchange: one chain) */
size_t rc_pq_assign_sinkhorn_dist_ws_bytes(int64_t B_local, int M, int K, int world);
int rc_pq_assign_sinkhorn_dist(rc_handle_t h, const float* x, int64_t ldx, const float* C, int64_t B_local,
                               int D, int M, int K, double eps, int iters, uint8_t* codes_u8,
                               int64_t* codes_i64, int* flags, void* ws, size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ a-6
 * decode (modeling_repconc.py:168-175): out[n, m*dsub:(m+1)*dsub] = C[m, codes[n,m], :], and
 * its gradient w.r.t. C (autograd of the gather at :175): grad_C[m,codes[n,m],:] += grad_out[n,m,:].
 * code_dtype: RC_CODE_U8 or RC_CODE_I64; codes are [n, M] row-major.
 * Only the low 8 bits of an int64 code are read (code & 255): no code can index outside the table. */
int rc_pq_decode(rc_handle_t h, const void* codes, int code_dtype, const float* C, int64_t n,
                 int M, int K, int dsub, float* out, rc_stream_t stream);
int rc_pq_decode_bwd(rc_handle_t h, const void* codes, int code_dtype, const float* grad_out,
                     int64_t n, int M, int K, int dsub, float* grad_C, rc_stream_t stream);
/* The same gradient summed in a fixed order (csrc/decode_det.hip; decode is modeling_repconc.py:168-184).  rc_pq_decode_bwd
 * adds with fp32 atomics, so its last bits depend on the order in which the waves arrive; this entry computes
 *   grad_C[m, c, j] = fp32( sum over the rows r with (codes[r, m] & 255) == c, r ascending, of (double) grad_out[r, m*dsub + j] )
 * with every sum in fp64, sequential from 0.0, rounded to fp32 once; an (m, c) that no row hits gets exactly +0.0f.  No atomics
 * on values: a stable counting sort of the rows by code per sub-quantiser, then one owner per output element.  The result is
 * a function of the inputs alone (bit-identical from run to run).  Unlike rc_pq_decode_bwd it OVERWRITES grad_C
 * [M, 256, dsub]: the caller need not zero it.  K must be 256; any M >= 1, dsub >= 1; 0 <= n < 2^31 (n >= 2^31: RC_ESHAPE).
 * n == 0: RC_OK, nothing is launched and grad_C is not touched.  Other argument checks as rc_pq_decode_bwd.
 * ws: rc_pq_decode_bwd_det_ws_bytes(n, M) bytes (needs no GPU; 0 for n <= 0, M <= 0 or n >= 2^31) — the sort's hist
 * [M][ceil(n/1024)][256], count [M][256], start [M][256] and perm [M][n], all uint32, each rounded up to 256 bytes; a null or
 * short workspace is RC_EWORKSPACE.  RC_DECODE_DET_MAX_GRID (default 65536) is a test switch: the most blocks a launch of this
 * entry may have, so that a small input walks every grid-stride loop. */
size_t rc_pq_decode_bwd_det_ws_bytes(int64_t n, int M);
int rc_pq_decode_bwd_det(rc_handle_t h, const void* codes, int code_dtype, const float* grad_out,
                         int64_t n, int M, int K, int dsub, float* grad_C, void* ws, size_t ws_bytes,
                         rc_stream_t stream);

/* ------------------------------------------------------------------ a-8
 * RepCONC.normalize_centrodis (modeling_repconc.py:112-116): C <- C / max(||C||_2, 1e-12). */
int rc_normalize_centroids(rc_handle_t h, float* C, int M, int K, int dsub, rc_stream_t stream);

/* ------------------------------------------------------------------ a-13
 * hist[m,k] = #{n : codes[n,m]==k} — eval_balance's 256 `.sum().item()` round trips
 * (models/repconc/finetune_repconc.py:588-592) for all sub-quantisers in one launch.
 * hist: [M,K] int32, overwritten.  Only the low 8 bits of an int64 code are read (code & 255). */
int rc_code_hist(rc_handle_t h, const void* codes, int code_dtype, int64_t n, int M, int K,
                 int32_t* hist, rc_stream_t stream);

/* ------------------------------------------------------------------ a-12 (centroid update)
 * Lloyd sufficient statistics of the k-means inside Faiss `index.train`
 * (train/run_warmup.py:113): sums[m,k,:] += x[n, m*dsub:(m+1)*dsub], counts[m,k] += 1 for
 * k = codes[n,m].  sums: [M,K,dsub] fp64, counts: [M,K] int64; ACCUMULATED into (caller
 * zeroes, so shards / ranks can be summed).  rc_kmeans_update: C = sums/counts where
 * counts>0, unchanged otherwise. */
int rc_kmeans_stats(rc_handle_t h, const float* x, int64_t ldx, const uint8_t* codes, int64_t n,
                    int D, int M, int K, double* sums, int64_t* counts, rc_stream_t stream);
int rc_kmeans_update(rc_handle_t h, const double* sums, const int64_t* counts, float* C, int M,
                     int K, int dsub, rc_stream_t stream);
/* Empty clusters after an update, by Faiss's published rule (Clustering.cpp `split_clusters`, run by `index.train`,
 * train/run_warmup.py:113): per sub-quantiser a std::mt19937(1234) walk picks a donor with probability proportional to
 * its size, the empty centroid becomes the donor's scaled by (1 +- 1/1024), the donor the opposite.  On the device (no host
 * synchronisation inside a Lloyd iteration).  counts: [M,K] int64 of the update just made; nsplit: optional device int,
 * incremented by the number of splits. */
int rc_kmeans_split_empty(rc_handle_t h, float* C, const int64_t* counts, int M, int K, int dsub, int* nsplit,
                          rc_stream_t stream);

/* ------------------------------------------------------------------ a-9 … a-11
 * PQ asymmetric-distance (inner product) top-k over raw codes — what `index.search` of the
 * faiss.IndexPQ / 1-list IndexIVFPQ does at models/repconc/evaluate_repconc.py:182 and
 * models/jpq/finetune_jpq.py:176.  Per query: LUT[m][k] = <q_m, C[m,k]>, score(n) = sum_m
 * LUT[m][codes[n,m]] (fp32, m ascending), the k largest scores sorted (score desc, id asc).
 *
 * codes: [N,M] uint8 (the index; stays resident, evaluate_repconc.py:89-98)
 * q: [nq,D] fp32;  scores: [nq,k] fp32;  ids: [nq,k] int64 = row + id_offset, -1 and -inf
 * score when fewer than k rows exist.  status_host semantics are reported through `status`
 * (device int, caller zeroes): bit0 = some query collected fewer than k candidates,
 * bit1 = candidate buffer overflowed; the host retries with another `sel_slack` (see
 * repconc_amd.index).  sel_slack: head-room of the sampled candidate threshold in standard deviations of the sample rank —
 * the threshold is the r-th best of 32768 exactly scored sample rows, r = floor(mu + sel_slack sqrt(mu + 1) + 4) + 1,
 * mu = k 32768 / N; the Python wrapper passes 3 (repconc_amd.ops.ADC_SEL_SLACK: 8e-6 repeated queries per query at k = 1000
 * over 8.84 M rows); larger = fewer repeats, more rows screened in.  ws: rc_adc_search_ws_bytes(N, M, K, nq, k) bytes. */
size_t rc_adc_search_ws_bytes(int64_t N, int M, int K, int nq, int k);
int rc_adc_search(rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C,
                  int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                  float* scores, int64_t* ids, int* status, void* ws, size_t ws_bytes,
                  rc_stream_t stream);
/* The same search with the index's PERMUTED CODE IMAGE supplied by the caller.  For M in {16,32,48,64,96} and
 * N >= 2^18 the integer screen reads a second copy of the code matrix in which the bytes of row n are stored in the
 * order its lanes visit the sub-quantisers (a fixed permutation that depends on n mod 16; csrc/adc_search.hip,
 * "conflict-free screen": every LDS gather of the byte tables is then bank-conflict-free whatever the codes).
 * rc_adc_scan_image_bytes(N, M): size of that image (0 = this M does not use one); rc_adc_scan_image converts rows
 * [n0, n0+n) (call it after appending rows — evaluate_repconc.py:89-98); rc_adc_search_img takes it (NULL = rebuild it
 * in the workspace on every call, which is what rc_adc_search does).  Results are identical with or without an image. */
size_t rc_adc_scan_image_bytes(int64_t N, int M);
/* layout introspection (host only, for tests): slot / phase-relative sub-quantiser read by `lane` in gather `step` */
int rc_adc_cf_describe(int M, int lane, int step, int* slot, int* m, int* slots_per_code, int* phases);
int rc_adc_scan_image(rc_handle_t h, const uint8_t* codes, int64_t n0, int64_t n, int M, uint8_t* image,
                      rc_stream_t stream);
/* Layouts.  The flat-search image (rc_adc_scan_image; rc_adc_scan_image_bytes(N, M) bytes, what rc_adc_search_img takes) is
 * row-major [N][M] for the one-phase M (16, 32, 48, 64) and, for M = 96, stored in tiles of 32768 rows, phase-major inside a
 * tile — [n / T][phase][n % T][48] — so each of the two screen passes streams dense 48-byte rows; the buffer holds whole
 * tiles, the position of a row does not depend on the buffer's capacity (rows can be appended).  The list-centric IVF search
 * (rc_ivf_search_lists / _probes) takes its own image for every M (rc_adc_scan_image_rows; layout below). */
int rc_adc_scan_image_rows(rc_handle_t h, const uint8_t* codes, int64_t n0, int64_t n, int M, uint8_t* image,
                           rc_stream_t stream);
/* The IVF image is blocked by chunks of 16 rows (round 3: a wave's load of one chunk and table phase is contiguous), so
 * its buffer holds whole chunks: rc_adc_scan_image_rows_bytes(N, M) bytes.  rc_adc_scan_image_rows_at (host only, no GPU)
 * = byte offset of codes[n][m] in it, -1 for arguments out of range: image[at(n, m)] == codes[n][m] is the whole contract. */
size_t rc_adc_scan_image_rows_bytes(int64_t N, int M);
int64_t rc_adc_scan_image_rows_at(int M, int64_t n, int m);
/* Round 6: the image of the 16-QUERY list-centric screen (rc_ivf_search_probes_q16).  Same blocking by chunks of 16 rows, but a
 * chunk holds [phase p16 = m / 16][lane = (n mod 16) + 16 g][step j] = codes[n][16 p16 + slot(lane, j)] — the order in which the
 * lanes of a ds_read_b128 gather visit the sub-quantisers (rc_adc_q16_describe), 4 bytes per lane and phase.
 * rc_adc_scan_image_rows16_bytes(N, M) bytes; rc_adc_scan_image_rows16_at = byte offset of codes[n][m] (host only). */
int rc_adc_scan_image_rows16(rc_handle_t h, const uint8_t* codes, int64_t n0, int64_t n, int M, uint8_t* image,
                             rc_stream_t stream);
size_t rc_adc_scan_image_rows16_bytes(int64_t N, int M);
int64_t rc_adc_scan_image_rows16_at(int M, int64_t n, int m);
/* Subset search over PQ codes: a SELECTION.  rows [ns] int64 on the device: rows of codes [N, M], strictly ascending, inside
 * [0, N) — the caller's word, never read on the host.  One kernel writes sel_codes [ns, M] = codes[rows] and sel_image = the
 * image of those ns rows in the layout asked for (0: rc_adc_scan_image's, 1: rc_adc_scan_image_rows', 2: _rows16's; the sizes
 * are the *_bytes helpers' for ns rows), byte for byte what the layout's own entry writes for a store that holds codes[rows], and
 * no other byte of the buffer.  Either output may be NULL; an M without an image (rc_adc_scan_image_bytes(1, M) == 0) takes
 * sel_image == NULL.  A subset search is then three calls: this one, any search entry over (sel_codes, sel_image, ns) with
 * id_offset 0, and rc_map_ids over its nq x k ids; the selection serves every later search of the same rows.
 * Checks, in this order: RC_ESHAPE (N > 2^32 - 1, M outside [1, 1024], layout outside 0 .. 2, an image asked for an M that has
 * none), RC_EINVAL for ns outside [1, N], RC_EINVAL for a missing handle, codes, rows or both outputs and — for an M with an
 * image — codes, sel_codes or sel_image off a 16-byte boundary; then device work.  No workspace. */
int rc_adc_select_rows(rc_handle_t h, const uint8_t* codes, int64_t N, int M, const int64_t* rows, int64_t ns, int layout,
                       uint8_t* sel_codes, uint8_t* sel_image, rc_stream_t stream);
/* ids[i] <- id_offset + rows[ids[i]] for the n entries with ids[i] >= 0; -1 (an unfilled slot) stays.  Checks: n < 0 is RC_ESHAPE,
 * then the pointers (RC_EINVAL); n == 0 succeeds without a launch. */
int rc_map_ids(rc_handle_t h, int64_t* ids, int64_t n, const int64_t* rows, int64_t id_offset, rc_stream_t stream);
/* Round 3: for the M whose flat search runs the 16-query screen (adc_screen_q16_kernel; M = 48 and 96 unless RC_ADC_Q16
 * says otherwise — read once per process) the flat-search image is [n / 32768][phase = m / 16][n % 32768][16 bytes], the 16
 * bytes of a (row, phase) ordered [lane quarter g][step j] = code of sub-quantiser 16 phase + slot(lane = (n & 15) + 16 g, j).
 * rc_adc_q16_describe (host only, tests): *slot = slot(lane, step); returns 1 if this M's flat search uses the layout, 0 if
 * not, RC_ESHAPE for an M without an image. */
int rc_adc_q16_describe(int M, int lane, int step, int* slot);
/* The 16-query screen has two block -> (query group, tile) maps; a search of nq queries (groups = ceil(nq / 16)) takes the
 * tile-dealt one (every XCD all groups and the tiles == x (mod 8)) when groups < 8 or groups <= RC_ADC_Q16_TILESPLIT_GROUPS
 * (environment, read on every call; default 64 / (M / 16)), else the group-dealt one (XCD x owns the groups == x (mod 8) and
 * walks every tile).  rc_adc_q16_by_tiles (host only, tests; the function the launch itself calls): 1 = tile-dealt, 0 =
 * group-dealt, RC_ESHAPE for an M without an image, RC_EINVAL for nq < 1. */
int rc_adc_q16_by_tiles(int M, int nq);
size_t rc_adc_search_img_ws_bytes(int64_t N, int M, int K, int nq, int k);
/* measurement: byte offsets, inside the workspace a search was given, of its per-query counts — unsigned[nq] rows that passed
 * the 8-bit screen (0: no screen at this size) and unsigned[nq] rows the exact rescoring kept */
int rc_adc_search_ws_counts(int64_t N, int M, int K, int nq, size_t* survivors_off, size_t* candidates_off);
int rc_adc_search_img(rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                      const float* C, int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                      float* scores, int64_t* ids, int* status, void* ws, size_t ws_bytes, rc_stream_t stream);
/* Search that cannot fail (evaluate_repconc.py:180-185: Faiss's IndexPQ.search returns for ANY index content).
 * rc_adc_search_q = rc_adc_search_img + qstatus: NULL, or nq ints zeroed by the caller that receive the status bits PER
 *   QUERY, so a caller repeats (other sel_slack) or re-routes only the queries concerned — one degenerate query does not
 *   tax the others of its batch.
 * rc_adc_search_exact: exact fp32 score of every row, the min(k, N) best by an 8-pass radix select over the 64-bit keys
 *   (ordered(score) << 32 | ~row), sorted (score desc, id asc).  No sample, no threshold, no status: terminates with the
 *   same answer as the fast path for any codes (all rows identical, k = N, ...).  Slower (N x 4 bytes of scores per query,
 *   ~10 passes): the route for the queries the fast path gives up on.  ws: rc_adc_search_exact_ws_bytes(N, M, K, nq, k). */
int rc_adc_search_q(rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                    const float* C, int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                    float* scores, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_adc_search_exact_ws_bytes(int64_t N, int M, int K, int nq, int k);
int rc_adc_search_exact(rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C, int D,
                        const float* q, int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                        size_t ws_bytes, rc_stream_t stream);
/* the look-up tables alone (test hook): lut [nq,M,K] fp32 */
int rc_adc_lut(rc_handle_t h, const float* C, const float* q, int nq, int D, int M, int K,
               float* lut, rc_stream_t stream);
/* L2 metric (faiss.IndexPQ(d, M, 8, METRIC_L2)).  Bit-defined like the inner-product search:
 *   sub-distance T[m][c] = fp32 chain acc = +0.0f; for j = 0 .. dsub-1 ascending: t = q[m dsub + j] - C[m][c][j] (one fp32
 *     subtraction), acc = acc + t * t (product and sum each rounded, no FMA: Faiss's scalar fvec_L2sqr);
 *   distance d(q, n) = fp32 sum over m ascending of T[m][code[n][m]];
 *   output: d ascending, ties by the lower id; a zero distance is +0.0f; +inf / -1 in the slots past N.
 * The pipeline runs unchanged on s = -d: rc_adc_lut_l2 (arguments of rc_adc_lut) writes S[m][c] = 0.0f - T[m][c] — -T for T > 0,
 * +0.0f for T = 0, so no entry is -0.0f — and a table is all a screen, a rescorer, a select or an IVF entry ever sees; the IVF
 * entries of an L2 index take this table and their caller forms d = 0.0f - s.  rc_adc_search_l2_q / rc_adc_search_l2_exact: the
 * arguments, workspaces, status bits and routes of rc_adc_search_q / rc_adc_search_exact with that table and one trailing kernel
 * that replaces each of the nq * k scores by 0.0f - s.  Precondition: finite inputs and every T finite (documented, not tested). */
int rc_adc_lut_l2(rc_handle_t h, const float* C, const float* q, int nq, int D, int M, int K,
                  float* lut, rc_stream_t stream);
int rc_adc_search_l2_q(rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                       const float* C, int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                       float* scores, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_adc_search_l2_exact(rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C, int D,
                           const float* q, int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                           size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ dense flat search
 * Exact inner-product top-k over an fp32 corpus: the GPU faiss.IndexFlatIP (useFloat16 = False) of
 * models/dense/evaluate_dense.py:84-129 (create_index, dense_search, batch_dense_search).
 * Score s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f, s = fmaf(q[d], x[n][d], s) (the fp32 matrix cores
 * compute exactly this), so ids AND score bits are defined; the min(k, N) best rows sorted (score desc, row asc),
 * ids = row + id_offset, -inf / -1 in the slots past N.
 * x: [N, ldx] fp32, ldx >= D; q: [nq, D] fp32 contiguous; scores [nq, k] fp32, ids [nq, k] int64.  Any D >= 1 (D % 16 == 0
 * is the fast path; then x and q must be 16-byte aligned and ldx % 4 == 0, else RC_EINVAL); N < 2^32 and 1 <= k <= 8192,
 * else RC_ESHAPE — both before anything is enqueued.  Finite inputs are assumed.
 * rc_dense_search_q: N <= 131072 takes the exact route below.  Above, the sampled-threshold route of rc_adc_search_q: the
 *   r-th best of 32768 exactly scored strided sample rows is the per-query threshold (r and sel_slack as at rc_adc_search;
 *   the Python wrapper passes 3), a GEMM over the whole corpus appends every row scoring >= it to the query's candidate
 *   list, the lists are sorted.  status (device int) / qstatus (nq device ints, may be NULL), both zeroed by the caller, get
 *   bit0 for a query that collected fewer than min(k, N) candidates and bit1 for one whose list overflowed (16384): repeat
 *   those queries with another sel_slack or answer them by rc_dense_search_exact.  ws: rc_dense_search_ws_bytes(N, D, nq, k).
 * rc_dense_search_exact: full score rows of a chunk of queries, then the 8-pass radix select of rc_adc_search_exact over the
 *   64-bit keys.  No status: terminates with the same answer for any content (all rows identical, k >= N, ...).
 *   ws: rc_dense_search_exact_ws_bytes(N, D, nq, k) (at most 256 MiB of score rows plus 128 KiB per query of a chunk). */
size_t rc_dense_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                      int64_t id_offset, double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus,
                      void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_search_exact_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_search_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                          int64_t id_offset, float* scores, int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ dense flat search, fp16 storage
 * The same search over a corpus stored as IEEE fp16 (faiss GpuClonerOptions.useFloat16): x [N, ldx] and q [nq, D] are fp16
 * bit patterns (uint16_t), finite.  Score s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f over the widened
 * values, s = fmaf((float)q[d], (float)x[n][d], s): ids AND score bits equal rc_dense_search_q on the widened arrays.
 * Order, padding (-inf / -1), id_offset and the limits (N < 2^32, 1 <= k <= 8192, else RC_ESHAPE) as above.  Any D >= 1;
 * D % 16 == 0 requires x and q 16-byte aligned and ldx % 8 == 0 (else RC_EINVAL); the f16 screen reads rows with 16-byte loads
 * when D % 8 == 0, ldx % 8 == 0 and both pointers are 16-byte aligned, element by element otherwise.
 * rc_dense_f16_search_q: N <= 131072 takes the exact route below.  Above: the f16 matrix cores compute approximate scores s~
 *   (their summation order is not the chain's); the r-th best s~ of 32768 strided sample rows is the threshold thr~ (r and
 *   sel_slack as at rc_adc_search), every row with s~ >= thr~ becomes a candidate, the candidates are rescored by the chain
 *   and sorted.  xnorm_max: DEVICE pointer to one float X >= the largest Euclidean row norm of x (read on the stream, no host
 *   synchronisation).  With E_q = 4 * D_pad * 2^-24 * ||q||_2 * X (D_pad = D rounded up to 16; every |s~ - s| <= E_q) and t =
 *   the query's k-th exact score, t >= thr~ + E_q, all rounded upwards, proves that no row outside the list can reach the
 *   top-k or tie with its last member.  status (device int) / qstatus (nq device ints, may be NULL), both zeroed by the caller:
 *   bit0 = fewer than min(k, N) candidates, bit1 = the list overflowed (16384), bit2 = not certified (t < thr~ + E_q): repeat
 *   those queries with another sel_slack or answer them by rc_dense_f16_search_exact.  ws: rc_dense_f16_search_ws_bytes.
 * rc_dense_f16_search_exact: full score rows from the fp32 matrix cores over rows widened on load (the chain itself), then the
 *   radix select; no status.  ws: rc_dense_f16_search_exact_ws_bytes(N, D, nq, k).
 * rc_dense_f16_scores (test hook): the screen's raw s~, out [nq][N] fp32.
 * rc_dense_f16_error_constant: the factor 4 of E_q as the certificate kernel was compiled with it (no GPU needed).
 * rc_dense_f16_screen_form: 16, the screen runs on v_mfma_f32_16x16x32_f16 (32 named the retired v_mfma_f32_32x32x16_f16 form). */
size_t rc_dense_f16_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_f16_search_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                          const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores, int64_t* ids,
                          int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_f16_search_exact_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_f16_search_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq, int k,
                              int64_t id_offset, float* scores, int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_f16_scores(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq, float* out,
                        rc_stream_t stream);
double rc_dense_f16_error_constant(void);
int rc_dense_f16_screen_form(void);

/* ------------------------------------------------------------------ dense flat search, fp32 corpus, bf16x3 screen
 * rc_dense_search_q's arguments, limits and RESULTS (ids and score bits) for finite x and q whose bf16 rounding is finite
 * (|v| < 2^128 - 2^119); x is not checked, a query outside the range is never certified.  Only the screen differs: every
 * operand is split a = a_h + a_l + r, a_h = bf16(a), a_l = bf16(a - a_h), round to nearest even, and the bf16 matrix cores
 * compute s~ = sum_d (q_h x_h + q_h x_l + q_l x_h).  The corpus is split as it is staged, the queries once per call.
 * rc_dense_bf16x3_search_q: N <= 131072 takes the route of rc_dense_search_exact.  Above: threshold thr~ from the s~ of 32768
 *   strided sample rows, every row with s~ >= thr~ a candidate, candidates rescored by the chain and sorted.  xnorm_max: DEVICE
 *   pointer to one float X >= the largest Euclidean row norm of x.  With D_pad = D rounded up to 16 and the constants c[0..3] of
 *   rc_dense_bf16x3_error_constants,
 *     E_q = (c0 D_pad 2^-24 + c1 2^-16) ||q||_2 X + c2 sqrt(D_pad) (||q||_2 + X) + c3 D_pad      (every |s~ - s| <= E_q),
 *   t >= thr~ + E_q for t = the query's k-th exact score proves the answer.  status / qstatus as rc_dense_f16_search_q: bit0,
 *   bit1, bit2 = not certified (also: a non-finite value anywhere, a query value that rounds to inf, D > 65536): repeat those
 *   queries with another sel_slack or answer them by rc_dense_search_exact.  ws (16-byte aligned): rc_dense_bf16x3_search_ws_bytes.
 * rc_dense_bf16x3_scores (test hook): the screen's raw s~, out [nq][N] fp32; ws: rc_dense_bf16x3_scores_ws_bytes(D, nq).
 * rc_dense_bf16x3_error_constants: c[4] = {8, 4, 2^-133, 4 * 2^-149} as the certificate kernel was compiled (no GPU needed). */
size_t rc_dense_bf16x3_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_bf16x3_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                             const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores, int64_t* ids,
                             int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_bf16x3_scores_ws_bytes(int D, int nq);
int rc_dense_bf16x3_scores(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, float* out,
                           void* ws, size_t ws_bytes, rc_stream_t stream);
void rc_dense_bf16x3_error_constants(double* c);

/* ------------------------------------------------------------------ dense flat search, 8-bit scalar-quantised storage
 * The same search over a corpus of 8-bit scalar-quantiser codes (faiss.IndexScalarQuantizer, QT_8bit): x [N, ldx] int8 holds
 * c' = c - 128 for the code c in 0 .. 255 of every dimension; dec [2][D] fp32 = step (row 0) and mid (row 1); q [nq, D] fp32,
 * finite.  A row decodes to x^[d] = fmaf((float)c'[d], step[d], mid[d]) and the score is s(q, n) = fp32 fmaf chain over
 * d = 0 .. D-1 ascending from +0.0f of q[d] * x^[n][d]: ids AND score bits equal rc_dense_search_q over the decoded corpus
 * (rc_dense_sq8_decode).  Order, padding (-inf / -1), id_offset and the limits (N < 2^32, 1 <= k <= 8192, else RC_ESHAPE) as
 * above; 1 <= D <= 65536 (else RC_ESHAPE: the screen's int32 accumulators hold 128 * 128 * D).  Any row pitch ldx >= D and
 * any alignment: rows are read with 16-byte loads when D % 16 == 0, ldx % 16 == 0 and x is 16-byte aligned, byte by byte
 * otherwise.
 * rc_dense_sq8_search_q: N <= 131072 takes the exact route below.  Above: a pre-pass turns every query into w[d] = q[d] step[d],
 *   bias = sum_d q[d] mid[d] (fp64, rounded once), alpha = max_d |w[d]| / 32639 and two int8 planes h, l with
 *   rint(w[d] / alpha) = 256 h[d] + l[d]; the int8 matrix cores accumulate A_h = sum_d h[d] c'[d], A_l = sum_d l[d] c'[d] in
 *   exact int32 and s~ = fmaf(alpha, fmaf(256, A_h, A_l), bias).  Threshold, candidates, rescoring by the chain and the sort as
 *   rc_dense_f16_search_q.  cstat: DEVICE pointer to two floats, C1 >= the largest sum_d |c'[d]| of a row and X >= the largest
 *   Euclidean norm of a decoded row.  With W1 = sum_d |w[d]|, B1 = sum_d |q[d] mid[d]|, u = 2^-24, D_pad = D rounded up to 16
 *   and the constants c[0..6] of rc_dense_sq8_error_constants,
 *     E_q = (c0 alpha C1 + u (c1 W1 + c2 alpha D + c3 alpha C1 + c4 B1 + c5 (D_pad + 1) ||q||_2 X)
 *            + c6 2^-149 (D_pad + sqrt(D_pad) ||q||_2 + C1 + 1)) (1 + 2^-20)                  (every |s~ - s| <= E_q),
 *   t >= thr~ + E_q for t = the query's k-th exact score proves the answer.  status / qstatus as rc_dense_f16_search_q: bit0,
 *   bit1, bit2 = not certified (also: a query value, w[d] or |q[d] mid[d]| not below 2^100, a NaN anywhere, alpha below 2^-100
 *   with a nonzero w): repeat those queries with another sel_slack or answer them by rc_dense_sq8_search_exact.
 *   ws (16-byte aligned): rc_dense_sq8_search_ws_bytes.
 * rc_dense_sq8_search_exact: the chain of every (query, row) pair over rows decoded on the fly, then the radix select; no
 *   status.  ws: rc_dense_sq8_search_exact_ws_bytes(N, D, nq, k).
 * rc_dense_sq8_search_ws_counts (measurement): *cnt_off = the byte offset in the workspace of rc_dense_sq8_search_q where, after
 *   the call, nq unsigned ints hold the rows of every query that passed the screen (more than 16384: the list overflowed); 0
 *   where the exact route answers (N <= 131072).  No GPU needed.
 * rc_dense_sq8_scores (test hook): the screen's raw s~, out [nq][N] fp32; ws: rc_dense_sq8_scores_ws_bytes(D, nq).
 * rc_dense_sq8_decode: out [N][D] fp32 = the decoded rows (N = 0: nothing).
 * rc_dense_sq8_error_constants: c[7] = {0.5, 520, 194, 515, 2.1, 1.02, 1}; rc_dense_sq8_qmax: 32639 = 127 * 256 + 127, the
 *   largest |256 h + l|; rc_dense_sq8_max_d: 65536 (none needs a GPU). */
size_t rc_dense_sq8_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_sq8_search_q(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                          const float* dec, const float* cstat, int k, int64_t id_offset, double sel_slack, float* scores,
                          int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_sq8_search_exact_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_sq8_search_exact(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                              const float* dec, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                              size_t ws_bytes, rc_stream_t stream);
int rc_dense_sq8_search_ws_counts(int64_t N, int D, int nq, int k, size_t* cnt_off);
size_t rc_dense_sq8_scores_ws_bytes(int D, int nq);
int rc_dense_sq8_scores(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq, const float* dec,
                        float* out, void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_sq8_decode(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* dec, float* out,
                        rc_stream_t stream);
void rc_dense_sq8_error_constants(double* c);
int rc_dense_sq8_qmax(void);
int rc_dense_sq8_max_d(void);

/* ------------------------------------------------------------------ dense flat search, L2 metric
 * Exact squared-Euclidean top-k over an fp32 corpus: faiss.IndexFlatL2, the flat index the reference names at
 * models/repconc/evaluate_repconc.py:102 and train/run_warmup.py:102,107.  Arguments, alignment rules and limits of
 * rc_dense_search_q (any D >= 1, N < 2^32, 1 <= k <= 8192 else RC_ESHAPE, finite inputs).
 * Distance d(q, n) = the fp32 chain acc = +0.0f; for j = 0 .. D-1 ascending: t = q[j] - x[n][j] (one fp32 subtraction),
 * acc = fmaf(t, t, acc) — the direct form, so ids AND distance bits are defined.  dist [nq, k]: the min(k, N) nearest rows
 * sorted (distance asc, row asc), every value >= +0.0f, ids = row + id_offset, +inf / -1 in the slots past N.  A distance that
 * overflows is +inf and sorts last.
 * rc_dense_l2_search_q (evaluate_repconc.py:102, run_warmup.py:102,107): N <= 131072 takes the exact route below.  Above: the
 *   fp32 matrix cores screen with sigma = fmaf(2, dot(q, x_n), -xsq[n]) = ||q||^2 - d up to rounding; the r-th best sigma of
 *   32768 strided sample rows is the threshold thr~ (r and sel_slack as at rc_adc_search), every row with sigma >= thr~ becomes a
 *   candidate, the candidates are rescored by the chain and sorted.  xsq: DEVICE fp32 [N], the squared norm of every row (an
 *   fp64 sum rounded to nearest); xnorm_max: DEVICE pointer to one float X >= the largest Euclidean row norm; NULL for either
 *   is RC_EINVAL.  With D_pad = D rounded up to 16 and the constants c[0..2] of rc_dense_l2_error_constants,
 *     E_q = c0 D_pad 2^-24 (||q||_2 + X)^2 + c1 sqrt(D_pad) (||q||_2 + X) + c2 D_pad   (every |sigma - ||q||^2 + d| <= E_q),
 *   -t >= thr~ - ||q||^2 + E_q for t = the query's k-th distance, all rounded to the safe side, proves that no row outside the
 *   list can reach the top-k or tie with its last member.  status (device int) / qstatus (nq device ints, may be NULL), both
 *   zeroed by the caller: bit0 = fewer than min(k, N) candidates, bit1 = the list overflowed (16384), bit2 = not certified
 *   (also: a non-finite query value, D > 65536, (||q||_2 + X)^2 >= 2^126): repeat those queries with another sel_slack or
 *   answer them by rc_dense_l2_search_exact.  ws: rc_dense_l2_search_ws_bytes(N, D, nq, k).
 * rc_dense_l2_search_exact (the same references): a vector-ALU kernel writes the full rows of -d of a chunk of queries, then the
 *   radix select of rc_dense_search_exact; takes no norms, no status, terminates with the same answer for any content.
 *   ws: rc_dense_l2_search_exact_ws_bytes(N, D, nq, k).
 * rc_dense_l2_scores (test hook): the screen's raw sigma, out [nq][N] fp32.
 * rc_dense_l2_error_constants: c[3] = {2, 4 * 2^-126, 4 * 2^-149} as the certificate kernel was compiled (no GPU needed). */
size_t rc_dense_l2_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, const float* xsq,
                         const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* dist, int64_t* ids,
                         int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_l2_search_exact_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_search_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                             int64_t id_offset, float* dist, int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_l2_scores(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, const float* xsq,
                       float* out, rc_stream_t stream);
void rc_dense_l2_error_constants(double* c);

/* ------------------------------------------------------------------ dense flat search, L2 metric, fp16 storage
 * The L2 search over a corpus stored as IEEE fp16 (faiss.IndexFlatL2 with useFloat16): x [N, ldx] and q [nq, D] are fp16 bit
 * patterns (uint16_t), finite.  Distance d(q, n) = the chain above over the widened values, t = (float)q[j] - (float)x[n][j],
 * acc = fmaf(t, t, acc): ids AND distance bits equal rc_dense_l2_search_q on the widened arrays.  Order, padding (+inf / -1),
 * id_offset and the limits (any D >= 1, N < 2^32, 1 <= k <= 8192, else RC_ESHAPE) as there; alignment rules of
 * rc_dense_f16_search_q (D % 16 == 0 requires x and q 16-byte aligned and ldx % 8 == 0, else RC_EINVAL; rows are read with
 * 16-byte loads when D % 8 == 0, ldx % 8 == 0 and both pointers are 16-byte aligned, element by element otherwise).
 * rc_dense_l2_f16_search_q: N <= 131072 takes the exact route below.  Above: the f16 matrix cores screen with sigma =
 *   fmaf(2, dot(q, x_n), -xsq[n]); threshold, candidates, rescoring by the chain and sorting as rc_dense_l2_search_q.  xsq:
 *   DEVICE fp32 [N], the squared norm of every stored (rounded) row, an fp64 sum rounded to nearest; xnorm_max: DEVICE pointer
 *   to one float X >= the largest Euclidean row norm; NULL for either is RC_EINVAL.  With D_pad = D rounded up to 16 and c[0] of
 *   rc_dense_l2_f16_error_constants,
 *     E_q = c0 D_pad 2^-24 (||q||_2 + X)^2                                        (every |sigma - ||q||^2 + d| <= E_q),
 *   -t >= thr~ - ||q||^2 + E_q for t = the query's k-th distance, all rounded to the safe side, proves the answer.  status /
 *   qstatus as rc_dense_l2_search_q: bit0, bit1, bit2 = not certified (also: a non-finite query value, D > 65536): repeat those
 *   queries with another sel_slack or answer them by rc_dense_l2_f16_search_exact.  ws: rc_dense_l2_f16_search_ws_bytes.
 * rc_dense_l2_f16_search_exact: the vector-ALU kernel of rc_dense_l2_search_exact over rows widened on load, then the radix
 *   select; takes no norms, no status.  ws: rc_dense_l2_f16_search_exact_ws_bytes(N, D, nq, k).
 * rc_dense_l2_f16_scores (test hook): the screen's raw sigma, out [nq][N] fp32.
 * rc_dense_l2_f16_error_constants: c[2] = {2.5, 65536}: the factor of E_q as the certificate kernel was compiled with it and
 *   the largest D it is proven for (no GPU needed). */
size_t rc_dense_l2_f16_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_f16_search_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                             const float* xsq, const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* dist,
                             int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_l2_f16_search_exact_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_f16_search_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                 int k, int64_t id_offset, float* dist, int64_t* ids, void* ws, size_t ws_bytes,
                                 rc_stream_t stream);
int rc_dense_l2_f16_scores(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                           const float* xsq, float* out, rc_stream_t stream);
void rc_dense_l2_f16_error_constants(double* c);

/* ------------------------------------------------------------------ dense flat search over a subset of the rows
 * The four searches above (fp32 and fp16 storage, inner product and L2) over the rows `rows` of the store, in place: no copy of
 * the rows is made and the cost follows ns, not N.  rows: DEVICE int64 [ns], corpus rows in ASCENDING order, no row twice,
 * every one in [0, N).  THE LIBRARY DOES NOT VERIFY THIS: rows is never read on the host, and a row outside [0, N) is a read
 * outside x (the Python wrapper checks the list unless told not to, ops.dense_search(rows=..., check_rows=True)).
 * Result: exactly what the entry of the same name without _rows returns over the matrix x[rows] (and xsq[rows]) of ns rows,
 * with every id i replaced by id_offset + rows[i] — ids and score / distance bits, the padding (-inf or +inf, -1) past ns
 * included; among equal scores the lower corpus row comes first because rows ascends.  Everything that follows the row count
 * follows ns: rc_dense*_search_rows_q takes the exact route for ns <= 131072, the sample is min(ns, 32768) rows of the subset,
 * and the workspace is that of the entry without _rows called with ns: rc_dense*_search_ws_bytes(ns, D, nq, k),
 * rc_dense*_search_exact_ws_bytes(ns, D, nq, k).  status / qstatus, sel_slack and the certificate as there; xnorm_max bounds the
 * row norms of ALL of x (a bound over a superset of the subset) and xsq is the [N] array of the whole store, read at rows[i].
 * Arguments: those of the entry without _rows with `rows, ns` inserted after the side operands (xsq, xnorm_max) and before the
 * scalars (k, ...): h, x, ldx, N, D, q, nq, [xsq], [xnorm_max], rows, ns, k, id_offset, ...
 * Checks, in this order: the shapes (N < 2^32 and k <= 8192 else RC_ESHAPE; 1 <= ns <= N and the other limits else RC_EINVAL),
 * the pointers (rows NULL is RC_EINVAL), nq == 0 (RC_OK, nothing enqueued), the workspace (RC_EWORKSPACE), then device work.
 * The bf16x3 screens and the int8 stores have no such entry. */
int rc_dense_search_rows_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                           const int64_t* rows, int64_t ns, int k, int64_t id_offset, double sel_slack, float* scores,
                           int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_search_rows_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                               const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                               size_t ws_bytes, rc_stream_t stream);
int rc_dense_f16_search_rows_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                               const float* xnorm_max, const int64_t* rows, int64_t ns, int k, int64_t id_offset,
                               double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus, void* ws,
                               size_t ws_bytes, rc_stream_t stream);
int rc_dense_f16_search_rows_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                   const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* scores, int64_t* ids,
                                   void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_l2_search_rows_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                              const float* xsq, const float* xnorm_max, const int64_t* rows, int64_t ns, int k,
                              int64_t id_offset, double sel_slack, float* dist, int64_t* ids, int* status, int* qstatus,
                              void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_l2_search_rows_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                  const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* dist, int64_t* ids, void* ws,
                                  size_t ws_bytes, rc_stream_t stream);
int rc_dense_l2_f16_search_rows_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                  const float* xsq, const float* xnorm_max, const int64_t* rows, int64_t ns, int k,
                                  int64_t id_offset, double sel_slack, float* dist, int64_t* ids, int* status, int* qstatus,
                                  void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_l2_f16_search_rows_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                      const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* dist, int64_t* ids,
                                      void* ws, size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ dense flat search, L2 metric, fp32 corpus, bf16x3 screen
 * rc_dense_l2_search_q with the screen on the bf16 matrix cores: the corpus stays fp32 and ids AND distance bits are those of
 * rc_dense_l2_search_q (the chain t = q[j] - x[n][j], acc = fmaf(t, t, acc); distance asc, row asc; +0.0f for a zero;
 * +inf / -1 past min(k, N)).  Arguments, alignment rules and limits of rc_dense_l2_search_q; the corpus must round to finite
 * bf16 (every |x| < 2^128 - 2^119).
 * rc_dense_l2_bf16x3_search_q: N <= 131072 takes the route of rc_dense_l2_search_exact.  Above: the screen is sigma~ =
 *   fmaf(2, s~(q, x_n), -xsq[n]) with s~ the three-product bf16 split sum of rc_dense_bf16x3_search_q; threshold, candidates,
 *   rescoring by the chain and sorting as rc_dense_l2_search_q.  xsq: DEVICE fp32 [N], the squared norm of every row (an fp64
 *   sum rounded to nearest); xnorm_max: DEVICE pointer to one float X >= the largest Euclidean row norm; NULL for either is
 *   RC_EINVAL.  With D_pad = D rounded up to 16, R = (||q||_2 + X)^2 and the constants c[0..3] of
 *   rc_dense_l2_bf16x3_error_constants,
 *     E_q = (c0 D_pad 2^-24 + c1 2^-16) R + c2 sqrt(D_pad) (||q||_2 + X) + c3 D_pad   (every |sigma~ - ||q||^2 + d| <= E_q),
 *   -t >= thr~ - ||q||^2 + E_q for t = the query's k-th distance, all rounded to the safe side, proves the answer.  status /
 *   qstatus as rc_dense_l2_search_q: bit0, bit1, bit2 = not certified (also: a query value that is not finite or whose bf16
 *   rounding is not, D > 65536, R >= 2^126): repeat those queries with another sel_slack or answer them by
 *   rc_dense_l2_search_exact; there is no exact entry of its own.  ws (16-byte aligned, it holds the queries' bf16 planes):
 *   rc_dense_l2_bf16x3_search_ws_bytes(N, D, nq, k).
 * rc_dense_l2_bf16x3_scores (test hook): the screen's raw sigma~, out [nq][N] fp32; ws (16-byte aligned):
 *   rc_dense_l2_bf16x3_scores_ws_bytes(D, nq).
 * rc_dense_l2_bf16x3_error_constants: c[4] = {5, 2, 4 * 2^-126, 8 * 2^-149} as the certificate kernel was compiled (no GPU
 *   needed). */
size_t rc_dense_l2_bf16x3_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_bf16x3_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                const float* xsq, const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* dist,
                                int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);
size_t rc_dense_l2_bf16x3_scores_ws_bytes(int D, int nq);
int rc_dense_l2_bf16x3_scores(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                              const float* xsq, float* out, void* ws, size_t ws_bytes, rc_stream_t stream);
void rc_dense_l2_bf16x3_error_constants(double* c);

/* ------------------------------------------------------------------ dense flat search, L2 metric, 8-bit scalar-quantised storage
 * rc_dense_l2_search_q over the store of rc_dense_sq8_search_q (faiss.IndexScalarQuantizer, QT_8bit, METRIC_L2): x [N, ldx]
 * int8 = c - 128, dec [2][D] = step, mid, q [nq, D] fp32, finite.  Distance d(q, n) = the chain of rc_dense_l2_search_q over
 * the decoded row x^[d] = fmaf((float)c'[d], step[d], mid[d]): ids AND distance bits equal rc_dense_l2_search_q over the
 * decoded corpus (rc_dense_sq8_decode).  dist ascending, lower id first among equals, +0.0f for a zero, +inf / -1 past N.
 * Limits, row pitch and alignment as rc_dense_sq8_search_q (1 <= D <= 65536, N < 2^32, 1 <= k <= 8192, else RC_ESHAPE).
 * rc_dense_l2_sq8_search_q: N <= 131072 takes the exact route below.  Above: the pre-pass and the int8 screen s~ of
 *   rc_dense_sq8_search_q, then sigma = fmaf(2, s~, -xsq[n]); xsq: DEVICE fp32 [N], the squared norm of every decoded row, an
 *   fp64 sum rounded to nearest (rc_dense_sq8_row_sqnorms); cstat as rc_dense_sq8_search_q.  With its W1, B1, alpha, C1, X, u,
 *   D_pad, R = (||q||_2 + X)^2 and the constants c[0..8] of rc_dense_l2_sq8_error_constants,
 *     E_q = (c0 alpha C1 + u (c1 W1 + c2 alpha D + c3 alpha C1 + c4 B1 + c5 (D_pad + 5) R)
 *            + c6 2^-149 (D_pad + sqrt(D_pad) ||q||_2 + C1 + 3)) (1 + 2^-20)        (every |sigma - ||q||^2 + d| <= E_q),
 *   +inf unless R < c7 and E_q < c8; -d_k >= thr~ - ||q||^2 + E_q for the query's k-th distance d_k proves the answer.
 *   status / qstatus, the refusals and ws (16-byte aligned, rc_dense_l2_sq8_search_ws_bytes) as rc_dense_sq8_search_q; bit2:
 *   repeat with another sel_slack or answer by rc_dense_l2_sq8_search_exact.
 * rc_dense_l2_sq8_search_exact: the chain of every (query, row) pair over rows decoded on the fly, then the radix select; no
 *   status, no norms.  ws: rc_dense_l2_sq8_search_exact_ws_bytes(N, D, nq, k).
 * rc_dense_l2_sq8_search_ws_counts (measurement): as rc_dense_sq8_search_ws_counts.
 * rc_dense_l2_sq8_scores (test hook): the screen's raw sigma, out [nq][N] fp32; ws: rc_dense_l2_sq8_scores_ws_bytes(D, nq).
 * rc_dense_sq8_row_sqnorms: out [N] fp32 = the squared norms of the decoded rows, computed from the codes (N = 0: nothing).
 * rc_dense_l2_sq8_error_constants: c[9] = {1, 1040, 388, 1030, 4.2, 1.01, 1, 2^126, 2^124} (no GPU needed). */
size_t rc_dense_l2_sq8_search_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_sq8_search_q(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                             const float* dec, const float* xsq, const float* cstat, int k, int64_t id_offset, double sel_slack,
                             float* dist, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                             rc_stream_t stream);
size_t rc_dense_l2_sq8_search_exact_ws_bytes(int64_t N, int D, int nq, int k);
int rc_dense_l2_sq8_search_exact(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                 const float* dec, int k, int64_t id_offset, float* dist, int64_t* ids, void* ws,
                                 size_t ws_bytes, rc_stream_t stream);
int rc_dense_l2_sq8_search_ws_counts(int64_t N, int D, int nq, int k, size_t* cnt_off);
size_t rc_dense_l2_sq8_scores_ws_bytes(int D, int nq);
int rc_dense_l2_sq8_scores(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                           const float* dec, const float* xsq, float* out, void* ws, size_t ws_bytes, rc_stream_t stream);
int rc_dense_sq8_row_sqnorms(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* dec, float* out,
                             rc_stream_t stream);
void rc_dense_l2_sq8_error_constants(double* c);

/* ------------------------------------------------------------------ dense stores: exact re-ranking of candidate lists
 * The second stage of faiss.IndexRefineFlat: cand [nq, ldc] int64 holds kc candidate ids per query (from a PQ or IVF search),
 * x [N, ldx] is the dense store (fp32; rc_dense_f16_rerank: fp16 bit patterns, x and q both), q [nq, D] the queries.  Only the
 * candidates' rows are read: nq * kc rows instead of nq * N.
 * metric: 0 = inner product, 1 = squared L2; anything else is RC_ESHAPE before any launch.
 * Limits: 1 <= k <= 8192, 1 <= kc <= 16384, N < 2^32 (else RC_ESHAPE); any D >= 1, any row pitch ldx >= D, any ldc >= kc,
 *   finite inputs, one device.  nq == 0 returns RC_OK and touches nothing; N == 0 pads every output slot.  Rows are staged with
 *   16-byte loads when x is 16-byte aligned and the pitch is a multiple of 16 bytes, read element by element otherwise.
 * Valid candidates: candidate c of query i is valid iff 0 <= c - id_offset < N.  Everything else is skipped silently: the -1
 *   holes of an IVF search, ids outside the store.  A list is a multiset: an id given twice is scored twice and may appear
 *   twice in the output.
 * Score of a valid candidate: bit for bit what rc_dense_search_exact / rc_dense_l2_search_exact (rc_dense_f16_search_exact /
 *   rc_dense_l2_f16_search_exact) produce for that (query, row): one fp32 accumulator from +0.0f, d ascending, over the values
 *   widened to fp32; inner product s = fmaf(q[d], x[n][d], s); L2 t = q[d] - x[n][d], s = fmaf(t, t, s).
 * Output scores / ids [nq, k]: the min(k, valid_i) best by the 64-bit key of the searches, then padding.  Inner product: score
 *   descending, ties by the lower id, padding (-inf, -1).  L2: distance ascending, ties by the lower id, padding (+inf, -1);
 *   a zero distance is +0.0f, an overflowed distance is +inf and sorts last, ahead of the padding.  Ids are emitted as given,
 *   id_offset included.
 * Runs on `stream`; no host synchronisation, no atomics on values, results bit-identical from run to run.
 * ws: rc_dense_rerank_ws_bytes(nq, kc), a multiple of 256 (128 KiB of keys per query); 0 for nq <= 0 or kc outside [1, 16384]. */
size_t rc_dense_rerank_ws_bytes(int nq, int kc);
int rc_dense_rerank(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, const int64_t* cand,
                    int64_t ldc, int kc, int k, int64_t id_offset, int metric, float* scores, int64_t* ids, void* ws,
                    size_t ws_bytes, rc_stream_t stream);
int rc_dense_f16_rerank(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                        const int64_t* cand, int64_t ldc, int kc, int k, int64_t id_offset, int metric, float* scores,
                        int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ a-9 … a-11, stateful form
 * The index object the reference keeps inside Faiss (initialize_index / add_docs / index.search,
 * models/repconc/evaluate_repconc.py:78-98,182; JPQ's per-step synchronize_model_index, models/jpq/finetune_jpq.py:209-214),
 * with the device memory owned by the library: codes [ntotal, M] uint8 in one allocation whose capacity doubles,
 * the centroid table [M,256,D/M] (set_centroids rewrites it in place: 786 KB per JPQ step instead of re-cloning the
 * index), and the search workspace.  All pointers are device pointers.  rc_index_search is synchronous: it loops over
 * rc_adc_search until the status word is clean (RC_ESELECT after 4 attempts).  Empty index: -inf scores, -1 ids.
 * One index per handle/device; not thread-safe. */
int rc_index_create(rc_handle_t h, int D, int M, int K, rc_index_t* out);
int rc_index_destroy(rc_index_t idx);
int rc_index_set_centroids(rc_index_t idx, const float* C, rc_stream_t stream);
int rc_index_reserve(rc_index_t idx, int64_t rows, rc_stream_t stream);
int rc_index_add_codes(rc_index_t idx, const uint8_t* codes, int64_t n, rc_stream_t stream);
int rc_index_reset(rc_index_t idx);
/* metric of rc_index_search: 0 inner product (the default), 1 L2 (distances ascending; empty index: +inf / -1); any other
 * value is RC_EINVAL.  The index keeps nothing that depends on the metric, so it may be set at any time between searches. */
int rc_index_set_metric(rc_index_t idx, int metric);
int64_t rc_index_ntotal(rc_index_t idx);
const uint8_t* rc_index_codes(rc_index_t idx);
const float* rc_index_centroids(rc_index_t idx);
int rc_index_search(rc_index_t idx, const float* q, int nq, int k, float* scores, int64_t* ids,
                    rc_stream_t stream);

/* ------------------------------------------------------------------ IVF extension (SURVEY §8d input D)
 * The reference only ever builds a 1-list IVFPQ (evaluate_repconc.py:101-118); BASELINE.json's nlist=5000 config is a
 * build-side extension.  Code rows are stored list-major (`codes` [N,M] sorted by coarse cell, `list_off` [nlist+1]
 * row offsets, `ids` [N] corpus position of every row), NOT residual-encoded.  For query qi the rows of lists
 * probes[qi, 0..nprobe) are scored exactly (same fp32 m-ascending sum as rc_adc_search) and the top-k returned with
 * the same order (score desc, id asc); probing every list gives exactly the flat result.
 * lut: [nq,M,256] from rc_adc_lut; base[qi,p] = rows scanned before probe p; count[qi] = rows scanned in total;
 * stride >= max count.  ids -1 / score -inf pad queries whose probed lists hold fewer than k rows.
 * ws: rc_ivf_search_ws_bytes(nq, stride).  status bit1: more than 16384 rows tie at the k-th score. */
/* Build side: cell[b] = argmin_l ||x_b - cent_l||^2 (first minimum) for nlist coarse centroids of the full dimension D,
 * evaluated as ||c||^2 - 2<x,c> on the fp32 matrix cores with the argmin fused in (the [B, nlist] score matrix is never
 * written).  x: [B, ldx >= D] fp32, 16-byte aligned rows, ldx % 4 == 0, D % 16 == 0; cent: [nlist, D], 16-byte aligned;
 * cell: [B] int32; ws: rc_ivf_coarse_assign_ws_bytes(nlist).  A misaligned x or cent is RC_ESHAPE, nothing is launched.
 * Score of (b, l): fl(cnorm_l - 2 acc), acc the fp32 fma chain over d ascending, cnorm_l the 64-lane strided fma chains
 * of c_l^2 added as a butterfly.  A NaN score never wins; a row with no score below +inf goes to cell 0. */
size_t rc_ivf_coarse_assign_ws_bytes(int nlist);
int rc_ivf_coarse_assign(rc_handle_t h, const float* x, int64_t ldx, const float* cent, int64_t B, int D, int nlist,
                         int* cell, void* ws, size_t ws_bytes, rc_stream_t stream);

/* Centroid update of the coarse k-means (the Lloyd step after rc_ivf_coarse_assign; repconc_amd/ivf.py::coarse_kmeans —
 * a build-side extension, BASELINE configs[3] "IVF nlist=5000"): cent[l] <- mean of the rows with assign[r] == l, summed in
 * a fixed order in fp64 by one block per cell after a stable counting sort (four interleaved row lanes, each ascending, then
 * ((p0 + p1) + p2) + p3: deterministic, no atomics on values);
 * an empty cell takes row splitmix64(seed, iter, l) mod n.  assign: int32 [n] (entries outside [0, nlist) are ignored);
 * counts_out: optional uint32 [nlist].  D % 4 == 0, D <= 1024, nlist <= 16384, 16-byte aligned x / cent rows.
 * ws: rc_ivf_coarse_update_ws_bytes(n, nlist). */
size_t rc_ivf_coarse_update_ws_bytes(int64_t n, int nlist);
int rc_ivf_coarse_update(rc_handle_t h, const float* x, int64_t ldx, const int* assign, int64_t n, int D, int nlist, float* cent,
                         unsigned* counts_out, uint64_t seed, int iter, void* ws, size_t ws_bytes, rc_stream_t stream);
/* List-centric search of the same index (M in {16,32,48,64,96}): all queries probing a cell are split into groups of up
 * to 8, one block per (cell, group) task runs the conflict-free 8-bit screen of the flat search over the cell's rows,
 * survivors are re-scored exactly — results identical to rc_ivf_search.  image: rc_adc_scan_image of the cell-major codes.
 * Per query: probes / sbase [nq,nprobe] (probed cells; position of each probe's first SAMPLED row — a cell of n rows is
 * sampled in runs of 16 rows every 16 ss rows, 16 floor(n / 16 ss) + min(16, n mod 16 ss) entries — in the query's sample
 * array of stride sstride), scount (sampled rows), rows (probed rows), rank (rank of the
 * sample score used as threshold, 0 = keep every probed row).  Tasks: task_list / task_qstart / task_qcnt [ntasks] over
 * sorted_q (query ids ordered by probed cell).  status bit0: a query kept fewer than min(k, rows) candidates (retry with
 * larger ranks), bit1: a candidate list overflowed. */
size_t rc_ivf_search_lists_ws_bytes(int M, int nq, int64_t sstride);
int rc_ivf_search_lists(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                        const int64_t* rowmap, int64_t N, int M, int K, const float* lut, int nq, const int* probes,
                        const int* sbase, const int* scount, const int* rows, const int* rank, int nprobe,
                        int64_t sstride, int ss, const int* task_list, const int* task_qstart, const int* task_qcnt,
                        const int* sorted_q, int ntasks, int k, float* scores, int64_t* out_ids, int* status, void* ws,
                        size_t ws_bytes, rc_stream_t stream);
/* The same search with the plan made on the device: sample layout, threshold ranks and the task list are derived from
 * `probes` by four small kernels (no host round trip).  probes [nq,nprobe]: distinct cells per query, nprobe <= nlist;
 * sstride: capacity of a query's sample array, >= the largest possible number of sampled rows of nprobe cells;
 * sel_slack: standard deviations of head-room in the threshold rank (the Python wrapper passes 4: IVFPQIndex.SEL_SLACK);
 * keep_all_rows: queries probing no more rows than this re-score every probed row.  Status bits and results as above.
 * ws: rc_ivf_search_probes_ws_bytes(M, nq, nprobe, nlist, sstride). */
/* Probe selection for the calls below: per query the nprobe cells with the largest coarse score (scores [nq,nlist] fp32,
 * e.g. q @ coarse^T from a library GEMM; ties at the boundary go to the lower cell id), written in ASCENDING CELL ORDER to
 * probes [nq,nprobe] int32 — the searches need the set of cells, not their ranking.  nlist <= 16384.
 * Order of the scores: that of the numbers, -0.0 and +0.0 tie (the kernel orders the bits of s + 0.0f).  A NaN orders by
 * its bits: above +inf with the sign bit clear, below -inf with it set, NaNs of one sign by payload; the output is nprobe
 * distinct ascending cells whatever the scores hold. */
int rc_ivf_select_probes(rc_handle_t h, const float* scores, int nq, int nlist, int nprobe, int* probes,
                         rc_stream_t stream);
size_t rc_ivf_search_probes_ws_bytes(int M, int nq, int nprobe, int nlist, int64_t sstride);
int rc_ivf_search_probes(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                         const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                         const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                         int keep_all_rows, float* scores, int64_t* out_ids, int* status, void* ws, size_t ws_bytes,
                         rc_stream_t stream);
/* rc_ivf_search_probes with per-query status words: qstatus [nq] int32 (zeroed by the caller, may be NULL) gets bit 0 for a
 * query that kept fewer than min(k, rows probed) candidates and bit 1 for one whose id list overflowed; the other queries'
 * results stand, so a caller answers only the flagged ones again (repconc_amd.ivf: by the per-query exact scan).  status bit 2
 * (value 4, both entries): a survivor stream of the screen filled up — nobody's results are reliable, repeat with a smaller
 * sel_slack. */
int rc_ivf_search_probes_q(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                           const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                           const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                           int keep_all_rows, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws,
                           size_t ws_bytes, rc_stream_t stream);
/* The same search on the 16-query screen (round 6; evaluate_repconc.py:180-206 with a list-centric index and whole-query-set
 * calls): tasks of up to 16 queries per probed cell, one ds_read_b128 gather + one i8 MFMA per (16 rows, 4 sub-quantisers,
 * 16 queries) — per query the same table bytes as the 8-query screen and half the gathers.  image16: rc_adc_scan_image_rows16.
 * Same workspace (rc_ivf_search_probes_ws_bytes), status bits and RESULTS as rc_ivf_search_probes_q; it pays when a probed
 * cell is shared by more than ~8 queries of the call (nq x nprobe / nlist). */
int rc_ivf_search_probes_q16(rc_handle_t h, const uint8_t* codes, const uint8_t* image16, const int64_t* list_off,
                             const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                             const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                             int keep_all_rows, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws,
                             size_t ws_bytes, rc_stream_t stream);
size_t rc_ivf_search_ws_bytes(int nq, int64_t stride);
int rc_ivf_search(rc_handle_t h, const uint8_t* codes, const int64_t* list_off, const int64_t* ids, int64_t N,
                  int M, int K, const float* lut, const int* probes, const int* base, const int* count, int nq,
                  int nprobe, int64_t stride, int k, float* scores, int64_t* out_ids, int* status, void* ws,
                  size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ IVF over dense rows (csrc/ivf_flat.hip; faiss.IndexIVFFlat)
 * The exact scan of the part of a dense store that a coarse quantiser selects.  x [N, ldx] holds the rows list-major (sorted by
 * coarse cell; fp32, rc_ivf_flat_f16_search: fp16 bit patterns, x and q both), list_off [nlist + 1] int64 the first row of
 * every cell, ids [N] int64 the corpus position of every row, q [nq, D] the queries, probes [nq, nprobe] int32 the probed
 * cells of every query: distinct, in ascending order, as rc_ivf_select_probes writes them.
 * metric: 0 = inner product, 1 = squared L2.
 * Score of a (query, row) pair: bit for bit the chain of the flat dense searches (rc_dense_search_exact /
 *   rc_dense_l2_search_exact and their f16 forms): one fp32 accumulator from +0.0f, d ascending, values widened to fp32; inner
 *   product s = fmaf(q[d], x[n][d], s); L2 t = q[d] - x[n][d], s = fmaf(t, t, s).
 * Output scores / ids [nq, k]: inner product: score descending; L2: distance ascending; ties by the lower CORPUS id (ids[row],
 *   not the row); (-inf, -1) / (+inf, -1) when the probed cells hold fewer than k rows; a zero L2 distance is +0.0f.  A score
 *   that overflows to +-inf from finite inputs is ordered as the number it is, ties by the lower corpus id, and every row of the
 *   probed cells comes ahead of the padding: L2 (+inf, id) after the finite distances and before (+inf, -1); inner product
 *   (+inf, id) first and (-inf, id) after the finite scores, before (-inf, -1).  More than 16384 such rows at the k-th score are
 *   a tie group like any other (status bit 1).  NaN scores (inf - inf inside a chain, NaN inputs) are outside the contract.
 *   Probing every cell gives exactly what the flat search gives over the same vectors.
 * The scan is list-centric: the plan (cells, the queries of every cell, tasks of up to 8 queries of one cell) is made on the
 *   device from `probes` and `list_off`, a cell's rows are read once per task, every pair's score goes to the query's dense
 *   score row (stride floats per query; ANY stride >= the rows the probed cells of every query of the call hold is valid, odd
 *   or far larger included — the largest number of rows nprobe cells can hold, rounded up to a multiple of 4, is merely what
 *   IVFFlatIndex passes; the result does not depend on it), then the exact k-th largest score per query, the keys at or above
 *   it and the select of the other searches.  No sampling, no slack.
 * status (one device int, zeroed by the caller) / qstatus [nq] (zeroed by the caller, may be NULL): bit 1 (value 2) = more than
 *   16384 probed rows tie at the query's k-th score, its output is not valid (answer it by an exact search over its probed
 *   rows); the other queries' results stand.  status bit 2 (value 4) = a caller's error the device found: a probe outside
 *   [0, nlist) or more probed rows than `stride`; nothing is written out of bounds, the results are not valid.
 * Limits: 1 <= k <= 8192, N < 2^32, nlist <= 16384, metric in {0, 1} (else RC_ESHAPE); any D >= 1, ldx >= D; probed rows per
 *   query < 2^31; finite inputs (rows, queries, dec, coarse: the scores they overflow to are served, see above); one device.
 *   Rows are read with 16-byte loads when x is 16-byte aligned and D and ldx are multiples of 16 bytes, element by element
 *   otherwise — the same arithmetic.  Null or non-positive arguments (nprobe > nlist, ldx < D included) are RC_EINVAL;
 *   nq == 0 returns RC_OK and touches nothing.
 * Runs on `stream`; no host synchronisation, no atomics on values, results bit-identical from run to run.
 * ws: rc_ivf_flat_search_ws_bytes(nq, nprobe, nlist, stride), a multiple of 256 (8 bytes per probed row and 128 KiB of keys per
 *   query, plus the plan); 0 for nq <= 0, nprobe <= 0, nprobe > nlist or stride <= 0.  RC_EWORKSPACE for a short one. */
size_t rc_ivf_flat_search_ws_bytes(int nq, int nprobe, int nlist, int64_t stride);
/* queries of one cell that share a task of the scan (8): what tests and tools need to hit the group boundary; no GPU involved */
int rc_ivf_flat_query_group(void);
int rc_ivf_flat_search(rc_handle_t h, const float* x, int64_t ldx, const int64_t* list_off, const int64_t* ids, int64_t N,
                       int nlist, int D, const float* q, int nq, const int* probes, int nprobe, int64_t stride, int k,
                       int metric, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                       rc_stream_t stream);
int rc_ivf_flat_f16_search(rc_handle_t h, const uint16_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                           int64_t N, int nlist, int D, const uint16_t* q, int nq, const int* probes, int nprobe,
                           int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status, int* qstatus,
                           void* ws, size_t ws_bytes, rc_stream_t stream);
/* rc_ivf_flat_sq8_search (faiss.IndexIVFScalarQuantizer, QT_8bit, vectors encoded themselves): the same search over a
 *   list-major store of 8-bit scalar-quantiser codes, x [N, ldx] int8 = c - 128 and dec [2][D] fp32 = step, mid as in
 *   rc_dense_sq8_search_q; q [nq, D] fp32, not rounded.  A value is decoded once, x^[n][d] = fmaf((float)c'[n][d], step[d],
 *   mid[d]), and feeds the chain above: scores are bit for bit what rc_ivf_flat_search gives over the decoded rows
 *   (rc_dense_sq8_decode), under either metric — the scan is the exact chain, no screen and no certificate.  D > rc_dense_sq8_max_d()
 *   is RC_ESHAPE and is checked first, as the rc_dense_sq8 entries check it; then the checks of rc_ivf_flat_search in their
 *   order, with dec among the pointers.  16-byte loads when x is
 *   16-byte aligned and D and ldx are multiples of 16, byte by byte otherwise.  ws: rc_ivf_flat_search_ws_bytes (the layout
 *   does not depend on the storage type). */
int rc_ivf_flat_sq8_search(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids, int64_t N,
                           int nlist, int D, const float* q, int nq, const float* dec, const int* probes, int nprobe,
                           int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status, int* qstatus,
                           void* ws, size_t ws_bytes, rc_stream_t stream);
/* rc_ivf_flat_sq8r_search (faiss.IndexIVFScalarQuantizer, QT_8bit, by_residual = true): rc_ivf_flat_sq8_search over codes of
 *   RESIDUALS.  Row n of cell l holds the codes of fp32(x[n][d] - coarse[l][d]) under one range (step, mid) shared by all cells;
 *   coarse [nlist, ldc] fp32, ldc >= D, are the centroids the rows were encoded against.  A stored value is
 *     x^[n][d] = fp32(fmaf((float)c'[n][d], step[d], mid[d]) + coarse[l][d]):
 *   the decode of rc_ivf_flat_sq8_search, then ONE separate fp32 addition (two roundings, never one fused operation), done once
 *   per value on its way into the scan's fp32 tile.  x^ feeds the chain above: scores are bit for bit what rc_ivf_flat_search
 *   gives over those rows, under either metric; plan, selection, ties, padding, status bits, limits and ws
 *   (rc_ivf_flat_search_ws_bytes) are those of rc_ivf_flat_sq8_search.  Only the centroids of probed cells are read, D values
 *   of a row each.  Checks in the order of rc_ivf_flat_sq8_search: D > rc_dense_sq8_max_d() is RC_ESHAPE and comes first; then
 *   dec and coarse among the pointers (a null coarse or ldc < D is RC_EINVAL). */
int rc_ivf_flat_sq8r_search(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids, int64_t N,
                            int nlist, int D, const float* q, int nq, const float* dec, const float* coarse, int64_t ldc,
                            const int* probes, int nprobe, int64_t stride, int k, int metric, float* scores, int64_t* out_ids,
                            int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ IVF over dense rows, a subset of the rows
 * The four searches above over the selected rows of the store, in place: no copy of the rows is made, and the score rows, the
 * workspace and the rows read follow the selection, not N.  rows: DEVICE int64 [ns], the LIST-MAJOR positions (rows of x, not
 * corpus ids) of the selected rows, strictly ASCENDING, no row twice, every one in [0, N) — ascending positions are grouped by
 * cell, and ascend by corpus id inside a cell because the store is stably sorted.  sel_off: DEVICE int64 [nlist + 1], the
 * offsets of the cells INSIDE rows: rows[sel_off[c] .. sel_off[c + 1]) are the selected rows of cell c, every one in
 * [list_off[c], list_off[c + 1]); sel_off[0] = 0, sel_off[nlist] = ns.  THE LIBRARY DOES NOT VERIFY ANY OF THIS: rows and
 * sel_off are never read on the host, and a row outside [0, N) is a read outside x (the Python wrapper checks the pair unless
 * told not to, ops.ivf_flat_search(rows=..., sel_off=..., check_rows=True)).
 * Result: exactly what the entry of the same name without _rows returns for a store that holds only the selected rows, each
 * under the cell it has here, with the same probes, dec and coarse — ids (ids[rows[i]], the corpus ids of THIS store) and
 * score / distance bits, ties by the lower corpus id, the padding (-inf or +inf, -1) where the probed cells hold fewer than k
 * selected rows.  The plan reads sel_off where it reads list_off; the scan reads logical row i of cell c at x + rows[sel_off[c]
 * + i] * ldx (rows[] once per row and chunk of 512 rows, never at or past sel_off[c + 1]) and hands the store position on, so
 * the k-th score, the filter, the select and the status bits are those of the entry without _rows.  The residual form adds the
 * centroid of the task's cell: a selected row's cell is its cell.
 * Arguments: those of the entry without _rows, then `rows, ns, sel_off`.  stride: >= the SELECTED rows the probed cells of any
 * query hold; ws: rc_ivf_flat_search_ws_bytes(nq, nprobe, nlist, stride) with that stride.  list_off is checked (non-null) and
 * otherwise not read.
 * Checks: the argument checks of the entry without _rows in their order (RC_EINVAL, RC_ESHAPE), then rows or sel_off NULL or
 * ns outside [1, N] (RC_EINVAL), then nq == 0 (RC_OK, nothing enqueued), the workspace (RC_EWORKSPACE), then device work. */
int rc_ivf_flat_search_rows(rc_handle_t h, const float* x, int64_t ldx, const int64_t* list_off, const int64_t* ids, int64_t N,
                            int nlist, int D, const float* q, int nq, const int* probes, int nprobe, int64_t stride, int k,
                            int metric, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                            rc_stream_t stream, const int64_t* rows, int64_t ns, const int64_t* sel_off);
int rc_ivf_flat_f16_search_rows(rc_handle_t h, const uint16_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                int64_t N, int nlist, int D, const uint16_t* q, int nq, const int* probes, int nprobe,
                                int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status, int* qstatus,
                                void* ws, size_t ws_bytes, rc_stream_t stream, const int64_t* rows, int64_t ns,
                                const int64_t* sel_off);
int rc_ivf_flat_sq8_search_rows(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                int64_t N, int nlist, int D, const float* q, int nq, const float* dec, const int* probes,
                                int nprobe, int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status,
                                int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream, const int64_t* rows, int64_t ns,
                                const int64_t* sel_off);
int rc_ivf_flat_sq8r_search_rows(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                 int64_t N, int nlist, int D, const float* q, int nq, const float* dec, const float* coarse,
                                 int64_t ldc, const int* probes, int nprobe, int64_t stride, int k, int metric, float* scores,
                                 int64_t* out_ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream,
                                 const int64_t* rows, int64_t ns, const int64_t* sel_off);

/* ------------------------------------------------------------------ JPQ scoring head (csrc/jpq_head.hip)
 * Scores of (query, document id) pairs straight from the resident codes, and their gradients (stage 2 of the recipe,
 * models/jpq/finetune_jpq.py:176-189, without the decoded embeddings and without atomics on values).
 * q [nq, D] fp32 (D = M*dsub, contiguous), codes [N, M] uint8, pids [nq, k] int64, C [M, 256, dsub] fp32, g [nq, k] fp32.
 * An id outside [0, N) is a hole: its score is +0.0f and it contributes to no gradient.
 * Every product is of two fp32 values taken in fp64 (exact); every sum is fp64, sequential from 0.0, rounded to fp32 once:
 *   scores[i,t]   = fp32(sum_m (sum_j q[i, m*dsub+j] * C[m, codes[pids[i,t], m], j]))       j ascending, then m ascending
 *   grad_q[i,d]   = fp32(sum_t g[i,t] * C[m, codes[pids[i,t], m], j]),  d = m*dsub+j          t ascending, holes skipped
 *   grad_C[m,c,j] = fp32(sum_p g[p] * q[p div k, m*dsub+j])  over the pairs p = i*k+t with codes[pids[p], m] == c, p ascending
 *                   (stable counting sort of the pairs by code per sub-quantiser, then one owner per (m, c) segment; a segment
 *                   no pair hits gets +0.0f).
 * The results are functions of the inputs alone (bit-identical from run to run).  K must be 256; any M >= 1, dsub >= 1;
 * nq*k < 2^31, N < 2^32.  nq == 0 or k == 0: RC_OK, nothing is launched and the outputs are not touched.
 * rc_jpq_head_bwd: grad_q [nq, D] and / or grad_C [M, 256, dsub]; a null output is not computed (both null: RC_EINVAL).
 * ws (rc_jpq_head_ws_bytes(nq, k, M), needs no GPU) is used for grad_C only. */
size_t rc_jpq_head_ws_bytes(int nq, int k, int M);
int rc_jpq_head_fwd(rc_handle_t h, const float* q, const uint8_t* codes, int64_t N, const int64_t* pids, const float* C,
                    int nq, int k, int M, int K, int dsub, float* scores, rc_stream_t stream);
int rc_jpq_head_bwd(rc_handle_t h, const float* q, const uint8_t* codes, int64_t N, const int64_t* pids, const float* C,
                    const float* g, int nq, int k, int M, int K, int dsub, float* grad_q, float* grad_C, void* ws,
                    size_t ws_bytes, rc_stream_t stream);

/* ------------------------------------------------------------------ stage-1 contrastive loss (csrc/contrastive.hip)
 * The in-batch softmax loss of stage 1 (models/repconc/finetune_repconc.py:398-451: compute_contrastive_loss with its false-negative
 * and duplicate masks and the dynamic top-k cut) on a similarity matrix the caller has already computed, and its gradient w.r.t.
 * that matrix.  No [nd, nd] compare, no [nq, nd] mask, no atomics on values.
 * sim [nq, nd] fp32 contiguous, finite, 1 <= nq <= nd <= 262144 (the duplicate flags are an all-pairs compare of the ids:
 * nd^2 / 2; RC_EINVAL above the limit, as for nq > nd); the label of row i is column i.  docids [nd] int64.  The positives of
 * query i are rel_ids[rel_off[i] .. rel_off[i+1]) — rel_off [nq+1] and rel_ids [R] int64, a row may be empty, both ends are
 * clamped into [0, R] (rel_ids may be NULL when R == 0).  0 <= topk <= nd, 0 = no cut.  Per row i:
 *   1. dup[j]    = some i' < j has docids[i'] == docids[j]              (the later occurrences: triu(diagonal=1).any(0))
 *   2. mask[i,j] = j != i and (dup[j] or docids[j] is one of the positives of i)
 *   3. z1[i,j]   = fp32(sim[i,j] - 10000) where mask, sim[i,j] elsewhere
 *   4. topk > 0: neg = z1 with neg[i,i] = -10000; keep = the topk largest of neg[i,:] (ordered as numbers, -0.0 and +0.0 tie;
 *      ties at the cut go to the lower j; masked columns take part), plus column i;  z = z1 where keep, fp32(z1 - 10000)
 *      elsewhere.  topk == 0: z = z1 (topk == nd keeps every column: the same).
 *   5. with mx = max_j z[i,j], e_j = exp((double)z[i,j] - mx), off = sum_{j != i} e_j and sum = off + e_i, all fp64:
 *      loss_i = (mx + log(sum)) - z[i,i].  off is summed in a fixed order: thread t of 256 adds the columns t, t + 256, ...
 *      ascending, the 64 lanes of a wave are added as a butterfly, the four waves in order.
 *      loss = fp32((sum_i loss_i) / nq), i ascending from 0.0 in fp64.
 *   6. grad_sim[i,j] = fp32((gout * v) / nq) in fp64, v = e_j / sum for j != i and v = -(off / sum) for j == i: the diagonal
 *      term (e_i - sum) / sum without its cancellation.
 * z is bit-equal to the torch composition's logits wherever the cut has no tie; loss and gradient are functions of the inputs
 * alone (bit-identical from run to run).
 * rc_contrastive_fwd: loss = one device float; z_out [nq, nd] is written only when non-null (test hook).  It fills ws (the
 *   duplicate flags, nq * ceil(nd / 64) 64-bit words of keep bits, four doubles per row), which
 * rc_contrastive_bwd reads back together with the same sim, ids and topk: gout = one device float, grad_sim [nq, nd] is overwritten.
 * ws: rc_contrastive_ws_bytes(nq, nd) bytes (needs no GPU; 0 for arguments outside the limits above); a null or short workspace
 * is RC_EWORKSPACE. */
size_t rc_contrastive_ws_bytes(int64_t nq, int64_t nd);
int rc_contrastive_fwd(rc_handle_t h, const float* sim, const int64_t* docids, const int64_t* rel_off, const int64_t* rel_ids,
                       int64_t R, int64_t nq, int64_t nd, int64_t topk, float* loss, float* z_out, void* ws, size_t ws_bytes,
                       rc_stream_t stream);
int rc_contrastive_bwd(rc_handle_t h, const float* sim, const int64_t* docids, const int64_t* rel_off, const int64_t* rel_ids,
                       int64_t R, int64_t nq, int64_t nd, int64_t topk, const float* gout, float* grad_sim, const void* ws,
                       size_t ws_bytes, rc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* REPCONC_HIP_H */
