// What the eight dense flat searches share beyond the fp32 GEMM of dense_gemm.h (dense_search.hip: fp32 corpus and screen,
// dense_search_f16.hip: fp16 corpus and f16 screen, dense_search_bf16x3.hip: fp32 corpus and bf16x3 screen,
// dense_search_l2.hip: fp32 corpus, squared Euclidean distance, dense_search_l2_f16.hip: the same over an fp16 corpus,
// dense_search_l2_bf16x3.hip: the fp32 L2 corpus under the bf16x3 screen, dense_search_sq8.hip: int8 scalar-quantiser codes,
// fp32 queries and the int8 screen, dense_search_l2_sq8.hip: the same codes under the squared Euclidean distance): the
// route of a search and the bodies of its entries, the pieces common to the two 16x16x32 screen GEMMs, the rescoring kernel
// and the certificate kernel.  Device code: every translation unit compiles its own copy, no -fgpu-rdc.
//
// The route (dense_search_route).  A variant V supplies the storage type, its screen GEMM, an optional query pre-pass and,
// if its screen only approximates the score (V::approximate), the bound E_q of its certificate.  The L2 variant (V::l2) scores
// s = -d: its screen takes the rows' squared norms as a side operand, its chain is the one of squared differences, and
// V::finish turns the k output values into d at the end.
//   Exact route (N <= DENSE_EXACT_MAX_N, and the queries the fast route gives up on; dense_exact): V::exact_rows writes the
//   full score rows of a chunk of queries, the chain itself (dense_gemm_kernel<STORE> of dense_gemm.h, the fp32 matrix cores
//   over rows widened on load; L2: dense_l2_exact_kernel), then the 8-pass radix select over the 64-bit keys
//   (topk_exact_select), then V::finish.  It terminates with the same answer for any content (all rows identical, k >= N, ...).
//   Fast route (N > 4 S, S = min(N, 32768)):
//   0. V::prepass: the bf16x3 screens split the queries into two bf16 planes in the tail of the workspace, the int8 screen
//      quantises them to two int8 planes there; nothing for the others
//   1. screen<STORE> over the strided sample j -> row j N / S: s~ of the sample (fp32 screen: s~ = s, the chain)
//   2. adc_threshold_kernel (topk.hip): thr~[q] = the r-th best s~ of the sample, r by the ADC formula (rc_adc_sample_rank)
//   3. screen<FILTER> over all N rows: the key (s~, row) of every s~ >= thr~[q] -> q's candidate list
//   4. approximate only: V::rescore (dense_rescore_kernel; coded: the same over rows decoded on the fly) replaces the score
//      half of every candidate key by the chain
//   5. adc_select_kernel (rc_adc_launch_select): sort + emit; qstatus bit0 = fewer than min(k, N) candidates, bit1 = overflow
//   6. approximate only: V::certify (dense_certify_kernel; coded: a kernel of its own).  With t = the query's k-th exact score
//      and |s~ - s| <= E_q for every row, a row outside the list has s~ < thr~, hence s < thr~ + E_q: if t >= thr~ + E_q
//      (everything in fp64, rounded upwards) no such row can enter the top-k or tie with its last member and the answer is
//      proven equal to the exact route's.
//      Otherwise qstatus bit2, "not certified": the caller repeats the query with another slack or takes the exact route.
//   7. V::finish, after the certificate has read the scores
#pragma once
#include "dense_gemm.h"

#include <limits.h>
#include <type_traits>

typedef float dense_f32x4 __attribute__((ext_vector_type(4)));

// ---- the two screen GEMMs (v_mfma_f32_16x16x32_f16 / _bf16) -----------------------------------------------------------------
// Both stage one operand tile as 128 rows of 128 bytes = 8 chunks of 16 bytes, two operands x two buffers: 64 KB, two blocks
// per CU; wave (wr, wc) owns 64 queries x 64 rows as 4 x 4 tiles of 16 x 16, lane l holds k = 8 (l / 16) .. + 7 of row l % 16 of
// both operands; result element r of lane l is corpus row l % 16 and query 4 (l / 16) + r of the tile.
#define DENSE_SCREEN_OPERAND_BYTES (DENSE_TILE * 128)
#define DENSE_SCREEN_LDS_BYTES (4 * DENSE_SCREEN_OPERAND_BYTES)

// byte offset of the 16-byte chunk c of tile row `row`: XOR swizzle with (row / 2) % 8.  Two rows share 256 bytes = all 64
// banks, and any 16 lanes that hold 16 consecutive rows of one chunk index (a quarter of a ds_read_b128 of the 16x16x32
// operand map) cover all 64 banks once.
__device__ __forceinline__ int dense_screen_lds_off(int row, int c) { return row * 128 + ((c ^ ((row >> 1) & 7)) << 4); }

// FILTER: the thresholds of the query tile at qt go where the operand buffer that the last of the nkc K stages did not read
// lies (sa: the query operand's two buffers); call after the K loop's last barrier.  Returns where they are.
template <int MODE>
__device__ __forceinline__ const float* dense_screen_stage_thr(unsigned char* sa, int nkc, const float* __restrict__ thr,
                                                               int qt, int nq, int tid) {
    float* s_thr = reinterpret_cast<float*>(sa + (nkc & 1) * DENSE_SCREEN_OPERAND_BYTES);
    if constexpr (MODE == DENSE_FILTER) {
        if (tid < DENSE_TILE) s_thr[tid] = (qt + tid < nq) ? thr[qt + tid] : INFINITY;
        __syncthreads();
    }
    return s_thr;
}

// this lane's side operand of the L2 epilogue: nxs[b] = minus the stored squared norm of its corpus row of column tile b,
// read at the mapped corpus row of the strided sample (smap != 0) as the screen's loader reads the row itself; once per block.
// MAP (subset search): at rows[that row], the norm of the corpus row the loader reads (dense_corpus_row)
template <bool MAP = false>
__device__ __forceinline__ void dense_screen_load_nxs(const float* __restrict__ xsq, int64_t j0, int wc, int col, int64_t N,
                                                      int64_t nrows, int64_t smap, float (&nxs)[4],
                                                      const int64_t* __restrict__ rows = nullptr) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t j = j0 + wc * 64 + b * 16 + col;
        const int64_t jc = j < nrows ? j : nrows - 1;
        nxs[b] = -xsq[dense_corpus_row<MAP>(jc, N, smap, rows)];
    }
}

// the epilogue of a wave's 4 x 4 result tiles: dense_emit on every element; L2: on sigma = fmaf(2, dot, nxs[b]) as
// dense_gemm_body<.., L2 = true> emits it (nxs: dense_screen_load_nxs)
template <int MODE, bool L2 = false>
__device__ __forceinline__ void dense_screen_epilogue(const dense_f32x4 (&acc)[4][4], int64_t j0, int wr, int wc, int col,
                                                      int grp, int qt, int nq, const float* s_thr, int64_t nrows,
                                                      float* __restrict__ out, unsigned* __restrict__ cnt,
                                                      unsigned long long* __restrict__ cand, int l,
                                                      const float* nxs = nullptr) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t j = j0 + wc * 64 + b * 16 + col;
        const bool jv = j < nrows;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qo = wr * 64 + a * 16 + 4 * grp + r;
                float sc = acc[a][b][r];
                if constexpr (L2) sc = __builtin_fmaf(2.f, sc, nxs[b]);
                dense_emit<MODE, 16>(sc, j, jv, qt + qo, nq, MODE == DENSE_FILTER ? s_thr[qo] : 0.f, nrows, out, cnt, cand, l);
            }
    }
}

// ---- rescoring --------------------------------------------------------------------------------------------------------------
#define DENSE_RESCORE_QCHUNK 1024                        // query values staged in LDS

// one step of the chain: s = fmaf(q, x, s), or for L2 a literal subtraction, then fmaf(t, t, s) (-ffp-contract=off: two roundings)
template <bool L2>
__device__ __forceinline__ float dense_chain_step(float q, float x, float s) {
    if constexpr (L2) {
        const float t = q - x;
        return __builtin_fmaf(t, t, s);
    } else {
        return __builtin_fmaf(q, x, s);
    }
}

// grid: (nq, ADC_CAND_CAP / 256) blocks of 256 threads; one lane per candidate key of query blockIdx.x.  The key's score half
// (the screen's s~) is replaced by the chain: dense_chain_step<L2>, d ascending, one accumulator, over the values widened to
// fp32 (exact); L2: by -d.  VEC: 16-byte aligned rows.  MAP (subset search): the key's row is a row of x[rows] and stays in
// the key; the row that is read is rows[row], one load per lane.  !MAP never reads rows.
template <bool VEC, typename T, bool L2, bool MAP = false>
__global__ __launch_bounds__(256) void dense_rescore_kernel(const T* __restrict__ x, int64_t ldx, int D, const T* __restrict__ q,
                                                            const unsigned* __restrict__ cnt,
                                                            unsigned long long* __restrict__ cand,
                                                            const int64_t* __restrict__ rows) {
    __shared__ float sq[DENSE_RESCORE_QCHUNK];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const unsigned raw = cnt[qi];
    const unsigned n = raw > ADC_CAND_CAP ? ADC_CAND_CAP : raw;
    if (blockIdx.y * 256u >= n) return;                                // block-uniform
    const unsigned i = blockIdx.y * 256u + tid;
    const bool mine = i < n;
    unsigned long long* kp = cand + (size_t)qi * ADC_CAND_CAP + i;
    const unsigned row = mine ? 0xFFFFFFFFu - (unsigned)(*kp & 0xFFFFFFFFull) : 0u;
    const T* xp = x + dense_corpus_row<MAP>((int64_t)row, 0, 0, rows) * ldx;
    const T* qp = q + (int64_t)qi * D;
    float s = 0.f;
    for (int d0 = 0; d0 < D; d0 += DENSE_RESCORE_QCHUNK) {
        const int dn = D - d0 < DENSE_RESCORE_QCHUNK ? D - d0 : DENSE_RESCORE_QCHUNK;
        __syncthreads();
        for (int d = tid; d < dn; d += 256) sq[d] = (float)qp[d0 + d];
        __syncthreads();
        if (mine) {
            int d = 0;
            if constexpr (VEC) {
                for (; d + 8 <= dn; d += 8) {
                    float v[8];
                    dense_load8(xp + d0 + d, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = dense_chain_step<L2>(sq[d + e], v[e], s);
                }
            }
            for (; d < dn; ++d) s = dense_chain_step<L2>(sq[d], (float)xp[d0 + d], s);
        }
    }
    if (mine) *kp = adc_exact_key(L2 ? -s : s, (int64_t)row);
}

// o.rows is read only if MAP: a template argument, as in dense_launch_gemm
template <bool L2, bool MAP = false, typename T>
static int dense_launch_rescore(rc_handle_t h, const dense_operands& o, const T* x, int64_t ldx, int D, const T* q, int nq,
                                const unsigned* cnt, unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)nq, ADC_CAND_CAP / 256);
    if (ldx % (16 / (int)sizeof(T)) == 0 && !((uintptr_t)x & 15u))
        hipLaunchKernelGGL((dense_rescore_kernel<true, T, L2, MAP>), grid, dim3(256), 0, s, x, ldx, D, q, cnt, cand, o.rows);
    else
        hipLaunchKernelGGL((dense_rescore_kernel<false, T, L2, MAP>), grid, dim3(256), 0, s, x, ldx, D, q, cnt, cand, o.rows);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ---- certificate ------------------------------------------------------------------------------------------------------------
// grid: nq blocks of 64 threads.  Sets bit2 of status / qstatus[q] unless t >= thr~ + E_q is proven (step 6 above).  V supplies
//   V::eq(D, ss, xnorm)   E_q in fp64 from the sum of the query's squares and X = xnorm >= the largest row norm of the corpus,
//                         pushed upwards by more than its rounding errors
//   V::refuse(v, D)       a query value (or a D) for which the bound is not proven
// The sum is pushed upwards too; a NaN anywhere is "not certified".
template <typename V>
__global__ __launch_bounds__(64) void dense_certify_kernel(const typename V::T* __restrict__ q, int D, int k,
                                                           const float* __restrict__ thr,
                                                           const float* __restrict__ xnorm_max,
                                                           const float* __restrict__ scores, int* __restrict__ status,
                                                           int* __restrict__ qstatus) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    const typename V::T* qp = q + (int64_t)qi * D;
    double ss = 0.0;
    int refused = 0;
    for (int d = lane; d < D; d += 64) {
        const float f = (float)qp[d];
        refused |= V::refuse(f, D);
        const double v = (double)f;
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o);
        refused |= __shfl_xor(refused, o);
    }
    if (lane != 0) return;
    const double sum = (double)thr[qi] + V::eq(D, ss, (double)xnorm_max[0]);
    const double bound = sum + fabs(sum) * 0x1p-30;
    const double t = (double)scores[(size_t)qi * k + (k - 1)];
    if (refused || !(t >= bound)) {
        atomicOr(status, 4);
        if (qstatus) atomicOr(qstatus + qi, 4);
    }
}

// ---- the route --------------------------------------------------------------------------------------------------------------
// A variant V : dense_variant_defaults<V>, one interface for all eight.  What it says about itself:
//   typedef T                      type of q, and of x unless V says otherwise
//   typedef X                      optional: the storage type of x where it is not T (dense_storage<V>)
//   typedef Q                      what its screen reads as the query operand (T, or what the pre-pass leaves in the workspace)
//   static constexpr bool approximate                     its screen only approximates the score: rescore and certify run
//   static constexpr bool l2                              scores are -d: the entries take o.xsq [N], the squared norm of every
//                                                         row, and the rescorer walks dense_chain_step<true>
//   static constexpr bool coded                           x holds codes that the per-dimension vectors o.dec decode
//                                                         (dense_sq8_chain.h): every entry takes o.dec, and nothing is asked of
//                                                         the alignment, the int8 screen has a form for any row pitch
//   static constexpr bool subset                          it serves the subset search ("subset search" below): its hooks choose
//                                                         the mapped form of their kernel where o.rows is set.  The others
//                                                         never see o.rows set and instantiate no mapped kernel.
//   static constexpr int max_d                            the largest D of its screen (int8: DENSE_I8_MAX_D)
//   static constexpr unsigned ws_align                    alignment the workspace must have
//   static constexpr bool screen_aligned                  launch_gemm reads rows of D % 16 == 0 elements with 16-byte loads
//                                                         whatever their pitch: the scores entry checks dense_aligned
//   static size_t extra_ws_bytes(nq, D)                   workspace after the fast layout, for the pre-pass
// and its hooks, each with the handle first, the operand bundle o (dense_operands, dense_gemm.h) second, and a stream last; a
// variant reads the fields of o that it has and ignores the rest:
//   static int prepass(h, o, q, nq, D, tail, &qs, s)      qs = the screen's query operand (tail: that extra workspace)
//   static int launch_gemm<MODE>(h, o, x, ldx, N, nrows, smap, qs, nq, D, thr, out, cnt, cand, s)
//   static int exact_rows(h, o, x, ldx, N, D, q, nq, out, s)                       out [nq][N] = the chain of every pair
//   static int rescore(h, o, x, ldx, D, q, nq, cnt, cand, s)                       approximate only; default: dense_rescore_kernel
//   static int certify(h, o, q, qs, nq, D, k, thr, xnorm_max, scores, status, qstatus, s)
//                                                         approximate only; default: dense_certify_kernel<V> on V::eq / V::refuse
//   static int finish(h, scores, n, s)                    the last step over the n output values; default: launches nothing
template <typename V>
struct dense_variant_defaults {
    static constexpr bool l2 = false;
    static constexpr bool coded = false;
    static constexpr bool subset = false;
    static constexpr int max_d = INT_MAX;
    static constexpr unsigned ws_align = 1;
    static constexpr bool screen_aligned = false;
    static size_t extra_ws_bytes(int, int) { return 0; }
    template <typename T>
    static int prepass(rc_handle_t, const dense_operands&, const T* q, int, int, char*, const T** qs, hipStream_t) {
        *qs = q;
        return RC_OK;
    }
    template <typename T>
    static int rescore(rc_handle_t h, const dense_operands& o, const T* x, int64_t ldx, int D, const T* q, int nq,
                       const unsigned* cnt, unsigned long long* cand, hipStream_t s) {
        if constexpr (V::subset) {
            if (o.rows) return dense_launch_rescore<V::l2, true>(h, o, x, ldx, D, q, nq, cnt, cand, s);
        }
        return dense_launch_rescore<V::l2>(h, o, x, ldx, D, q, nq, cnt, cand, s);
    }
    template <typename T, typename Q>
    static int certify(rc_handle_t h, const dense_operands&, const T* q, const Q*, int nq, int D, int k, const float* thr,
                       const float* xnorm_max, const float* scores, int* status, int* qstatus, hipStream_t s) {
        hipLaunchKernelGGL(dense_certify_kernel<V>, dim3((unsigned)nq), dim3(64), 0, s, q, D, k, thr, xnorm_max, scores, status,
                           qstatus);
        RC_LAUNCH_CHECK(h);
        return RC_OK;
    }
    static int finish(rc_handle_t, float*, int64_t, hipStream_t) { return RC_OK; }
};

template <typename V, typename = void>
struct dense_storage { typedef typename V::T type; };
template <typename V>
struct dense_storage<V, std::void_t<typename V::X>> { typedef typename V::X type; };

template <typename V>
static bool dense_variant_shape_ok(int64_t N, int D, int nq, int k) { return dense_shape_ok(N, D, nq, k) && D <= V::max_d; }
template <typename V>
static size_t dense_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_variant_shape_ok<V>(N, D, nq, k) ? dense_exact_ws(N, nq).sel.total : 0;
}
template <typename V>
static size_t dense_search_ws_bytes(int64_t N, int D, int nq, int k) {
    if (!dense_variant_shape_ok<V>(N, D, nq, k)) return 0;
    return dense_exact_route(N) ? dense_exact_ws(N, nq).sel.total : dense_fast_ws(N, nq).total + V::extra_ws_bytes(nq, D);
}

// ---- subset search ------------------------------------------------------------------------------------------------------------
// A search over the rows o.rows [ns] of the store (int64, ascending, unique, in [0, N): the caller's word, nothing here checks
// it) is the unchanged route over the virtual matrix x' = x[rows] with N := ns: the sample size, the rank of the threshold, the
// exact-route limit and the workspace follow ns.  Four kernels form a row's address (dense_gemm_body, the f16 screen,
// dense_l2_exact_kernel, dense_rescore_kernel) and read rows[] there in their MAP form, and the L2 screens read xsq at the same
// row.  MAP stays a template argument of the kernels and of their launchers; `o.rows ? <.., true> : <.., false>` is said once per
// hook, in the four variants with V::subset (fp32 and fp16 storage, both metrics) and in the default rescorer.  The keys carry
// rows of x', so the order among equal scores (lower row of x' first) is the order of the corpus rows because rows ascends.  The
// certificate's X bounds the norms of all of x, a superset of x'.  With o.rows set the routes run the select with id_offset 0
// and dense_map_ids_kernel (dense_search.hip) turns the nq x k rows of x' into id_offset + rows[.] after V::finish; -1 stays.
int dense_launch_map_ids(rc_handle_t h, int64_t* ids, int64_t n, const int64_t* rows, int64_t id_offset, hipStream_t s);

// the end of both routes
template <typename V>
static int dense_finish(rc_handle_t h, const dense_operands& o, float* scores, int64_t* ids, int64_t n, int64_t id_offset,
                        hipStream_t s) {
    const int rc = V::finish(h, scores, n, s);
    if (rc != RC_OK || !o.rows) return rc;
    return dense_launch_map_ids(h, ids, n, o.rows, id_offset, s);
}

// the exact route: full score rows of L.qx queries at a time, then the radix select.  N: the rows searched (ns with o.rows)
template <typename V>
static int dense_exact(rc_handle_t h, const dense_operands& o, const typename dense_storage<V>::type* x, int64_t ldx, int64_t N,
                       int D, const typename V::T* q, int nq, int k, int64_t id_offset, float* scores, int64_t* ids, char* w,
                       const dense_exact_layout& L, hipStream_t s) {
    float* sc = (float*)(w + L.sc);             // (the select's status word is never set: exactly min(k, N) keys are collected)
    for (int q0 = 0; q0 < nq; q0 += L.qx) {
        const int nx = nq - q0 < L.qx ? nq - q0 : L.qx;
        int rc = V::exact_rows(h, o, x, ldx, N, D, q + (int64_t)q0 * D, nx, sc, s);
        if (rc != RC_OK) return rc;
        rc = topk_exact_select(h, sc, N, nx, k, o.rows ? 0 : id_offset, w, L.sel, scores + (size_t)q0 * k, ids + (size_t)q0 * k, s);
        if (rc != RC_OK) return rc;
    }
    return dense_finish<V>(h, o, scores, ids, (int64_t)nq * k, id_offset, s);
}

// checked arguments (dense_search_entry).  N: the rows searched (ns with o.rows)
template <typename V>
static int dense_search_route(rc_handle_t h, const dense_operands& o, const typename dense_storage<V>::type* x, int64_t ldx,
                              int64_t N, int D, const typename V::T* q, int nq, const float* xnorm_max, int k, int64_t id_offset,
                              double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus, char* w, hipStream_t s) {
    if (dense_exact_route(N))
        return dense_exact<V>(h, o, x, ldx, N, D, q, nq, k, id_offset, scores, ids, w, dense_exact_ws(N, nq), s);
    const dense_fast_layout L = dense_fast_ws(N, nq);
    float* sample = (float*)(w + L.sample);
    float* thr = (float*)(w + L.thr);
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    const typename V::Q* qs;
    int rc = V::prepass(h, o, q, nq, D, w + L.total, &qs, s);
    if (rc != RC_OK) return rc;
    rc = V::template launch_gemm<DENSE_STORE>(h, o, x, ldx, N, L.S, L.S, qs, nq, D, nullptr, sample, nullptr, nullptr, s);
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_threshold(h, sample, L.S, nq, rc_adc_sample_rank(N, L.S, k, sel_slack), thr, s);
    if (rc != RC_OK) return rc;
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    rc = V::template launch_gemm<DENSE_FILTER>(h, o, x, ldx, N, N, 0, qs, nq, D, thr, nullptr, cnt, cand, s);
    if (rc != RC_OK) return rc;
    if constexpr (V::approximate) {
        rc = V::rescore(h, o, x, ldx, D, q, nq, cnt, cand, s);
        if (rc != RC_OK) return rc;
    }
    rc = rc_adc_launch_select(h, cand, cnt, nq, N, k, o.rows ? 0 : id_offset, scores, ids, status, s, qstatus);
    if (rc != RC_OK) return rc;
    if constexpr (V::approximate) {
        rc = V::certify(h, o, q, qs, nq, D, k, thr, xnorm_max, scores, status, qstatus, s);
        if (rc != RC_OK) return rc;
    }
    return dense_finish<V>(h, o, scores, ids, (int64_t)nq * k, id_offset, s);
}

// ---- the entries ------------------------------------------------------------------------------------------------------------
// The bodies of rc_dense*_search_exact and rc_dense*_search_q, and with sub = true of rc_dense*_search_rows_exact and
// rc_dense*_search_rows_q: the same search over the rows o.rows [ns] of the store.  The order of the checks is part of the C ABI.
//   whole store  shapes, then pointers and alignment (dense_check; a coded variant has a screen for any row pitch and is asked
//                for none), then a missing status / xsq / dec / xnorm_max, then the nq == 0 success, then the workspace
//   rows         RC_ESHAPE on N, k (or D), then RC_EINVAL for ns outside [1, N], then dense_check, then the pointers, rows among
//                them, then the nq == 0 success, then the workspace, sized by ns
// and only then device work.  rows is never read on the host: ascending, unique and in [0, N) is the caller's word.  Only a
// variant with V::subset has entries that say sub; the check refuses it for the others.
template <typename V>
static int dense_entry_check(rc_handle_t h, const dense_operands& o, const typename dense_storage<V>::type* x, int64_t ldx,
                             int64_t N, int D, const typename V::T* q, int nq, bool sub, int64_t ns, int k, const float* scores,
                             const int64_t* ids) {
    if (N > 0xFFFFFFFFll || k > ADC_CAND_CAP / 2 || D > V::max_d) return RC_ESHAPE;
    if (sub && (!V::subset || ns < 1 || ns > N)) return RC_EINVAL;
    const int crc = dense_check(h, x, ldx, N, D, q, nq, k, scores, ids, !V::coded);
    if (crc != RC_OK) return crc;
    return (sub && !o.rows) || (V::coded && !o.dec) ? RC_EINVAL : RC_OK;
}

template <typename V>
static int dense_exact_entry(rc_handle_t h, const typename dense_storage<V>::type* x, int64_t ldx, int64_t N, int D,
                             const typename V::T* q, int nq, const dense_operands& o, bool sub, int64_t ns, int k,
                             int64_t id_offset, float* scores, int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int crc = dense_entry_check<V>(h, o, x, ldx, N, D, q, nq, sub, ns, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (nq == 0) return RC_OK;
    const int64_t n = sub ? ns : N;
    const dense_exact_layout L = dense_exact_ws(n, nq);
    if (!ws || ws_bytes < L.sel.total) return RC_EWORKSPACE;
    return dense_exact<V>(h, o, x, ldx, n, D, q, nq, k, id_offset, scores, ids, (char*)ws, L, (hipStream_t)stream);
}

// o.xsq is read if V::l2, o.dec if V::coded, xnorm_max if V::approximate
template <typename V>
static int dense_search_entry(rc_handle_t h, const typename dense_storage<V>::type* x, int64_t ldx, int64_t N, int D,
                              const typename V::T* q, int nq, const dense_operands& o, const float* xnorm_max, bool sub,
                              int64_t ns, int k, int64_t id_offset, double sel_slack, float* scores, int64_t* ids, int* status,
                              int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int crc = dense_entry_check<V>(h, o, x, ldx, N, D, q, nq, sub, ns, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (!status || (V::l2 && !o.xsq) || (V::approximate && !xnorm_max)) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    const int64_t n = sub ? ns : N;
    if (!ws || ((uintptr_t)ws & (V::ws_align - 1)) || ws_bytes < dense_search_ws_bytes<V>(n, D, nq, k)) return RC_EWORKSPACE;
    return dense_search_route<V>(h, o, x, ldx, n, D, q, nq, xnorm_max, k, id_offset, sel_slack, scores, ids, status, qstatus,
                                 (char*)ws, (hipStream_t)stream);
}

// The body of rc_dense*_scores, the screen's raw values out [nq][N] (a test hook): shapes, then pointers (o.xsq, o.dec where the
// variant reads them), then the alignment where the screen needs it, then the nq == 0 success, then the pre-pass's workspace
// where the variant has one (ws, ws_bytes; the others pass none), then V::prepass into it and the screen's STORE form.
template <typename V>
static int dense_scores_entry(rc_handle_t h, const typename dense_storage<V>::type* x, int64_t ldx, int64_t N, int D,
                              const typename V::T* q, int nq, const dense_operands& o, float* out, void* ws, size_t ws_bytes,
                              rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll || D > V::max_d) return RC_ESHAPE;
    if (!h || !x || !q || (V::coded && !o.dec) || (V::l2 && !o.xsq) || !out || N <= 0 || D <= 0 || nq < 0 || ldx < D)
        return RC_EINVAL;
    if (V::screen_aligned && !dense_aligned(x, ldx, D, q)) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    const size_t extra = V::extra_ws_bytes(nq, D);
    if (extra && (!ws || ((uintptr_t)ws & (V::ws_align - 1)) || ws_bytes < extra)) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const typename V::Q* qs;
    const int rc = V::prepass(h, o, q, nq, D, (char*)ws, &qs, s);
    if (rc != RC_OK) return rc;
    return V::template launch_gemm<DENSE_STORE>(h, o, x, ldx, N, N, 0, qs, nq, D, nullptr, out, nullptr, nullptr, s);
}
