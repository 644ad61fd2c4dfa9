// What the three dense flat searches share beyond the fp32 GEMM of dense_gemm.h (dense_search.hip: fp32 corpus and screen,
// dense_search_f16.hip: fp16 corpus and f16 screen, dense_search_bf16x3.hip: fp32 corpus and bf16x3 screen): the route of a
// search, the pieces common to the two 16x16x32 screen GEMMs, the rescoring kernel and the certificate kernel.  Device code:
// every translation unit compiles its own copy, no -fgpu-rdc.
//
// The route (dense_search_route).  A variant V supplies the storage type, its screen GEMM, an optional query pre-pass and,
// if its screen only approximates the score (V::approximate), the bound E_q of its certificate.
//   Exact route (N <= DENSE_EXACT_MAX_N, and the queries the fast route gives up on): dense_gemm_kernel<STORE> (dense_gemm.h,
//   the fp32 matrix cores over rows widened on load, i.e. the chain itself) writes the full score rows of a chunk of queries,
//   then the 8-pass radix select over the 64-bit keys (rc_adc_launch_exact_select).  It terminates with the same answer for
//   any content (all rows identical, k >= N, ...).
//   Fast route (N > 4 S, S = min(N, 32768)):
//   0. V::prepass: bf16x3 splits the queries into two bf16 planes in the tail of the workspace; nothing for the others
//   1. screen<STORE> over the strided sample j -> row j N / S: s~ of the sample (fp32 screen: s~ = s, the chain)
//   2. adc_threshold_kernel (topk.hip): thr~[q] = the r-th best s~ of the sample, r by the ADC formula (rc_adc_sample_rank)
//   3. screen<FILTER> over all N rows: the key (s~, row) of every s~ >= thr~[q] -> q's candidate list
//   4. approximate only: dense_rescore_kernel replaces the score half of every candidate key by the chain
//   5. adc_select_kernel (rc_adc_launch_select): sort + emit; qstatus bit0 = fewer than min(k, N) candidates, bit1 = overflow
//   6. approximate only: dense_certify_kernel.  With t = the query's k-th exact score and |s~ - s| <= E_q for every row, a
//      row outside the list has s~ < thr~, hence s < thr~ + E_q: if t >= thr~ + E_q (everything in fp64, rounded upwards) no
//      such row can enter the top-k or tie with its last member and the answer is proven equal to the exact route's.
//      Otherwise qstatus bit2, "not certified": the caller repeats the query with another slack or takes the exact route.
#pragma once
#include "dense_gemm.h"

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

// the epilogue of a wave's 4 x 4 result tiles: dense_emit on every element
template <int MODE>
__device__ __forceinline__ void dense_screen_epilogue(const dense_f32x4 (&acc)[4][4], int64_t j0, int wr, int wc, int col,
                                                      int grp, int qt, int nq, const float* s_thr, int64_t nrows,
                                                      float* __restrict__ out, unsigned* __restrict__ cnt,
                                                      unsigned long long* __restrict__ cand, int l) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t j = j0 + wc * 64 + b * 16 + col;
        const bool jv = j < nrows;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qo = wr * 64 + a * 16 + 4 * grp + r;
                dense_emit<MODE, 16>(acc[a][b][r], j, jv, qt + qo, nq, MODE == DENSE_FILTER ? s_thr[qo] : 0.f, nrows, out, cnt,
                                     cand, l);
            }
    }
}

// ---- rescoring --------------------------------------------------------------------------------------------------------------
#define DENSE_RESCORE_QCHUNK 1024                        // query values staged in LDS

// grid: (nq, ADC_CAND_CAP / 256) blocks of 256 threads; one lane per candidate key of query blockIdx.x.  The key's score half
// (the screen's s~) is replaced by the chain: literal fmaf calls, d ascending, one accumulator, over the values widened to
// fp32 (exact).  VEC: 16-byte aligned rows.
template <bool VEC, typename T>
__global__ __launch_bounds__(256) void dense_rescore_kernel(const T* __restrict__ x, int64_t ldx, int D, const T* __restrict__ q,
                                                            const unsigned* __restrict__ cnt,
                                                            unsigned long long* __restrict__ cand) {
    __shared__ float sq[DENSE_RESCORE_QCHUNK];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const unsigned raw = cnt[qi];
    const unsigned n = raw > ADC_CAND_CAP ? ADC_CAND_CAP : raw;
    if (blockIdx.y * 256u >= n) return;                                // block-uniform
    const unsigned i = blockIdx.y * 256u + tid;
    const bool mine = i < n;
    unsigned long long* kp = cand + (size_t)qi * ADC_CAND_CAP + i;
    const unsigned row = mine ? 0xFFFFFFFFu - (unsigned)(*kp & 0xFFFFFFFFull) : 0u;
    const T* xp = x + (int64_t)row * ldx;
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
                    for (int e = 0; e < 8; ++e) s = __builtin_fmaf(sq[d + e], v[e], s);
                }
            }
            for (; d < dn; ++d) s = __builtin_fmaf(sq[d], (float)xp[d0 + d], s);
        }
    }
    if (mine) *kp = adc_exact_key(s, (int64_t)row);
}

template <typename T>
static int dense_launch_rescore(rc_handle_t h, const T* x, int64_t ldx, int D, const T* q, int nq, const unsigned* cnt,
                                unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)nq, ADC_CAND_CAP / 256);
    if (ldx % (16 / (int)sizeof(T)) == 0 && !((uintptr_t)x & 15u))
        hipLaunchKernelGGL((dense_rescore_kernel<true, T>), grid, dim3(256), 0, s, x, ldx, D, q, cnt, cand);
    else
        hipLaunchKernelGGL((dense_rescore_kernel<false, T>), grid, dim3(256), 0, s, x, ldx, D, q, cnt, cand);
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
// A variant V:
//   typedef T                      storage type of x and q
//   typedef Q                      what its screen reads as the query operand (T, or the bf16 planes of the pre-pass)
//   static constexpr bool approximate
//   static size_t extra_ws_bytes(nq, D)                   workspace after the fast layout, for the pre-pass
//   static int prepass(h, q, nq, D, tail, &qs, s)         qs = the screen's query operand (tail: that extra workspace)
//   static int launch_gemm<MODE>(h, x, ldx, N, nrows, smap, qs, nq, D, thr, out, cnt, cand, s)
//   static int exact(h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, w, L, s)
//   approximate: eq / refuse of dense_certify_kernel
static inline size_t dense_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_shape_ok(N, D, nq, k) ? dense_exact_ws(N, nq).sel.total : 0;
}
template <typename V>
static size_t dense_search_ws_bytes(int64_t N, int D, int nq, int k) {
    if (!dense_shape_ok(N, D, nq, k)) return 0;
    return dense_exact_route(N) ? dense_exact_ws(N, nq).sel.total : dense_fast_ws(N, nq).total + V::extra_ws_bytes(nq, D);
}

// checked arguments (dense_check, status, xnorm_max if approximate, nq > 0, a workspace of dense_search_ws_bytes<V>)
template <typename V>
static int dense_search_route(rc_handle_t h, const typename V::T* x, int64_t ldx, int64_t N, int D, const typename V::T* q,
                              int nq, const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores,
                              int64_t* ids, int* status, int* qstatus, char* w, hipStream_t s) {
    if (dense_exact_route(N)) return V::exact(h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, w, dense_exact_ws(N, nq), s);
    const dense_fast_layout L = dense_fast_ws(N, nq);
    float* sample = (float*)(w + L.sample);
    float* thr = (float*)(w + L.thr);
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    const typename V::Q* qs;
    int rc = V::prepass(h, q, nq, D, w + L.total, &qs, s);
    if (rc != RC_OK) return rc;
    rc = V::template launch_gemm<DENSE_STORE>(h, x, ldx, N, L.S, L.S, qs, nq, D, nullptr, sample, nullptr, nullptr, s);
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_threshold(h, sample, L.S, nq, rc_adc_sample_rank(N, L.S, k, sel_slack), thr, s);
    if (rc != RC_OK) return rc;
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    rc = V::template launch_gemm<DENSE_FILTER>(h, x, ldx, N, N, 0, qs, nq, D, thr, nullptr, cnt, cand, s);
    if (rc != RC_OK) return rc;
    if constexpr (V::approximate) {
        rc = dense_launch_rescore(h, x, ldx, D, q, nq, cnt, cand, s);
        if (rc != RC_OK) return rc;
    }
    rc = rc_adc_launch_select(h, cand, cnt, nq, N, k, id_offset, scores, ids, status, s, qstatus);
    if constexpr (V::approximate) {
        if (rc != RC_OK) return rc;
        hipLaunchKernelGGL(dense_certify_kernel<V>, dim3((unsigned)nq), dim3(64), 0, s, q, D, k, thr, xnorm_max, scores,
                           status, qstatus);
        RC_LAUNCH_CHECK(h);
    }
    return rc;
}
