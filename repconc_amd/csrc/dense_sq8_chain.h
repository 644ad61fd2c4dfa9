// The exact chain over rows of 8-bit scalar-quantiser codes decoded on the fly, shared by the two flat searches over codes
// (dense_search_sq8.hip: inner product, dense_search_l2_sq8.hip: squared Euclidean distance): the rescoring kernel of the fast
// route, the score rows of the exact route and the certificate kernel around the unit's bound.  L2: the step is
// dense_chain_step<true>, t = q - x^, fmaf(t, t, acc), and the value written is -d.  Device code: each unit instantiates the
// forms it launches, no -fgpu-rdc.
#pragma once
#include "dense_i8_gemm.h"
#include "dense_sq8.h"

typedef signed char dense_i8x16 __attribute__((ext_vector_type(16)));

// ---- rescoring --------------------------------------------------------------------------------------------------------------
// dense_rescore_kernel (dense_screen.h) over coded rows: grid (nq, ADC_CAND_CAP / 256) blocks of 256 threads, one lane per
// candidate key of query blockIdx.x; step, mid and the query are staged in LDS chunk by chunk.  VEC: 16-byte aligned rows.
template <bool VEC, bool L2 = false>
__global__ __launch_bounds__(256) void dense_sq8_rescore_kernel(const signed char* __restrict__ x, int64_t ldx, int D,
                                                                const float* __restrict__ dec, const float* __restrict__ q,
                                                                const unsigned* __restrict__ cnt,
                                                                unsigned long long* __restrict__ cand) {
    __shared__ float sq[DENSE_RESCORE_QCHUNK], ss[DENSE_RESCORE_QCHUNK], sm[DENSE_RESCORE_QCHUNK];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const unsigned raw = cnt[qi];
    const unsigned n = raw > ADC_CAND_CAP ? ADC_CAND_CAP : raw;
    if (blockIdx.y * 256u >= n) return;                                // block-uniform
    const unsigned i = blockIdx.y * 256u + tid;
    const bool mine = i < n;
    unsigned long long* kp = cand + (size_t)qi * ADC_CAND_CAP + i;
    const unsigned row = mine ? 0xFFFFFFFFu - (unsigned)(*kp & 0xFFFFFFFFull) : 0u;
    const signed char* xp = x + (int64_t)row * ldx;
    const float* qp = q + (int64_t)qi * D;
    float s = 0.f;
    for (int d0 = 0; d0 < D; d0 += DENSE_RESCORE_QCHUNK) {
        const int dn = D - d0 < DENSE_RESCORE_QCHUNK ? D - d0 : DENSE_RESCORE_QCHUNK;
        __syncthreads();
        for (int d = tid; d < dn; d += 256) { sq[d] = qp[d0 + d]; ss[d] = dec[d0 + d]; sm[d] = dec[D + d0 + d]; }
        __syncthreads();
        if (mine) {
            int d = 0;
            if constexpr (VEC) {
                for (; d + 16 <= dn; d += 16) {
                    const dense_i8x16 v = *reinterpret_cast<const dense_i8x16*>(xp + d0 + d);
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        s = dense_chain_step<L2>(sq[d + e], dense_sq8_decode(v[e], ss[d + e], sm[d + e]), s);
                }
            }
            for (; d < dn; ++d) s = dense_chain_step<L2>(sq[d], dense_sq8_decode(xp[d0 + d], ss[d], sm[d]), s);
        }
    }
    if (mine) *kp = adc_exact_key(L2 ? -s : s, (int64_t)row);
}

template <bool L2>
static int dense_sq8_launch_rescore(rc_handle_t h, const dense_operands& o, const signed char* x, int64_t ldx, int D,
                                    const float* q, int nq, const unsigned* cnt, unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)nq, ADC_CAND_CAP / 256);
    if (ldx % 16 == 0 && !((uintptr_t)x & 15u))
        hipLaunchKernelGGL((dense_sq8_rescore_kernel<true, L2>), grid, dim3(256), 0, s, x, ldx, D, o.dec, q, cnt, cand);
    else
        hipLaunchKernelGGL((dense_sq8_rescore_kernel<false, L2>), grid, dim3(256), 0, s, x, ldx, D, o.dec, q, cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ---- the exact route's score rows -------------------------------------------------------------------------------------------
#define DENSE_SQ8_ROWS_QB 4                              // queries that share a decoded value
// grid: (ceil(N / 256), ceil(nq / 4)) blocks of 256 threads; thread -> one corpus row and four queries: out [nq][N] = the chain
// of every pair (L2: -d).  A value is decoded once and feeds four chains.  Plain fp32: the exact route serves small corpora and
// the few queries the fast route gives up on.
template <bool L2 = false>
__global__ __launch_bounds__(256) void dense_sq8_rows_kernel(const signed char* __restrict__ x, int64_t ldx, int64_t N, int D,
                                                             const float* __restrict__ dec, const float* __restrict__ q, int nq,
                                                             float* __restrict__ out) {
    __shared__ float sq[DENSE_SQ8_ROWS_QB][DENSE_RESCORE_QCHUNK], ss[DENSE_RESCORE_QCHUNK], sm[DENSE_RESCORE_QCHUNK];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * DENSE_SQ8_ROWS_QB;
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    const bool mine = j < N;
    const signed char* xp = x + (mine ? j : N - 1) * ldx;
    float s[DENSE_SQ8_ROWS_QB];
#pragma unroll
    for (int b = 0; b < DENSE_SQ8_ROWS_QB; ++b) s[b] = 0.f;
    for (int d0 = 0; d0 < D; d0 += DENSE_RESCORE_QCHUNK) {
        const int dn = D - d0 < DENSE_RESCORE_QCHUNK ? D - d0 : DENSE_RESCORE_QCHUNK;
        __syncthreads();
        for (int d = tid; d < dn; d += 256) {
            ss[d] = dec[d0 + d];
            sm[d] = dec[D + d0 + d];
#pragma unroll
            for (int b = 0; b < DENSE_SQ8_ROWS_QB; ++b) sq[b][d] = q[(int64_t)(q0 + b < nq ? q0 + b : nq - 1) * D + d0 + d];
        }
        __syncthreads();
        for (int d = 0; d < dn; ++d) {
            const float v = dense_sq8_decode(xp[d0 + d], ss[d], sm[d]);
#pragma unroll
            for (int b = 0; b < DENSE_SQ8_ROWS_QB; ++b) s[b] = dense_chain_step<L2>(sq[b][d], v, s[b]);
        }
    }
    if (mine)
#pragma unroll
        for (int b = 0; b < DENSE_SQ8_ROWS_QB; ++b)
            if (q0 + b < nq) out[(int64_t)(q0 + b) * N + j] = L2 ? -s[b] : s[b];
}

template <bool L2>
static int dense_sq8_launch_exact_rows(rc_handle_t h, const dense_operands& o, const signed char* x, int64_t ldx, int64_t N,
                                       int D, const float* q, int nq, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)((nq + DENSE_SQ8_ROWS_QB - 1) / DENSE_SQ8_ROWS_QB));
    hipLaunchKernelGGL(dense_sq8_rows_kernel<L2>, grid, dim3(256), 0, s, x, ldx, N, D, o.dec, q, nq, out);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ---- certificate ------------------------------------------------------------------------------------------------------------
#define DENSE_SQ8_BIG 0x1p100f                           // the certificate's range: |values| below it, alpha above its inverse

// grid: nq blocks of 64 threads, as dense_certify_kernel.  cstat: [2] fp32 = C1, X.  Sets bit2 of status / qstatus[q] unless
// t >= thr~ + B::add(..) is proven; a NaN anywhere is "not certified".  B::add(D, alpha, w1, b1, ss, c1, X): what the unit's
// bound adds to thr~, in fp64 and pushed upwards, from alpha_q, W1 = sum_d |fl(q_d step_d)|, B1 = sum_d |q_d mid_d| and
// ss = sum_d q_d^2 as summed here (the unit's header says what they bound).
template <typename B>
__global__ __launch_bounds__(64) void dense_sq8_certify_kernel(const float* __restrict__ q, int D, int k,
                                                               const float* __restrict__ dec, const float* __restrict__ alpha,
                                                               const float* __restrict__ thr, const float* __restrict__ cstat,
                                                               const float* __restrict__ scores, int* __restrict__ status,
                                                               int* __restrict__ qstatus) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    const float* qp = q + (int64_t)qi * D;
    double ss = 0.0, w1 = 0.0, b1 = 0.0;
    int refused = 0, nonzero = 0;
    for (int d = lane; d < D; d += 64) {
        const float f = qp[d];
        const float w = fabsf(f * dec[d]);
        const double b = fabs((double)f * (double)dec[D + d]);
        refused |= !(fabsf(f) < DENSE_SQ8_BIG) || !(w < DENSE_SQ8_BIG) || !(b < (double)DENSE_SQ8_BIG);
        nonzero |= w > 0.f;
        ss += (double)f * (double)f;
        w1 += (double)w;
        b1 += b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o);
        w1 += __shfl_xor(w1, o);
        b1 += __shfl_xor(b1, o);
        refused |= __shfl_xor(refused, o);
        nonzero |= __shfl_xor(nonzero, o);
    }
    if (lane != 0) return;
    const float a = alpha[qi];
    refused |= D > DENSE_I8_MAX_D || (nonzero && !(a >= 1.f / DENSE_SQ8_BIG));
    const double sum = (double)thr[qi] + B::add(D, (double)a, w1, b1, ss, (double)cstat[0], (double)cstat[1]);
    const double bound = sum + fabs(sum) * 0x1p-30;
    const double t = (double)scores[(size_t)qi * k + (k - 1)];
    if (refused || !(t >= bound)) {
        atomicOr(status, 4);
        if (qstatus) atomicOr(qstatus + qi, 4);
    }
}

template <typename B>
static int dense_sq8_launch_certify(rc_handle_t h, const dense_operands& o, const float* q, const char* qs, int nq, int D, int k,
                                    const float* thr, const float* cstat, const float* scores, int* status, int* qstatus,
                                    hipStream_t s) {
    const float* alpha = (const float*)(qs + dense_i8_query_ws(nq, D).alpha);
    hipLaunchKernelGGL(dense_sq8_certify_kernel<B>, dim3((unsigned)nq), dim3(64), 0, s, q, D, k, o.dec, alpha, thr, cstat, scores,
                       status, qstatus);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ---- the variant ------------------------------------------------------------------------------------------------------------
// What the variants of the two searches over codes share (dense_screen.h), which is all but the L2 unit's finish: o.dec on every
// route, o.xsq in the screen if L2, the query pre-pass into the tail of the workspace.  B: the unit's bound
// (dense_sq8_certify_kernel).
template <typename V, bool L2, typename B>
struct dense_sq8_variant_base : dense_variant_defaults<V> {
    typedef float T;
    typedef signed char X;
    typedef char Q;                                      // the pre-pass's part of the workspace (dense_i8_query_ws)
    static constexpr bool approximate = true;
    static constexpr bool coded = true;
    static constexpr bool l2 = L2;
    static constexpr int max_d = DENSE_I8_MAX_D;
    static constexpr unsigned ws_align = 16;             // the planes are read with 16-byte loads
    static size_t extra_ws_bytes(int nq, int D) { return dense_i8_query_ws(nq, D).total; }
    static int prepass(rc_handle_t h, const dense_operands& o, const float* q, int nq, int D, char* tail, const Q** qs,
                       hipStream_t s) {
        *qs = tail;                                      // 16-byte aligned: the workspace is, and the fast layout is a multiple of 256
        return dense_i8_launch_prepass(h, q, nq, D, o.dec, tail, s);
    }
    template <int MODE, typename... A>
    static int launch_gemm(A... a) { return dense_i8_launch_gemm<MODE, L2>(a...); }
    static constexpr auto* exact_rows = &dense_sq8_launch_exact_rows<L2>;
    static constexpr auto* rescore = &dense_sq8_launch_rescore<L2>;
    static constexpr auto* certify = &dense_sq8_launch_certify<B>;
};

// rc_dense*_sq8_search_ws_counts: where the fast route's candidate counts lie in the workspace (0: the exact route has none)
template <typename V>
static int dense_search_ws_counts(int64_t N, int D, int nq, int k, size_t* cnt_off) {
    if (!cnt_off) return RC_EINVAL;
    *cnt_off = 0;
    if (!dense_variant_shape_ok<V>(N, D, nq, k)) return RC_ESHAPE;
    if (!dense_exact_route(N)) *cnt_off = dense_fast_ws(N, nq).cnt;
    return RC_OK;
}
