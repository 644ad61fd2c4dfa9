// What the three dense L2 searches share beyond dense_screen.h (dense_search_l2.hip: fp32 corpus, dense_search_l2_f16.hip: fp16
// corpus, dense_search_l2_bf16x3.hip: fp32 corpus, bf16x3 screen): the exact route's kernel over either storage type and the
// sign flip at the end.  Device code: each unit instantiates the storage type it searches, no -fgpu-rdc; the fp32 form is
// instantiated in dense_search_l2.hip alone and reached from the bf16x3 unit through dense_l2_exact_rows_f32.
#pragma once
#include "dense_screen.h"

// ---- the exact route's kernel ------------------------------------------------------------------------------------------------
// The matrix cores cannot compute a chain of squared differences: this is vector-ALU work, two lane-operations per (q, n, d),
// the subtraction and the fmaf.  grid: ceil(N / 128) blocks of 256 threads, two per CU.  A block owns 128 corpus rows and walks
// every tile of 64 queries (the corpus is read from HBM once per launch), K in chunks of 16 through LDS, double buffered, both
// tiles stored k-major: thread (tx = tid % 32, ty = tid / 32) owns rows 4 tx .. + 3 and queries 8 ty .. + 7 of the tiles, 32
// accumulators that each walk d ascending, and reads per k one 16-byte vector of corpus values (32 lanes: 512 contiguous bytes)
// and two of query values (broadcast) for 64 vector operations.  out [nq][N] = -d, the score rows topk_exact_select reads.
// T: the storage type of x and q, widened to fp32 on load (exact); the LDS tiles, the arithmetic and the order are the same.
// !PAD: 16-byte aligned rows, read with vector loads — fp32: D % 16 == 0 (dense_check); fp16: D % 8 == 0, ldx % 8 == 0, a
// vector is inside or outside the row and the part of the last K chunk past D is zero.  PAD reads element by element and pads
// K with zeros.  MAP (subset search): the matrix is x[rows], rows [N] ascending corpus rows: one rows[] load per thread at block
// start for the row's address; the output column stays the logical row.  !MAP never reads rows.
// (-O3 pairs the 32 independent subtractions and fmas of a k step into v_pk_add_f32 / v_pk_fma_f32: two IEEE operations per
// instruction with the roundings of the plain forms.  Forcing v_sub_f32 + v_fmac_f32 one by one was measured slower)
#define DENSE_L2_QT 64
#define DENSE_L2_XLD (DENSE_TILE + 4)                    // words per k of the corpus tile: 8 k apart is 32 banks apart
#define DENSE_L2_QLD (DENSE_L2_QT + 4)                   // words per k of the query tile: 4 k apart is 16 banks apart

// the !PAD loads of an fp16 loader thread at column k of its row: 8 corpus values, 4 query values, zeros past D
__device__ __forceinline__ void dense_l2_load_x(const _Float16* p, int k, int D, float* r) {
    if (k < D) {
        dense_load8(p, r);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = 0.f;
    }
}
__device__ __forceinline__ void dense_l2_load_q(const _Float16* p, int k, int D, float* r) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 v = {(_Float16)0, (_Float16)0, (_Float16)0, (_Float16)0};
    if (k < D) v = *reinterpret_cast<const h4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (float)v[i];
}

template <bool PAD, typename T, bool MAP = false>
__global__ __launch_bounds__(256, 2) void dense_l2_exact_kernel(const T* __restrict__ x, int64_t ldx, int64_t N,
                                                                const T* __restrict__ q, int nq, int D,
                                                                float* __restrict__ out, const int64_t* __restrict__ rows) {
    __shared__ __attribute__((aligned(16))) float sx[2][DENSE_KC * DENSE_L2_XLD];
    __shared__ __attribute__((aligned(16))) float sq[2][DENSE_KC * DENSE_L2_QLD];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: corpus thread -> (row tid / 2, 8 consecutive k), query thread -> (row tid / 4, 4 consecutive k)
    const int xr = tid >> 1, xk = (tid & 1) * 8, qr = tid >> 2, qk = (tid & 3) * 4;
    const T* xp = x + dense_corpus_row<MAP>((j0 + xr < N) ? j0 + xr : N - 1, N, 0, rows) * ldx;
    const int nkc = (D + DENSE_KC - 1) / DENSE_KC;
    for (int qt = 0; qt < nq; qt += DENSE_L2_QT) {
        const T* qp = q + (int64_t)((qt + qr < nq) ? qt + qr : nq - 1) * D;
        float acc[8][4];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][r] = 0.f;
        float rx[8], rq[4];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_KC;
            if constexpr (PAD) {
#pragma unroll
                for (int i = 0; i < 8; ++i) rx[i] = (k0 + xk + i < D) ? (float)xp[k0 + xk + i] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) rq[i] = (k0 + qk + i < D) ? (float)qp[k0 + qk + i] : 0.f;
            } else {
                if constexpr (sizeof(T) == 4) {
                    dense_load8(xp + k0 + xk, rx);
                    const float4 v = *reinterpret_cast<const float4*>(qp + k0 + qk);
                    rq[0] = v.x; rq[1] = v.y; rq[2] = v.z; rq[3] = v.w;
                } else {
                    dense_l2_load_x(xp + k0 + xk, k0 + xk, D, rx);
                    dense_l2_load_q(qp + k0 + qk, k0 + qk, D, rq);
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 8; ++i) sx[buf][(xk + i) * DENSE_L2_XLD + xr] = rx[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) sq[buf][(qk + i) * DENSE_L2_QLD + qr] = rq[i];
        };
        const bool act = qt + 8 * ty < nq;                           // this thread's 8 queries are not all padding
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
            if (act) {
#pragma unroll
                for (int k = 0; k < DENSE_KC; ++k) {
                    const float4 xv = *reinterpret_cast<const float4*>(&sx[buf][k * DENSE_L2_XLD + 4 * tx]);
                    const float4 qa = *reinterpret_cast<const float4*>(&sq[buf][k * DENSE_L2_QLD + 8 * ty]);
                    const float4 qb = *reinterpret_cast<const float4*>(&sq[buf][k * DENSE_L2_QLD + 8 * ty + 4]);
                    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
                    const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                    for (int a = 0; a < 8; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float t = qv[a] - xs[r];
                            acc[a][r] = __builtin_fmaf(t, t, acc[a][r]);
                        }
                }
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int qi = qt + 8 * ty + a;
            if (qi < nq) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t j = j0 + 4 * tx + r;
                    if (j < N) out[(int64_t)qi * N + j] = -acc[a][r];
                }
            }
        }
    }
}

// o.rows is read only if MAP: a template argument, as in dense_launch_gemm
template <typename T, bool MAP = false>
static int dense_l2_launch_exact_rows(rc_handle_t h, const dense_operands& o, const T* x, int64_t ldx, int64_t N, int D,
                                      const T* q, int nq, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((N + DENSE_TILE - 1) / DENSE_TILE));
    const bool vec = sizeof(T) == 4 ? D % DENSE_KC == 0
                                    : D % 8 == 0 && ldx % 8 == 0 && !((uintptr_t)x & 15u) && !((uintptr_t)q & 15u);
    if (vec)
        hipLaunchKernelGGL((dense_l2_exact_kernel<false, T, MAP>), grid, dim3(256), 0, s, x, ldx, N, q, nq, D, out, o.rows);
    else
        hipLaunchKernelGGL((dense_l2_exact_kernel<true, T, MAP>), grid, dim3(256), 0, s, x, ldx, N, q, nq, D, out, o.rows);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// -d -> d in place over the n output values: -0.0f -> +0.0f, the -inf of the padding -> +inf.  The finish of every L2 variant,
// defined once in dense_search_l2.hip.
int dense_l2_launch_negate(rc_handle_t h, float* v, int64_t n, hipStream_t s);

// dense_l2_launch_exact_rows<float>, the rows of rc_dense_l2_search_exact (through o.rows for a subset), for the other unit
// that searches an fp32 corpus; defined in dense_search_l2.hip.
int dense_l2_exact_rows_f32(rc_handle_t h, const dense_operands& o, const float* x, int64_t ldx, int64_t N, int D, const float* q,
                            int nq, float* out, hipStream_t s);
