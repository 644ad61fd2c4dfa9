// The screen GEMM on the int8 matrix cores over a corpus of 8-bit scalar-quantiser codes (dense_search_sq8.hip, and with the L2
// epilogue dense_search_l2_sq8.hip), and the query pre-pass that feeds it.  Device code: the unit instantiates the forms it launches, no -fgpu-rdc.
//
// Screen.  The store holds c'_d = c_d - 128 as int8; a row decodes to x^_d = fmaf(c'_d, step_d, mid_d).  With w_d = q_d step_d
// and bias_q = sum_d q_d mid_d the score is sum_d w_d c'_d + bias_q up to roundings.  The pre-pass quantises w to integers
//   v_d = rint(w_d / alpha_q),  alpha_q = max_d |w_d| / DENSE_I8_QMAX,  |v_d| <= DENSE_I8_QMAX = 127 * 256 + 127,
// and splits v_d = 256 h_d + l_d with h_d = floor((v_d + 128) / 256), l_d = v_d - 256 h_d.  Both limbs are int8:
//   l_d = ((v_d + 128) mod 256) - 128 is in [-128, 127] by construction, and
//   -32639 <= v_d <= 32639 gives -32511 <= v_d + 128 <= 32767, hence -127 <= h_d <= 127.
// (A cap of 32767 would not do: rint(32767 / 256) = 128.)  The GEMM accumulates A_h = sum_d h_d c'_d and A_l = sum_d l_d c'_d
// in exact int32 (|h c'|, |l c'| <= 2^14 and D <= 65536 = DENSE_I8_MAX_D: |A| <= 2^30) and its epilogue emits
//   s~ = fmaf(alpha_q, fmaf(256, (float)A_h, (float)A_l), bias_q).
// The only error that is not a rounding is |w_d - alpha_q v_d| <= alpha_q / 2 per dimension: the bound is in
// dense_search_sq8.hip.
#pragma once
#include "dense_screen.h"

typedef int dense_i32x4 __attribute__((ext_vector_type(4)));
#define DENSE_I8_QMAX 32639                              // 127 * 256 + 127: the largest |v_d|
#define DENSE_I8_MAX_D 65536                             // 128 * 128 * D < 2^31: the int32 accumulators cannot overflow
#define DENSE_I8_KC 64                                   // bytes of K per LDS stage: one v_mfma_i32_16x16x64_i8 step
// LDS: the query operand is a tile of dense_screen.h (128 rows of 128 bytes: chunks 0 - 3 = k = 16 c .. + 15 of the high limb,
// 4 - 7 the same k of the low limb), the corpus operand 128 rows of 64 bytes; two buffers each: 48 KB, two blocks per CU.
#define DENSE_I8_CORPUS_BYTES (DENSE_TILE * DENSE_I8_KC)
#define DENSE_I8_LDS_BYTES (2 * DENSE_SCREEN_OPERAND_BYTES + 2 * DENSE_I8_CORPUS_BYTES)

// byte offset of the 16-byte chunk c < 4 of corpus tile row `row`: XOR swizzle with (row / 4) % 4.  Four rows share 256 bytes =
// all 64 banks, and 16 lanes that hold 16 consecutive rows of one chunk index (a quarter of a ds_read_b128 of the 16x16x64
// operand map) cover all 64 banks once: row % 4 picks the 64-byte quarter, (row / 4) % 4 ^ c the chunk inside it.
__device__ __forceinline__ int dense_i8_lds_off(int row, int c) { return row * 64 + ((c ^ ((row >> 2) & 3)) << 4); }

static inline int dense_i8_dpad(int D) { return (D + DENSE_I8_KC - 1) / DENSE_I8_KC * DENSE_I8_KC; }

// the pre-pass's part of the workspace: alpha [nq] fp32, bias [nq] fp32, then the two limb planes [2][nq][Dp] int8, Dp = D
// rounded up to a whole K stage, columns D .. Dp - 1 zero
struct dense_i8_query_layout { size_t alpha, bias, planes, total; int Dp; };
static inline dense_i8_query_layout dense_i8_query_ws(int nq, int D) {
    dense_i8_query_layout L;
    L.Dp = dense_i8_dpad(D);
    size_t o = 0;
    L.alpha = o;  o += rc_align_up((size_t)nq * sizeof(float), 256);
    L.bias = o;   o += rc_align_up((size_t)nq * sizeof(float), 256);
    L.planes = o; o += rc_align_up(2 * (size_t)nq * (size_t)L.Dp, 256);
    L.total = o;
    return L;
}

// the larger of two values, a NaN if either is one
__device__ __forceinline__ float dense_i8_max_nan(float a, float b) { return (a != a || b <= a) ? a : b; }

// grid: nq blocks of 256 threads.  dec: [2][D] fp32, row 0 = step, row 1 = mid.  Writes alpha, bias and the planes of query
// blockIdx.x.  w_d = q_d * step_d in fp32; bias = sum_d q_d mid_d in fp64 (the order of the block reduction), rounded once;
// v_d = rint(w_d / alpha) in fp64, clamped to +-DENSE_I8_QMAX (a normal alpha is within 2^-24 of the ratio and the largest
// quotient rounds to QMAX itself: the clamp can bite only under a subnormal alpha, which the certificate refuses).  A query whose w is not finite, or whose alpha underflows to
// zero although some w_d is not, gets alpha = 0 and zero planes: nothing divides by zero, and the certificate refuses it.
static __global__ __launch_bounds__(256) void dense_i8_prepass_kernel(const float* __restrict__ q, int D, int Dp,
                                                                      const float* __restrict__ dec, int nq,
                                                                      float* __restrict__ alpha, float* __restrict__ bias,
                                                                      signed char* __restrict__ planes) {
    __shared__ float s_max[4];
    __shared__ double s_sum[4];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const float* qp = q + (int64_t)qi * D;
    const float* step = dec;
    const float* mid = dec + D;
    float wmax = 0.f;
    double b = 0.0;
    for (int d = tid; d < D; d += 256) {
        const float w = fabsf(qp[d] * step[d]);
        wmax = dense_i8_max_nan(wmax, w);
        b += (double)qp[d] * (double)mid[d];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        wmax = dense_i8_max_nan(wmax, __shfl_xor(wmax, o));
        b += __shfl_xor(b, o);
    }
    if ((tid & 63) == 0) { s_max[tid >> 6] = wmax; s_sum[tid >> 6] = b; }
    __syncthreads();
    wmax = s_max[0];
    for (int i = 1; i < 4; ++i) wmax = dense_i8_max_nan(wmax, s_max[i]);
    b = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    float a = wmax / (float)DENSE_I8_QMAX;
    if (!(wmax < INFINITY)) a = 0.f;                                    // inf or NaN
    if (tid == 0) { alpha[qi] = a; bias[qi] = (float)b; }
    signed char* ph = planes + (int64_t)qi * Dp;
    signed char* pl = planes + ((int64_t)nq + qi) * Dp;
    for (int d = tid; d < Dp; d += 256) {
        int v = 0;
        if (d < D && a > 0.f) {
            const double r = rint((double)(qp[d] * step[d]) / (double)a);
            v = r > (double)DENSE_I8_QMAX ? DENSE_I8_QMAX : r < -(double)DENSE_I8_QMAX ? -DENSE_I8_QMAX : (int)r;
        }
        const int hi = (v + 128) >> 8;                                  // floor: an arithmetic shift
        ph[d] = (signed char)hi;
        pl[d] = (signed char)(v - 256 * hi);
    }
}

static int dense_i8_launch_prepass(rc_handle_t h, const float* q, int nq, int D, const float* dec, char* tail, hipStream_t s) {
    const dense_i8_query_layout L = dense_i8_query_ws(nq, D);
    hipLaunchKernelGGL(dense_i8_prepass_kernel, dim3((unsigned)nq), dim3(256), 0, s, q, D, L.Dp, dec, nq, (float*)(tail + L.alpha),
                       (float*)(tail + L.bias), (signed char*)(tail + L.planes));
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// grid: ceil(nrows / 128) blocks of 256 threads, two per CU (48 KB of LDS each).  Arguments as dense_gemm_kernel, except that
// x holds int8 codes and the queries arrive as the pre-pass left them (alpha, bias, planes [2][nq][Dp]).  !PAD: D % 16 == 0 and
// 16-byte aligned corpus rows; PAD assembles the corpus chunks byte by byte.  The block owns 128 corpus rows and walks every
// tile of 128 queries; wave (wr, wc) owns 64 queries x 64 rows as 4 x 4 tiles of v_mfma_i32_16x16x64_i8 with two accumulators
// each (high and low limb); lane l holds k = 16 (l / 16) .. + 15 of row l % 16 of every operand, one 16-byte LDS read per
// operand tile, limb and K step; result element r of lane l is corpus row l % 16 and query 4 (l / 16) + r of the tile.
// L2 (dense_search_l2_sq8.hip): the epilogue emits sigma = fmaf(2, s~, -xsq[row]), xsq [N] = the stored fp32 squared norm of
// every decoded corpus row (a lane holds one corpus row per column tile: four values, loaded once per block by
// dense_screen_load_nxs, at the mapped row of the strided sample).  !L2: xsq is unused.
template <int MODE, bool PAD, bool L2 = false>
__global__ __launch_bounds__(256, 2) void dense_i8_gemm_kernel(const signed char* __restrict__ x, int64_t ldx, int64_t N,
                                                               int64_t nrows, int64_t smap,
                                                               const signed char* __restrict__ planes,
                                                               const float* __restrict__ alpha, const float* __restrict__ bias,
                                                               int nq, int D, int Dp, const float* __restrict__ thr,
                                                               float* __restrict__ out, unsigned* __restrict__ cnt,
                                                               unsigned long long* __restrict__ cand,
                                                               const float* __restrict__ xsq) {
    constexpr int TM = 16, NT = 4;
    __shared__ __attribute__((aligned(16))) unsigned char dense_i8_smem[DENSE_I8_LDS_BYTES];
    __shared__ float s_thr[DENSE_TILE], s_alpha[DENSE_TILE], s_bias[DENSE_TILE];
    unsigned char* sa = dense_i8_smem;                                      // [2][128 rows][128 bytes] query limbs
    unsigned char* sb = dense_i8_smem + 2 * DENSE_SCREEN_OPERAND_BYTES;     // [2][128 rows][64 bytes] corpus codes
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l % TM, grp = l / TM;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping, queries: thread -> chunk qc = tid % 8 of rows tid / 8 + 32 i, i < 4; corpus: chunk xc = tid % 4 of rows
    // tid / 4 + 64 i, i < 2 (4 threads read 64 contiguous bytes of a row)
    const int qrow = tid >> 3, qc = tid & 7;
    const int xr = tid >> 2, xc = tid & 3;
    const signed char* xp[2];
    int sox[2], soq[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t jl = (j0 + xr + 64 * i < nrows) ? j0 + xr + 64 * i : nrows - 1;
        const int64_t xrow = smap ? (int64_t)((uint64_t)jl * (uint64_t)N / (uint64_t)smap) : jl;
        xp[i] = x + xrow * ldx;
        sox[i] = dense_i8_lds_off(xr + 64 * i, xc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) soq[i] = dense_screen_lds_off(qrow + 32 * i, qc);
    float nxs[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (L2) dense_screen_load_nxs(xsq, j0, wc, col, N, nrows, smap, nxs);
    const int nkc = Dp / DENSE_I8_KC;
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        const signed char* qp[4];                                          // this thread's limb plane, at its chunk's first k
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qi = (qt + qrow + 32 * i < nq) ? qt + qrow + 32 * i : nq - 1;
            qp[i] = planes + ((int64_t)(qc >> 2) * nq + qi) * Dp + (qc & 3) * 16;
        }
        if (tid < DENSE_TILE) {
            const int qi = qt + tid < nq ? qt + tid : nq - 1;
            s_alpha[tid] = alpha[qi];
            s_bias[tid] = bias[qi];
            if constexpr (MODE == DENSE_FILTER) s_thr[tid] = (qt + tid < nq) ? thr[qt + tid] : INFINITY;
        }
        dense_i32x4 acch[NT][NT], accl[NT][NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) { acch[a][b][r] = 0; accl[a][b][r] = 0; }
        dense_i32x4 ra[4], rb[2];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_I8_KC;
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const dense_i32x4*>(qp[i] + k0);     // Dp: whole stages
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int kx = k0 + xc * 16;
                if constexpr (PAD) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        unsigned u = 0;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (kx + 4 * w + e < D) u |= (unsigned)(unsigned char)xp[i][kx + 4 * w + e] << (8 * e);
                        rb[i][w] = (int)u;
                    }
                } else if (kx < D) {                                        // D % 16 == 0: a chunk is inside or outside
                    rb[i] = *reinterpret_cast<const dense_i32x4*>(xp[i] + kx);
                } else {
                    rb[i] = dense_i32x4{0, 0, 0, 0};
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<dense_i32x4*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + soq[i]) = ra[i];
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<dense_i32x4*>(sb + buf * DENSE_I8_CORPUS_BYTES + sox[i]) = rb[i];
        };
        // query tiles that hold only padding skip their MFMAs, wave-uniformly (a call with <= 32 queries issues a quarter of
        // the matrix work and is bounded by the corpus read)
        bool act[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) act[a] = qt + wr * 64 + a * TM < nq;
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
            const unsigned char* pa = sa + buf * DENSE_SCREEN_OPERAND_BYTES;
            const unsigned char* pb = sb + buf * DENSE_I8_CORPUS_BYTES;
            dense_i32x4 fb[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
                fb[t] = *reinterpret_cast<const dense_i32x4*>(pb + dense_i8_lds_off(wc * 64 + t * TM + col, grp));
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a]) {
                    const int row = wr * 64 + a * TM + col;
                    const dense_i32x4 fh = *reinterpret_cast<const dense_i32x4*>(pa + dense_screen_lds_off(row, grp));
                    const dense_i32x4 fl = *reinterpret_cast<const dense_i32x4*>(pa + dense_screen_lds_off(row, 4 + grp));
#pragma unroll
                    for (int b = 0; b < NT; ++b) {
                        acch[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fh, fb[b], acch[a][b], 0, 0, 0);
                        accl[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fl, fb[b], accl[a][b], 0, 0, 0);
                    }
                }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int64_t j = j0 + wc * 64 + b * TM + col;
            const bool jv = j < nrows;
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qo = wr * 64 + a * TM + 4 * grp + r;
                    const float t = __builtin_fmaf(256.f, (float)acch[a][b][r], (float)accl[a][b][r]);
                    float sc = __builtin_fmaf(s_alpha[qo], t, s_bias[qo]);
                    if constexpr (L2) sc = __builtin_fmaf(2.f, sc, nxs[b]);
                    dense_emit<MODE, 16>(sc, j, jv, qt + qo, nq, MODE == DENSE_FILTER ? s_thr[qo] : 0.f, nrows, out, cnt, cand, l);
                }
        }
        __syncthreads();                                           // the next query tile overwrites buffer 0 and the side values
    }
}

static bool dense_i8_aligned(const void* x, int64_t ldx, int D) { return D % 16 == 0 && ldx % 16 == 0 && !((uintptr_t)x & 15u); }

// qs: the pre-pass's part of the workspace (dense_i8_query_ws), 16-byte aligned; o.xsq is read only if L2
template <int MODE, bool L2 = false>
static int dense_i8_launch_gemm(rc_handle_t h, const dense_operands& o, const signed char* x, int64_t ldx, int64_t N,
                                int64_t nrows, int64_t smap, const char* qs, int nq, int D, const float* thr, float* out,
                                unsigned* cnt, unsigned long long* cand, hipStream_t s) {
    const dense_i8_query_layout L = dense_i8_query_ws(nq, D);
    const signed char* planes = (const signed char*)(qs + L.planes);
    const float* alpha = (const float*)(qs + L.alpha);
    const float* bias = (const float*)(qs + L.bias);
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (dense_i8_aligned(x, ldx, D))
        hipLaunchKernelGGL((dense_i8_gemm_kernel<MODE, false, L2>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, planes, alpha,
                           bias, nq, D, L.Dp, thr, out, cnt, cand, o.xsq);
    else
        hipLaunchKernelGGL((dense_i8_gemm_kernel<MODE, true, L2>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, planes, alpha,
                           bias, nq, D, L.Dp, thr, out, cnt, cand, o.xsq);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
