// The bf16x3 screen GEMM over an fp32 corpus, shared by the two searches that screen with it (dense_search_bf16x3.hip: inner
// product, dense_search_l2_bf16x3.hip: squared Euclidean distance), its query split pre-pass and the constants of the part of
// the certificate's bound that belongs to the screen's dot product.  Device code: each unit instantiates the forms it
// launches, no -fgpu-rdc.
//
// Screen.  Every fp32 operand a is split a = a_h + a_l + r with round-to-nearest-even conversions (v_cvt_pk_bf16_f32):
//   a_h = bf16(a),  a_l = bf16(a - a_h)   (the subtraction is exact in fp32: a - a_h is the low 16 bits of a's significand),
// and s~ = sum_d (q_h x_h + q_h x_l + q_l x_h): three bf16 MFMAs per K step into one fp32 accumulator.  A product of two bf16
// values has 16 significant bits: exact in fp32 unless it underflows.  The corpus is split while it is staged global -> LDS
// (no second copy in HBM); the queries are split once per call into two bf16 planes in the workspace, zero-padded to a
// multiple of 32 columns (dense_bf16x3_split_kernel: the bytes of q again).
#pragma once
#include "dense_screen.h"

typedef __bf16 dense_bf16x8 __attribute__((ext_vector_type(8)));
#define DENSE_B3_KC 32                                   // K per LDS stage: one v_mfma_f32_16x16x32_bf16 step
// one operand's tile row (dense_screen.h): 128 bytes = [32 bf16 high plane | 32 bf16 low plane]; chunks 0 - 3 hold
// k = 8c .. 8c + 7 of the high plane, 4 - 7 the same k of the low plane
#define DENSE_B3_C_SUM 8.0                               // E_rel = (C_SUM D_pad 2^-24 + C_SPLIT 2^-16) ||q|| X
#define DENSE_B3_C_SPLIT 4.0
// E_abs = C_SUB sqrt(D_pad) (||q|| + X) + C_UNDER D_pad, for hardware that does not flush.  Measured on the MI355X (the subnormal
// families of the screen-error test, tests/test_dense_bf16x3.py): neither v_cvt_pk_bf16_f32 nor
// v_mfma_f32_16x16x32_bf16 flushes — fp32-subnormal rows score ~7e-38 with an error of 3.5e-40, at most 0.21 E_q, where a flushed
// operand would lose the whole score; values whose low parts are bf16 subnormals stay below 0.06 E_q.
#define DENSE_B3_C_SUB 0x1p-133
#define DENSE_B3_C_UNDER 0x1p-147
#define DENSE_B3_MAX_D 65536                             // the certificate's second-order terms are bounded up to here

__device__ __forceinline__ void dense_b3_split8(const float* a, dense_bf16x8& h, dense_bf16x8& l) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 hi = (__bf16)a[e];                  // round to nearest even
        h[e] = hi;
        l[e] = (__bf16)(a[e] - (float)hi);               // exact difference, rounded once
    }
}

// grid: ceil(nq * (D32 / 8) / 256) blocks of 256 threads; thread -> 8 consecutive columns of one query.  qs: [2][nq][D32] bf16,
// plane 0 = q_h, plane 1 = q_l, columns D .. D32 - 1 zero.  (static: not a template, and two units of one library include it.)
static __global__ __launch_bounds__(256) void dense_bf16x3_split_kernel(const float* __restrict__ q, int nq, int D, int D32,
                                                                 __bf16* __restrict__ qs) {
    const int cpr = D32 / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)nq * cpr) return;
    const int row = (int)(i / cpr), k0 = (int)(i % cpr) * 8;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (k0 + e < D) ? q[(int64_t)row * D + k0 + e] : 0.f;
    dense_bf16x8 h, l;
    dense_b3_split8(a, h, l);
    *reinterpret_cast<dense_bf16x8*>(qs + (int64_t)row * D32 + k0) = h;
    *reinterpret_cast<dense_bf16x8*>(qs + ((int64_t)nq + row) * D32 + k0) = l;
}

// grid: ceil(nrows / 128) blocks of 256 threads, two per CU (64 KB of LDS each).  Arguments as dense_gemm_kernel, except that
// the queries arrive split: qs [2][nq][D32] (dense_bf16x3_split_kernel).  !PAD: D % 8 == 0 and 16-byte aligned corpus rows; PAD
// reads the corpus element by element.  The block owns 128 corpus rows and walks every tile of 128 queries; wave (wr, wc) owns
// 64 queries x 64 rows as 4 x 4 tiles of v_mfma_f32_16x16x32_bf16 (tiling, operand map and epilogue as laid out in
// dense_screen.h), three per tile and K step, one 16-byte LDS read per operand tile, plane and K step.
// L2: the epilogue emits sigma~ = fmaf(2, s~, -xsq[row]), xsq [N] = the stored fp32 squared norm of every corpus row (a lane
// holds one corpus row per column tile: four values, loaded once per block, at the mapped row in the pass over the strided
// sample).  !L2: xsq is unused.
template <int MODE, bool PAD, bool L2 = false>
__global__ __launch_bounds__(256, 2) void dense_bf16x3_gemm_kernel(const float* __restrict__ x, int64_t ldx, int64_t N,
                                                                int64_t nrows, int64_t smap, const __bf16* __restrict__ qs,
                                                                int nq, int D, int D32, const float* __restrict__ thr,
                                                                float* __restrict__ out, unsigned* __restrict__ cnt,
                                                                unsigned long long* __restrict__ cand,
                                                                const float* __restrict__ xsq) {
    constexpr int TM = 16, NT = 4;
    __shared__ __attribute__((aligned(16))) unsigned char dense_b3_smem[DENSE_SCREEN_LDS_BYTES];
    unsigned char* sa = dense_b3_smem;                                      // [2][128 rows][128 bytes] queries
    unsigned char* sb = dense_b3_smem + 2 * DENSE_SCREEN_OPERAND_BYTES;         // [2][128 rows][128 bytes] corpus
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l % TM, grp = l / TM;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> k = 8 lc .. 8 lc + 7 of rows tid / 4 + 64 i, i < 2 (4 threads read 128 contiguous bytes of fp32)
    const int lrow = tid >> 2, lc = tid & 3;
    const float* xp[2];
    int so[2];                                                             // swizzled LDS offsets of the high-plane chunks
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t jl = (j0 + lrow + 64 * i < nrows) ? j0 + lrow + 64 * i : nrows - 1;
        const int64_t xrow = smap ? (int64_t)((uint64_t)jl * (uint64_t)N / (uint64_t)smap) : jl;
        xp[i] = x + xrow * ldx;
        so[i] = dense_screen_lds_off(lrow + 64 * i, lc);
    }
    float nxs[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (L2) dense_screen_load_nxs(xsq, j0, wc, col, N, nrows, smap, nxs);
    // the low-plane chunk 4 + lc of the same row: (4 + lc) ^ m = (lc ^ m) ^ 4 for any 3-bit m
    const int nkc = (D + DENSE_B3_KC - 1) / DENSE_B3_KC;                    // == D32 / 32
    const __bf16* ql = qs + (int64_t)nq * D32;
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        int64_t qo_[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) qo_[i] = (int64_t)((qt + lrow + 64 * i < nq) ? qt + lrow + 64 * i : nq - 1) * D32 + lc * 8;
        dense_f32x4 acc[NT][NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
        dense_bf16x8 rah[2], ral[2];
        float rb[2][8];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_B3_KC + lc * 8;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                rah[i] = *reinterpret_cast<const dense_bf16x8*>(qs + qo_[i] + kc * DENSE_B3_KC);      // padded planes: in bounds
                ral[i] = *reinterpret_cast<const dense_bf16x8*>(ql + qo_[i] + kc * DENSE_B3_KC);
                if constexpr (PAD) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) rb[i][e] = (k0 + e < D) ? xp[i][k0 + e] : 0.f;
                } else if (k0 < D) {                                        // D % 8 == 0: a chunk is inside or outside
                    dense_load8(xp[i] + k0, rb[i]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) rb[i][e] = 0.f;
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                dense_bf16x8 h, lo;
                dense_b3_split8(rb[i], h, lo);
                *reinterpret_cast<dense_bf16x8*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = rah[i];
                *reinterpret_cast<dense_bf16x8*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + (so[i] ^ 64)) = ral[i];
                *reinterpret_cast<dense_bf16x8*>(sb + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = h;
                *reinterpret_cast<dense_bf16x8*>(sb + buf * DENSE_SCREEN_OPERAND_BYTES + (so[i] ^ 64)) = lo;
            }
        };
        // query tiles that hold only padding skip their MFMAs, wave-uniformly
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
            const unsigned char* pb = sb + buf * DENSE_SCREEN_OPERAND_BYTES;
            dense_bf16x8 fah[NT], fal[NT], fbh[NT], fbl[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int oa = dense_screen_lds_off(wr * 64 + t * TM + col, grp), ob = dense_screen_lds_off(wc * 64 + t * TM + col, grp);
                fah[t] = *reinterpret_cast<const dense_bf16x8*>(pa + oa);
                fal[t] = *reinterpret_cast<const dense_bf16x8*>(pa + (oa ^ 64));
                fbh[t] = *reinterpret_cast<const dense_bf16x8*>(pb + ob);
                fbl[t] = *reinterpret_cast<const dense_bf16x8*>(pb + (ob ^ 64));
            }
            // the two small terms first, then q_h x_h: 16 independent accumulators between two MFMAs on the same one
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a])
#pragma unroll
                    for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fal[a], fbh[b], acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a])
#pragma unroll
                    for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fah[a], fbl[b], acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a])
#pragma unroll
                    for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fah[a], fbh[b], acc[a][b], 0, 0, 0);
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        const float* s_thr = dense_screen_stage_thr<MODE>(sa, nkc, thr, qt, nq, tid);
        dense_screen_epilogue<MODE, L2>(acc, j0, wr, wc, col, grp, qt, nq, s_thr, nrows, out, cnt, cand, l, nxs);
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

static inline int dense_b3_d32(int D) { return (D + 31) / 32 * 32; }
static inline size_t dense_b3_split_bytes(int nq, int D) { return rc_align_up((size_t)2 * (size_t)nq * (size_t)dense_b3_d32(D) * 2, 256); }

static int dense_b3_launch_split(rc_handle_t h, const float* q, int nq, int D, __bf16* qs, hipStream_t s) {
    const int D32 = dense_b3_d32(D);
    const int64_t n = (int64_t)nq * (D32 / 8);
    hipLaunchKernelGGL(dense_bf16x3_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, nq, D, D32, qs);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// o.xsq is read only if L2
template <int MODE, bool L2 = false>
static int dense_b3_launch_gemm(rc_handle_t h, const dense_operands& o, const float* x, int64_t ldx, int64_t N, int64_t nrows,
                                int64_t smap, const __bf16* qs, int nq, int D, const float* thr, float* out, unsigned* cnt,
                                unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    const int D32 = dense_b3_d32(D);
    if (D % 8 == 0 && ldx % 4 == 0 && !((uintptr_t)x & 15u))
        hipLaunchKernelGGL((dense_bf16x3_gemm_kernel<MODE, false, L2>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, qs, nq, D,
                           D32, thr, out, cnt, cand, o.xsq);
    else
        hipLaunchKernelGGL((dense_bf16x3_gemm_kernel<MODE, true, L2>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, qs, nq, D,
                           D32, thr, out, cnt, cand, o.xsq);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// What the two bf16x3 variants (inner product, L2) share: the split pre-pass into the tail of the workspace, the screen and
// the query values the certificate refuses.  Each unit's variant adds its metric's exact rows, finish and eq.
template <typename V, bool L2>
struct dense_b3_variant_base : dense_variant_defaults<V> {
    typedef float T;
    typedef __bf16 Q;
    static constexpr bool approximate = true;
    static constexpr bool l2 = L2;
    static constexpr unsigned ws_align = 16;             // the planes are read with 16-byte loads
    static size_t extra_ws_bytes(int nq, int D) { return dense_b3_split_bytes(nq, D); }
    static int prepass(rc_handle_t h, const dense_operands&, const float* q, int nq, int D, char* tail, const Q** qs,
                       hipStream_t s) {
        *qs = (const __bf16*)tail;                       // 16-byte aligned: the workspace is, and the fast layout is a multiple of 256
        return dense_b3_launch_split(h, q, nq, D, (__bf16*)tail, s);
    }
    template <int MODE, typename... A>
    static int launch_gemm(A... a) { return dense_b3_launch_gemm<MODE, L2>(a...); }
    // |v| >= 2^128 - 2^119 rounds to a bf16 inf; inf and NaN lie above it
    __device__ static bool refuse(float v, int D) {
        return (__float_as_uint(v) & 0x7FFFFFFFu) >= 0x7F7F8000u || D > DENSE_B3_MAX_D;
    }
};
