// The screen GEMM on the f16 matrix cores over an fp16 corpus, shared by the two searches that store fp16
// (dense_search_f16.hip: inner product, dense_search_l2_f16.hip: squared Euclidean distance).  Device code: each unit
// instantiates the forms it launches, no -fgpu-rdc.
#pragma once
#include "dense_screen.h"

typedef _Float16 dense_f16x8 __attribute__((ext_vector_type(8)));
#define DENSE_F16_KC 64                                  // halves of K per LDS stage: 128-byte rows, 8 chunks of 16 bytes

// grid: ceil(nrows / 128) blocks of 256 threads, two per CU (64 KB of LDS each).  Arguments as dense_gemm_kernel; x and q are
// fp16.  !PAD: D % 8 == 0, 16-byte aligned rows; PAD assembles its chunks element by element.  The block owns 128 corpus rows
// and walks every tile of 128 queries; tiling, operand map and epilogue of v_mfma_f32_16x16x32_f16 as laid out in
// dense_screen.h, one 16-byte LDS read per operand tile and K step.  (v_mfma_f32_32x32x16_f16 at 2 x 2 tiles per wave was
// measured slower, 28.0 ms against 27.1 ms per FILTER launch over 8 841 823 x 768, and is retired: DESIGN.md 4.9,
// profiles/dense_f16_form_ab.txt.)
// L2: the epilogue emits sigma = fmaf(2, dot, -xsq[row]), xsq [N] = the stored fp32 squared norm of every corpus row (a lane
// holds one corpus row per column tile: four values, loaded once per block).  !L2: xsq is unused.
// MAP (subset search): x is read through rows [N] as dense_gemm_body reads it, four rows[] loads per thread at block start
// and the four of dense_screen_load_nxs; !MAP never reads rows.
template <int MODE, bool PAD, bool L2 = false, bool MAP = false>
__global__ __launch_bounds__(256, 2) void dense_f16_gemm_kernel(const _Float16* __restrict__ x, int64_t ldx, int64_t N,
                                                             int64_t nrows, int64_t smap, const _Float16* __restrict__ q,
                                                             int nq, int D, const float* __restrict__ thr,
                                                             float* __restrict__ out, unsigned* __restrict__ cnt,
                                                             unsigned long long* __restrict__ cand,
                                                             const float* __restrict__ xsq,
                                                             const int64_t* __restrict__ rows) {
    constexpr int TM = 16, NT = 4, KS = 32;
    __shared__ __attribute__((aligned(16))) unsigned char dense_f16_smem[DENSE_SCREEN_LDS_BYTES];
    unsigned char* sa = dense_f16_smem;                                     // [2][128 rows][128 bytes] queries
    unsigned char* sb = dense_f16_smem + 2 * DENSE_SCREEN_OPERAND_BYTES;    // [2][128 rows][128 bytes] corpus
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l % TM, grp = l / TM;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> chunk lc = tid % 8 of rows tid / 8 + 32 i, i < 4 (8 threads read 128 contiguous bytes of a row)
    const int lrow = tid >> 3, lc = tid & 7;
    const _Float16* xp[4];
    int so[4];                                                             // swizzled LDS offsets of the four chunks
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t jl = (j0 + lrow + 32 * i < nrows) ? j0 + lrow + 32 * i : nrows - 1;
        xp[i] = x + dense_corpus_row<MAP>(jl, N, smap, rows) * ldx;
        so[i] = dense_screen_lds_off(lrow + 32 * i, lc);
    }
    float nxs[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (L2) dense_screen_load_nxs<MAP>(xsq, j0, wc, col, N, nrows, smap, nxs, rows);
    const int nkc = (D + DENSE_F16_KC - 1) / DENSE_F16_KC;
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        const _Float16* qp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qp[i] = q + (int64_t)((qt + lrow + 32 * i < nq) ? qt + lrow + 32 * i : nq - 1) * D;
        dense_f32x4 acc[NT][NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
        dense_f16x8 ra[4], rb[4];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_F16_KC + lc * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (PAD) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        ra[i][e] = (k0 + e < D) ? qp[i][k0 + e] : (_Float16)0;
                        rb[i][e] = (k0 + e < D) ? xp[i][k0 + e] : (_Float16)0;
                    }
                } else if (k0 < D) {                                        // D % 8 == 0: a chunk is inside or outside
                    ra[i] = *reinterpret_cast<const dense_f16x8*>(qp[i] + k0);
                    rb[i] = *reinterpret_cast<const dense_f16x8*>(xp[i] + k0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { ra[i][e] = (_Float16)0; rb[i][e] = (_Float16)0; }
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<dense_f16x8*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = ra[i];
                *reinterpret_cast<dense_f16x8*>(sb + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = rb[i];
            }
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
            const unsigned char* pb = sb + buf * DENSE_SCREEN_OPERAND_BYTES;
#pragma unroll
            for (int ks = 0; ks < DENSE_F16_KC / KS; ++ks) {
                dense_f16x8 fa[NT], fb[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    fa[t] = *reinterpret_cast<const dense_f16x8*>(pa + dense_screen_lds_off(wr * 64 + t * TM + col, (KS / 8) * ks + grp));
                    fb[t] = *reinterpret_cast<const dense_f16x8*>(pb + dense_screen_lds_off(wc * 64 + t * TM + col, (KS / 8) * ks + grp));
                }
#pragma unroll
                for (int a = 0; a < NT; ++a)
                    if (act[a])
#pragma unroll
                        for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        const float* s_thr = dense_screen_stage_thr<MODE>(sa, nkc, thr, qt, nq, tid);
        dense_screen_epilogue<MODE, L2>(acc, j0, wr, wc, col, grp, qt, nq, s_thr, nrows, out, cnt, cand, l, nxs);
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

static bool dense_f16_aligned(const void* x, int64_t ldx, const void* q, int D) {
    return D % 8 == 0 && ldx % 8 == 0 && !((uintptr_t)x & 15u) && !((uintptr_t)q & 15u);
}

// o.xsq is read only if L2, o.rows only if MAP: a template argument, as in dense_launch_gemm
template <int MODE, bool L2, bool MAP = false>
static int dense_f16_launch_gemm(rc_handle_t h, const dense_operands& o, const _Float16* x, int64_t ldx, int64_t N, int64_t nrows,
                                 int64_t smap, const _Float16* q, int nq, int D, const float* thr, float* out, unsigned* cnt,
                                 unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (dense_f16_aligned(x, ldx, q, D))
        hipLaunchKernelGGL((dense_f16_gemm_kernel<MODE, false, L2, MAP>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D,
                           thr, out, cnt, cand, o.xsq, o.rows);
    else
        hipLaunchKernelGGL((dense_f16_gemm_kernel<MODE, true, L2, MAP>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D,
                           thr, out, cnt, cand, o.xsq, o.rows);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
