// The round-1 screens of the flat ADC search (adc_search.hip, step 4b) on the canonical codes — the widths without a permuted
// image (M = 8, 12, 24) and the tests' A/B partners (RC_ADC_OLD_SCREEN, RC_ADC_VALU_SCREEN): the kernel that writes their byte
// tables, the VALU screen and the matrix-core screen.
#pragma once
#include "adc_common.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------ 4b. screening

// One block per query: per-m minimum, the common step Delta = max_m(range_m)/255, the integer threshold and
// the byte tables, written interleaved [group][m][c][QS] (group = query / QS) so the screen kernel copies one
// contiguous slab per block.
__global__ __launch_bounds__(RC_K) void adc_qlut_kernel(const float* __restrict__ lut, const float* __restrict__ thr,
                                                        int M, int QS, uint8_t* __restrict__ qlut,
                                                        int* __restrict__ tint) {
    __shared__ float lo_m[128], rng_m[128], ab_m[128];
    __shared__ float red_lo[4], red_hi[4];
    __shared__ float s_delta;
    const int qi = blockIdx.x, c = threadIdx.x;
    const float* lq = lut + (size_t)qi * M * RC_K;
    for (int m = 0; m < M; ++m) {
        const float v = lq[m * RC_K + c];
        float lo = v, hi = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o));
            hi = fmaxf(hi, __shfl_xor(hi, o));
        }
        if ((c & 63) == 0) { red_lo[c >> 6] = lo; red_hi[c >> 6] = hi; }
        __syncthreads();
        lo = fminf(fminf(red_lo[0], red_lo[1]), fminf(red_lo[2], red_lo[3]));
        hi = fmaxf(fmaxf(red_hi[0], red_hi[1]), fmaxf(red_hi[2], red_hi[3]));
        if (c == 0) { lo_m[m] = lo; rng_m[m] = hi - lo; ab_m[m] = fmaxf(fabsf(lo), fabsf(hi)); }
        __syncthreads();
    }
    if (c == 0) {
        const adc_table_sums sums = adc_table_summary(lo_m, rng_m, ab_m, M);
        s_delta = sums.delta;
        tint[qi] = adc_screen_tint(thr[qi], sums, M);
    }
    __syncthreads();
    const float delta = s_delta;
    uint8_t* dst = qlut + (size_t)(qi / QS) * M * RC_K * QS + (qi % QS);
    for (int m = 0; m < M; ++m) dst[((size_t)m * RC_K + c) * QS] = (uint8_t)adc_quant8(lq[m * RC_K + c], lo_m[m], delta);
}

// grid (query groups of QS, doc tiles).  LDS: [M][256] entries of QS bytes (uint2 for QS = 8, uint for 4).
template <int M, int QS>
__global__ __launch_bounds__(ADC_THREADS) void adc_screen_kernel(const uint8_t* __restrict__ codes, int64_t N,
                                                                 const uint8_t* __restrict__ qlut,
                                                                 const int* __restrict__ tint, int nq,
                                                                 unsigned* __restrict__ id_count,
                                                                 unsigned* __restrict__ ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using E = typename std::conditional<QS == 8, uint2, unsigned>::type;
    E* tab = reinterpret_cast<E*>(smem);
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * QS;
    {
        const uint4* src = reinterpret_cast<const uint4*>(qlut + (size_t)blockIdx.x * M * RC_K * QS);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (int i = tid; i < M * RC_K * QS / 16; i += ADC_THREADS) dst[i] = src[i];
    }
    int tq[QS];
#pragma unroll
    for (int t = 0; t < QS; ++t) tq[t] = (q0 + t < nq) ? tint[q0 + t] : INT_MAX;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.y * ADC_TILE_DOCS;
    const int64_t t1 = (t0 + ADC_TILE_DOCS < N) ? t0 + ADC_TILE_DOCS : N;
    // the row of the NEXT trip is loaded before the current one is scored (register double buffer), so the
    // code loads (L2 latency) overlap the 48 gathers of the current row
    auto load_row = [&](int64_t n, unsigned (&dst)[M / 4]) {
        adc_load_code_bytes<M>(codes + (n < t1 ? n : (t1 - 1)) * M, dst);
    };
    unsigned w[M / 4], wn[M / 4];
    load_row(t0 + tid, w);
    for (int64_t i0 = t0; i0 < t1; i0 += ADC_THREADS) {
        const int64_t n = i0 + tid;
        const bool live = n < t1;
        load_row(n + ADC_THREADS, wn);
        // Byte accumulation in packed 16-bit fields: one v_perm_b32 spreads bytes (0,2) of a gathered word into
        // the two halves of a dword, another bytes (1,3); plain 32-bit adds then accumulate two queries at
        // once (a field never exceeds 96*255 < 2^16, so no carry crosses).  4 full-rate VALU ops per 4 queries —
        // v_dot4_u32_u8 with a one-hot mask does one query per instruction at half rate (PMC: VALU-bound at
        // 11.5 instr/gather, 4 cycles each).
        unsigned pe[QS / 4], po[QS / 4];
#pragma unroll
        for (int u = 0; u < QS / 4; ++u) pe[u] = po[u] = 0u;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const unsigned c = (w[m >> 2] >> (8 * (m & 3))) & 0xFFu;
            const E v = tab[m * RC_K + c];
            if constexpr (QS == 8) {
                pe[0] += __builtin_amdgcn_perm(0u, v.x, 0x0C020C00u);
                po[0] += __builtin_amdgcn_perm(0u, v.x, 0x0C030C01u);
                pe[1] += __builtin_amdgcn_perm(0u, v.y, 0x0C020C00u);
                po[1] += __builtin_amdgcn_perm(0u, v.y, 0x0C030C01u);
            } else {
                pe[0] += __builtin_amdgcn_perm(0u, v, 0x0C020C00u);
                po[0] += __builtin_amdgcn_perm(0u, v, 0x0C030C01u);
            }
        }
        int acc[QS];   // query t = 4u + j: byte j of word u -> (j even ? pe : po)[u], field j/2
#pragma unroll
        for (int u = 0; u < QS / 4; ++u) {
            acc[4 * u + 0] = (int)(pe[u] & 0xFFFFu);
            acc[4 * u + 1] = (int)(po[u] & 0xFFFFu);
            acc[4 * u + 2] = (int)(pe[u] >> 16);
            acc[4 * u + 3] = (int)(po[u] >> 16);
        }
#pragma unroll
        for (int t = 0; t < QS; ++t) {
            const bool pass = live && (acc[t] >= tq[t]);
            const unsigned long long mask = __ballot(pass);
            if (mask) {  // wave-uniform
                const unsigned slot = adc_wave_append(mask, id_count + q0 + t);
                if (pass && slot < ADC_ID_CAP) ids[(size_t)(q0 + t) * ADC_ID_CAP + slot] = (unsigned)n;
            }
        }
#pragma unroll
        for (int j = 0; j < M / 4; ++j) w[j] = wn[j];
    }
}

// XCD-aware block remap (guide T1).  The dispatcher places workgroup b on XCD b % 8 and every XCD has a private L2; the
// grid is (query groups, row tiles) with the group index fastest, so by default the ~150 blocks that scan the same
// row tile land on all 8 XCDs and the tile is fetched from HBM once per XCD.  The bijective remap hands each XCD a
// contiguous range of (tile, group) pairs: all groups of a tile run on ONE XCD, whose L2 (4 MiB) keeps the 1.5 MiB tile.
__device__ __forceinline__ void adc_xcd_remap(unsigned& group, unsigned& tile) {
    const unsigned gx = gridDim.x, total = gx * gridDim.y;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    const unsigned q = total / 8u, r = total % 8u, xcd = lin % 8u;
    const unsigned virt = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + lin / 8u;
    group = virt % gx;
    tile = virt / gx;
}

// The same screen with the byte accumulation on the matrix cores (M % 8 == 0; 8 queries per group, 4 when M > 64).
// PMC on adc_screen_kernel<48,8>: 9.3e9 VALU instructions per 1200-query launch = 95 % of the kernel's VALU cycles,
// the LDS gathers active 12 of its 18 ms — the v_perm/v_add accumulation is the limiter.  Here a wave takes 32 rows;
// lanes l and l+32 share row (l & 31) and gather the two halves of its M codes.  Two gathered 8-byte entries (two
// sub-quantisers x 8 queries) ARE the 16-byte A operand of v_mfma_i32_32x32x32_i8 in lane-natural layout
// (A[row][t], t = 8 g + query); B is the constant selection matrix B[t][j] = [t % 8 == j], so
//     D[row][j] += sum_{g, half} entry_{g,half}[j]      — one MFMA folds 4 sub-quantisers of 32 rows x 8 queries
// (QS = 4: four 4-byte entries per lane, 8 sub-quantisers x 4 queries).
// The pairing of A and B bytes is by (half-wave, byte position), so it does not depend on how the hardware numbers k.
// VALU per gather drops from ~10 instructions to the address computation; results arrive as D: lane j (< 8) of each
// half-wave holds query j's sums for 16 rows (row = (r&3) + 8 (r>>2) + 4 (lane>>5)).  The MFMA is signed: bytes are
// staged as l - 128 and the integer threshold is lowered by 128 M.
typedef int adc_i32x4 __attribute__((ext_vector_type(4)));
typedef int adc_i32x16 __attribute__((ext_vector_type(16)));

template <int M, int QS>
__global__ __launch_bounds__(ADC_THREADS) void adc_screen_mfma_kernel(const uint8_t* __restrict__ codes, int64_t N,
                                                                      const uint8_t* __restrict__ qlut,
                                                                      const int* __restrict__ tint, int nq,
                                                                      unsigned* __restrict__ id_count,
                                                                      unsigned* __restrict__ ids) {
    constexpr int HM = M / 2, NW = HM / 4;                  // codes per half-wave, dwords of codes per lane
    constexpr int G = 16 / QS;                              // gathered entries per A operand (QS bytes each)
    static_assert((QS == 8 || QS == 4) && HM % G == 0 && HM % 4 == 0, "unsupported (M, QS)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    unsigned bgroup, btile;
    adc_xcd_remap(bgroup, btile);
    const int q0 = (int)bgroup * QS;
    {
        const uint4* src = reinterpret_cast<const uint4*>(qlut + (size_t)bgroup * M * RC_K * QS);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (int i = tid; i < M * RC_K * QS / 16; i += ADC_THREADS) {
            uint4 v = src[i];
            v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;   // l -> l - 128 (signed)
            dst[i] = v;
        }
    }
    const int l = tid & 63, wv = tid >> 6;
    const int d = l & 31, hh = l >> 5;
    int tq = INT_MAX;                                        // this lane's query (as the D column j = d)
    if (d < QS && q0 + d < nq) {
        const int t = tint[q0 + d];
        tq = (t == INT_MIN) ? INT_MIN : t - 128 * M;
    }
    adc_i32x4 bsel = {0, 0, 0, 0};                           // B[t][j = d] = [t % QS == d]
    if (d < QS) {
        const int one = 1 << (8 * (d & 3));
        if constexpr (QS == 8) {
            bsel[d >> 2] = one;
            bsel[2 + (d >> 2)] = one;
        } else {
            bsel[0] = bsel[1] = bsel[2] = bsel[3] = one;
        }
    }
    __syncthreads();
    const int64_t t0 = (int64_t)btile * ADC_TILE_DOCS;
    const int64_t t1 = (t0 + ADC_TILE_DOCS < N) ? t0 + ADC_TILE_DOCS : N;
    constexpr int NWAVES = ADC_THREADS / 64;
    const unsigned char* tabh = smem + (size_t)hh * HM * RC_K * QS;      // this half-wave's sub-quantisers
    auto load_row = [&](int64_t n, unsigned (&dst)[NW]) {
        adc_load_code_bytes<HM>(codes + (n < t1 ? n : (t1 - 1)) * M + hh * HM, dst);
    };
    unsigned w[NW], wn[NW];
    load_row(t0 + wv * 32 + d, w);
    for (int64_t i0 = t0 + wv * 32; i0 < t1; i0 += NWAVES * 32) {   // wave-uniform
        load_row(i0 + NWAVES * 32 + d, wn);
        adc_i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int n = 0; n < HM / G; ++n) {
            adc_i32x4 a;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int mm = G * n + g;
                const unsigned c = (w[mm >> 2] >> (8 * (mm & 3))) & 0xFFu;
                const unsigned char* e = tabh + ((size_t)mm * RC_K + c) * QS;
                if constexpr (QS == 8) {
                    const uint2 v = *reinterpret_cast<const uint2*>(e);
                    a[2 * g] = (int)v.x;
                    a[2 * g + 1] = (int)v.y;
                } else {
                    a[g] = (int)*reinterpret_cast<const unsigned*>(e);
                }
            }
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bsel, acc, 0, 0, 0);
        }
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) any |= (acc[r] >= tq);
        if (__ballot(any)) {                                  // rare: ~2e-4 of the (row, query) pairs pass
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t n = i0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (acc[r] >= tq && n < t1) {
                    const unsigned slot = atomicAdd(id_count + q0 + d, 1u);
                    if (slot < ADC_ID_CAP) ids[(size_t)(q0 + d) * ADC_ID_CAP + slot] = (unsigned)n;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = wn[j];
    }
}
