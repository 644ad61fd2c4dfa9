// Nearest-code assignment with the matrix cores as a SCREEN and the exact-order arithmetic as the JUDGE.
//
// Reference: RepCONC.quantize with use_constraint=False, models/repconc/modeling_repconc.py:49-52,66 — the index-build
// path for all 8.84 M passages.  Bit-exact codes need the reference's own fp32 rounding (sub, square, torch-CPU sum
// order; pq_distance.hip), which a GEMM cannot reproduce.  But the GEMM form
//     S[k,b] = ||c_k||^2 - 2 <c_k, x_b>            ( = d[k,b] - ||x_b||^2 up to rounding )
// is within a provable distance E of the reference's d (both measured from the real-number distance), so the
// reference's argmin is among the centroids with S <= S_min + 2E.  The MFMA pass keeps, per (row, sub-quantiser), the
// best and second-best S: when the gap exceeds the margin the best IS the reference's code; otherwise (~3e-3 of the
// pairs, and every exact tie) the pair is appended to a list and assign_redo_kernel recomputes it with the exact
// arithmetic and the first-minimum rule.  Output = reference codes, bit for bit (tests compare with the exact kernel
// and the oracle).
//
// Which MFMA.  v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate (64 cycles / instruction, sharing the pipe with the
// VALU epilogue: measured 19 ms per 4 M rows, 2.4x the exact kernel).  The bf16 XDL pipe is 16x faster and co-issues
// with the VALU, so the screen splits every fp32 operand in two bf16 pieces (round to nearest even, 8 significant bits
// each), v = vh + vl + rest, and takes three products  wh.xh + wh.xl + wl.xh  (w = -2c) accumulated in fp32.
// The split.  |v - vh| <= half a bf16 ulp of v <= 2^-8 |v|, so |vl| <= 2^-8 |v| (measured over a whole binade:
// 1.992 * 2^-9); the remainder v - vh is exact in fp32 and lies in a binade at most 2^-8 of v's, so
// |rest| <= half a bf16 ulp of it <= 2^-17 |v| (measured: 1.996 * 2^-18, e.g. at 0x3f8040c0).  The terms of E, each as
// a multiple of (||x||^2 + ||c||^2) >= 2 sum|c_j x_j| = sum|w_j x_j|:
//     dropped products  wl.xl + (wh + wl).xr + wr.x :  (2^-16 + 2^-17 + 2^-17) sum|w_j x_j| = 8 * 2^-18     3.052e-5
//       (tests/test_assign_screen.py builds rows and centroids whose dropped terms all have one sign: 3.01e-5)
//     the 4 tag bits (below) replace the low mantissa bits of a screened value <= 3 (||x||^2 + ||c||^2):
//       < 16 ulp = 2^-19 of it                                                                                5.73e-6
//     fp32 accumulation of 3*KP+6 terms (||c||^2 and the document offset below enter as 3 exact bf16 pieces each), each
//       <= 1 ulp of a partial sum <= 3 (||x||^2+||c||^2) (the rounding inside a bf16 MFMA is not documented: one ulp
//       per term, not half):                                                                    (3 KP + 7) 3.6e-7
//     ||c||^2 (fma chain) and the reference's own d: (dsub+2) 1.2e-7 each                       (2 dsub + 4) 1.2e-7
// => E = [3.63e-5 + (3 KP + 7) 3.6e-7 + (2 dsub + 4) 1.2e-7] (||x||^2 + max_k ||c_k||^2),  margin = 2 E
// (3.052e-5 + 5.73e-6 = 3.625e-5, rounded up; mf_margin below, rc_pq_assign_nearest_fast_margin returns it).  Until
// the split bound was corrected the first line read 3.1 * 2^-18 (unit round-off 2^-9 instead of 2^-8) and the constant
// 1.8e-5: the built inputs above used 71-75 % of that E with this one term at dsub 8 / 16, and the codes held only
// through the slack of the accumulation allowance.
//
// Mapping (v_mfma_f32_32x32x16_bf16, 32 cycles): D = A*B + C with A[i][kk] = piece of -2 c_{32 kt + i}[kk] (LDS, 16 B
// per lane), B[kk][j] = piece of x_{b0 + j}[kk] (registers); one more MFMA adds ||c||^2 (three pieces against 1.0) and a
// per-document offset ||x_b||^2 + margin (1.0 against its three pieces) — so every screened value is distance^2 + margin > 0,
// the float bits order like signed integers, and the epilogue may mix v_med3_f32 with v_min3_i32 (integer instructions
// need no canonicalisation of the bit-tagged operands).  Rows of D = centroids, columns = documents, so a lane holds 16
// centroids of ONE document per tile and the running (min, second min) needs no cross-lane traffic until the two
// half-waves merge once per sub-quantiser.  A wave owns 64 documents (two column sets): the A fragments of a centroid tile
// are read once for both, and the two accumulator tiles ping-pong so that the VALU epilogue of one overlaps the MFMAs of
// the next.  Epilogue per (document, centroid) pair: v_and_or (tag) + 1.25 instructions — candidates are folded in pairs,
// t = med3(m1, u1, u2), m2' = min(m2, t), m1' = min3(m1, u1, u2), and the compiler merges the m2 updates of two pairs
// into one min3 (round 1/2a: two v_med3 per candidate, 3 instructions in all).  The staged centroids (bf16 pieces, norms)
// are the same for every block: assign_prep_kernel writes them once per call and the blocks fetch them with
// global_load_lds_dwordx4 straight into the free LDS buffer (no registers, no conversion per block).
// [MI355X] 2^20 rows, M = 48: 2.29 ms = 458 M vectors/s (2.40-2.45 ms before the pair folding and the prepared
// centroids); VALU instructions per wave and sub-quantiser 1150 -> ~870, matrix pipe 35 % busy — what is left is not
// issue-bound on either pipe (waves wait ~45 % of their cycles: LDS operand reads ahead of every MFMA, one barrier per
// sub-quantiser).
#include "rc_common.h"

#include <type_traits>

typedef float mf_f32x16 __attribute__((ext_vector_type(16)));
typedef float mf_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mf_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mf_bf16x8 __attribute__((ext_vector_type(8)));

#define MF_COLS 32                 // documents per MFMA tile
#define MF_SETS 2                  // tiles (column sets) per wave
#define MF_WAVES 4
#define MF_ROWS_PER_BLOCK (MF_COLS * MF_SETS * MF_WAVES)

// exact reference distance (identical code to sqdist_exact in pq_distance.hip; duplicated because device functions
// do not link across translation units without -fgpu-rdc)
template <int DSUB>
__device__ __forceinline__ float mf_exact(const float* __restrict__ x, const float* __restrict__ c) {
    constexpr int NV = DSUB / 8, TAIL = DSUB % 8, FULL = NV / 4;
    float sq[DSUB];
#pragma unroll
    for (int j = 0; j < DSUB; ++j) {
        const float t = x[j] - c[j];
        sq[j] = t * t;
    }
    float a[8];
    if constexpr (FULL == 0) {
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            float s = sq[l];
#pragma unroll
            for (int v = 1; v < NV; ++v) s = s + sq[8 * v + l];
            a[l] = s;
        }
    } else {
        float acc[4][8];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                float s = sq[8 * q + l];
#pragma unroll
                for (int i = 1; i < FULL; ++i) s = s + sq[8 * (4 * i + q) + l];
                acc[q][l] = s;
            }
#pragma unroll
        for (int v = 4 * FULL; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < 8; ++l) acc[0][l] = acc[0][l] + sq[8 * v + l];
#pragma unroll
        for (int l = 0; l < 8; ++l) a[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
    }
    float r;
    if constexpr (TAIL == 0) {
        r = a[0];
#pragma unroll
        for (int l = 1; l < 8; ++l) r = r + a[l];
    } else {
        r = sq[NV * 8];
#pragma unroll
        for (int j = 1; j < TAIL; ++j) r = r + sq[NV * 8 + j];
#pragma unroll
        for (int l = 0; l < 8; ++l) r = r + a[l];
    }
    return r;
}

// min / second-min updates as two v_med3_f32: m2' = med3(m1, m2, u), m1' = med3(m1, u, -inf).  The target intrinsic
// needs no canonicalisation of the bit-tagged values and stays visible to the instruction scheduler (inline asm does
// not); -inf comes through an opaque SGPR, otherwise the compiler folds the second one into v_max + v_min (2 ops).
__device__ __forceinline__ float mf_opaque_neg_inf() {
    float v;
    asm volatile("s_mov_b32 %0, 0xff800000" : "=s"(v));
    return v;
}
__device__ __forceinline__ float mf_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

// (v0, v1) -> packed bf16 pair of the leading pieces and of the remainders (v_cvt_pk_bf16_f32, round to nearest even)
__device__ __forceinline__ void mf_split2(float v0, float v1, unsigned& hi, unsigned& lo) {
    const mf_f32x2 v = {v0, v1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, mf_bf16x2));
    const mf_f32x2 r = {v0 - __uint_as_float(hi << 16), v1 - __uint_as_float(hi & 0xFFFF0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, mf_bf16x2));
}

// rounding bound of the screen (file header): margin = 2 E, as a multiple of ||x||^2 + max_k ||c_k||^2
constexpr float mf_margin(int dsub) {
    const int kp = (dsub + 15) / 16 * 16;
    return 2.0f * (3.63e-5f + (float)(3 * kp + 7) * 3.6e-7f + (float)(2 * dsub + 4) * 1.2e-7f);
}

template <int DSUB>
struct mf_geom {
    static constexpr int KP = (DSUB + 15) / 16 * 16;     // reduction length padded to the MFMA's 16
    static constexpr int KS = KP / 16;                   // MFMA k-steps
    // LDS centroid buffers.  Rounds 2-4 double-buffered the narrow widths (the next sub-quantiser's centroids arrived by LDS-DMA
    // during the tile loop).  Round 5 measured the single buffer — barrier, DMA, wait, barrier between two sub-quantisers, the
    // other two blocks of the CU computing meanwhile — FASTER for every width: ms per 2^20 rows, M = 48 / 96 / 64 / 32 / 24:
    // 2.19 -> 1.97, 4.42 -> 4.17, 3.17 -> 2.79, 3.08 -> 2.67, 1.99 -> 1.87 (the DMA's LDS writes no longer compete with the
    // A-fragment reads of the loop, and a block needs 32 KiB instead of 52).
    static constexpr int NBUF = 1;
    static constexpr int BUF_BYTES = RC_K * KP * 2 * 2 + RC_K * 16 + 32;  // hi | lo | cn pieces | wave maxima
};

// Staged centroids of every sub-quantiser, in the LDS layout of assign_mfma_kernel: grid M, block 256 (thread = centroid).
template <int DSUB>
__global__ __launch_bounds__(256) void assign_prep_kernel(const float* __restrict__ C, unsigned char* __restrict__ cpre,
                                                          unsigned* __restrict__ redo_count) {
    using G = mf_geom<DSUB>;
    constexpr int KP = G::KP;
    const int tid = threadIdx.x, m = blockIdx.x, wv = tid >> 6, l = tid & 63;
    if (m == 0 && tid == 0) *redo_count = 0u;               // the doubt list starts empty (a kernel store, not a memset node: a
                                                             // hipGraph holding several of these calls faulted on its second replay)
    unsigned char* buf = cpre + (size_t)m * G::BUF_BYTES;
    float4 cst[DSUB / 4];
    const float4* cp = reinterpret_cast<const float4*>(C + ((size_t)m * RC_K + tid) * DSUB);
#pragma unroll
    for (int j4 = 0; j4 < DSUB / 4; ++j4) cst[j4] = cp[j4];
    // 16-byte chunk g of centroid tid sits at [tile = tid / 32][g][tid % 32]: the 64 lanes of a wave that fetch one A fragment
    // (32 centroids x 2 chunks) read 1 KiB of CONSECUTIVE 16-byte slots — conflict-free for ds_read_b128 (round 5; the row-major
    // layout [centroid][chunk] put lanes 12-15 and 20-23 of a service group on the same banks: 34 % of the LDS cycles)
    uint4* whi = reinterpret_cast<uint4*>(buf) + (size_t)(tid >> 5) * (KP / 8) * 32 + (tid & 31);
    uint4* wlo = reinterpret_cast<uint4*>(buf + RC_K * KP * 2) + (size_t)(tid >> 5) * (KP / 8) * 32 + (tid & 31);
    uint4* cn3 = reinterpret_cast<uint4*>(buf + RC_K * KP * 4);
    float* wmax = reinterpret_cast<float*>(buf + RC_K * KP * 4 + RC_K * 16);
    float nrm = 0.f;
#pragma unroll
    for (int g = 0; g < KP / 8; ++g) {                          // 8 elements -> one 16-byte chunk of each piece
        unsigned h[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (8 * g + 4 * q < DSUB) {
                const float4 v = cst[2 * g + q];
                mf_split2(-2.0f * v.x, -2.0f * v.y, h[2 * q], lo[2 * q]);
                mf_split2(-2.0f * v.z, -2.0f * v.w, h[2 * q + 1], lo[2 * q + 1]);
                nrm = __builtin_fmaf(v.x, v.x, nrm);
                nrm = __builtin_fmaf(v.y, v.y, nrm);
                nrm = __builtin_fmaf(v.z, v.z, nrm);
                nrm = __builtin_fmaf(v.w, v.w, nrm);
            }
        }
        whi[g * 32] = make_uint4(h[0], h[1], h[2], h[3]);
        wlo[g * 32] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
    {   // ||c||^2 = p0 + p1 + p2 exactly (3 x 8 significant bits); it enters the tile as one more MFMA against ones
        unsigned p01, r01, p2, dummy;
        mf_split2(nrm, 0.f, p01, r01);                           // p01.lo16 = p0, r01.lo16 = p1
        const float rest = (nrm - __uint_as_float(p01 << 16)) - __uint_as_float(r01 << 16);
        mf_split2(rest, 0.f, p2, dummy);
        // k-slots 0-2: the pieces of ||c||^2 (against 1.0);  k-slots 3-5: 1.0 against the pieces of the document's offset
        cn3[tid] = make_uint4((p01 & 0xFFFFu) | (r01 << 16), (p2 & 0xFFFFu) | 0x3F800000u, 0x3F803F80u, 0u);
    }
    float mx = nrm;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (l == 0) wmax[wv] = mx;
}

// LDS per block: NBUF x { whi[256][KP] bf16 | wlo[256][KP] bf16 | cn3[256] (3 bf16 pieces of ||c||^2, 16 B) | wave
// maxima[8] } | code tile [256][M].
// NBUF = 2: sub-quantiser m+1's centroids are fetched into registers before the tile loop of m and written to the other
// buffer after it, so one barrier per m and no exposed L2 latency.
// (four waves per SIMD — __launch_bounds__(256, 4) — spills 120-144 bytes per lane at 128 VGPRs: 3.0-3.1 ms against 2.2, round 5)
template <int DSUB>
__global__ __launch_bounds__(256, (DSUB <= 16 ? 3 : (DSUB <= 32 ? 2 : 1))) void assign_mfma_kernel(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ C, int64_t B, int M,
                                                          uint8_t* __restrict__ codes_u8, int64_t* __restrict__ codes_i64,
                                                          unsigned* __restrict__ redo_count, unsigned* __restrict__ redo,
                                                          unsigned redo_cap, int MC, const unsigned char* __restrict__ cpre) {
    // blockIdx.y selects a chunk of MC sub-quantisers (small batches: more blocks than B / 256 alone would give)
    using G = mf_geom<DSUB>;
    constexpr int KP = G::KP, KS = G::KS, NBUF = G::NBUF;
    extern __shared__ __attribute__((aligned(16))) unsigned char mf_smem[];
    unsigned char* tile = mf_smem + NBUF * G::BUF_BYTES;           // [256][M]

    const int tid = threadIdx.x;
    const int wv = tid >> 6, l = tid & 63;
    const int col = l & 31, half = l >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * MF_ROWS_PER_BLOCK;
    int64_t brow[MF_SETS];
    const float* xrow[MF_SETS];
#pragma unroll
    for (int s = 0; s < MF_SETS; ++s) {
        brow[s] = row0 + (wv * MF_SETS + s) * MF_COLS + col;       // shared by lanes l and l^32
        xrow[s] = x + (brow[s] < B ? brow[s] : (B - 1)) * ldx;
    }

    // The staged form of a sub-quantiser's centroids (bf16 pieces of -2 c, pieces of ||c||^2, wave maxima) is the same for
    // every block: assign_prep_kernel writes it once per call, in the LDS layout; here it is a plain copy (fetched into
    // registers early, stored to the free buffer later).  Converting in every block cost ~90 VALU per wave and sub-quantiser.
    constexpr int CH_TOTAL = G::BUF_BYTES / 16, CH_PER = (CH_TOTAL + 255) / 256;
    // asynchronous copy global -> LDS (global_load_lds_dwordx4: 16 bytes per lane, a wave fills 1 KiB of consecutive LDS; no
    // registers in between).  Completion = vmcnt, awaited with stage_wait() before the barrier that publishes the buffer.
    auto stage = [&](int m, unsigned char* buf) {
        const unsigned char* src = cpre + (size_t)m * G::BUF_BYTES;
#pragma unroll
        for (int j = 0; j < CH_PER; ++j) {
            const int w0 = 256 * j + (tid & ~63);                    // first chunk of this wave (wave-uniform)
            if (w0 + l < CH_TOTAL)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)(w0 + l) * 16),
                                                 (__attribute__((address_space(3))) void*)(buf + (size_t)w0 * 16), 16, 0, 0);
        }
    };
    auto stage_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    // this lane's 8 elements of k-step ks: [16 ks + 8 half, +8); zero beyond DSUB
    float4 xq[MF_SETS][KS][2];
    auto fetch_x = [&](int m) {
#pragma unroll
        for (int s = 0; s < MF_SETS; ++s)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int e = 16 * ks + 8 * half + 4 * q;
                    xq[s][ks][q] = (e < DSUB) ? *reinterpret_cast<const float4*>(xrow[s] + m * DSUB + e)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
                }
    };

    const int m0 = blockIdx.y * MC;
    const int mc = (m0 + MC <= M) ? MC : (M - m0);
    stage(m0, mf_smem);
    fetch_x(m0);
    stage_wait();
    __syncthreads();

    for (int mi = 0; mi < mc; ++mi) {
        const int m = m0 + mi;
        const unsigned char* buf = mf_smem + (NBUF == 2 ? (mi & 1) : 0) * G::BUF_BYTES;
        const uint4* whi = reinterpret_cast<const uint4*>(buf);
        const uint4* wlo = reinterpret_cast<const uint4*>(buf + RC_K * KP * 2);
        const uint4* cn3 = reinterpret_cast<const uint4*>(buf + RC_K * KP * 4);
        const float* wmax = reinterpret_cast<const float*>(buf + RC_K * KP * 4 + RC_K * 16);
        const float cnmax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));

        // B operands: bf16 pieces of this lane's elements; squared norm of the whole slice
        mf_bf16x8 bh[MF_SETS][KS], bl[MF_SETS][KS];
        float xn[MF_SETS];
#pragma unroll
        for (int s = 0; s < MF_SETS; ++s) {
            float nrm = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                unsigned h[4], lo[4];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 v = xq[s][ks][q];
                    mf_split2(v.x, v.y, h[2 * q], lo[2 * q]);
                    mf_split2(v.z, v.w, h[2 * q + 1], lo[2 * q + 1]);
                    nrm = __builtin_fmaf(v.x, v.x, nrm);
                    nrm = __builtin_fmaf(v.y, v.y, nrm);
                    nrm = __builtin_fmaf(v.z, v.z, nrm);
                    nrm = __builtin_fmaf(v.w, v.w, nrm);
                }
                bh[s][ks] = __builtin_bit_cast(mf_bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
                bl[s][ks] = __builtin_bit_cast(mf_bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
            }
            xn[s] = nrm + __shfl_xor(nrm, 32);
        }
        constexpr float MARGIN = mf_margin(DSUB);                   // rounding bound of the screen (file header)
        // B operand of the ||c||^2 MFMA: 1.0 in k-slots 0-2, and in k-slots 3-5 the three bf16 pieces of the document's
        // offset ||x||^2 + margin: every screened value becomes (distance^2 + margin) > 0, so the float bits order like
        // signed integers and the epilogue can use v_min3_i32 / v_min_i32 next to v_med3_f32
        mf_bf16x8 bcn[MF_SETS];
#pragma unroll
        for (int s = 0; s < MF_SETS; ++s) {
            const float off = xn[s] + MARGIN * (xn[s] + cnmax);
            unsigned p01, r01, p2, dummy;
            mf_split2(off, 0.f, p01, r01);
            const float rest = (off - __uint_as_float(p01 << 16)) - __uint_as_float(r01 << 16);
            mf_split2(rest, 0.f, p2, dummy);
            bcn[s] = __builtin_bit_cast(mf_bf16x8, make_uint4(0x3F803F80u, 0x00003F80u | (p01 << 16),
                                                              (r01 & 0xFFFFu) | (p2 << 16), 0u));
        }
        const int mn = (mi + 1 < mc) ? m + 1 : m;
        fetch_x(mn);                                                // in flight during the tile loop
        if (NBUF == 2 && mi + 1 < mc)                               // the other buffer: last read before the previous barrier
            stage(m + 1, mf_smem + ((mi + 1) & 1) * G::BUF_BYTES);

        // Tiles T(kt, set), accumulators ping-pong: MFMAs of one tile  ||  epilogue of the previous one.
        // Epilogue: running best / second best over this lane's 16 centroids of the tile; the register index r rides
        // in the 4 low mantissa bits, the tile index of the best is tracked once per tile.
        float m1[MF_SETS], m2[MF_SETS];
        int ktb[MF_SETS];
#pragma unroll
        for (int s = 0; s < MF_SETS; ++s) { m1[s] = INFINITY; m2[s] = INFINITY; ktb[s] = 0; }
        constexpr int NMF = 3 * KS + 1;                             // MFMAs per tile
        constexpr int PER = (16 + NMF - 1) / NMF;                   // epilogue elements per MFMA slot
        struct afrag { mf_bf16x8 h[KS], l[KS], cn; };
        auto load_a = [&](afrag& A, int kt) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int idx = (kt * (KP / 8) + 2 * ks + half) * 32 + col;      // [tile][chunk][centroid in tile]
                A.h[ks] = __builtin_bit_cast(mf_bf16x8, whi[idx]);
                A.l[ks] = __builtin_bit_cast(mf_bf16x8, wlo[idx]);
            }
            const uint4 c = cn3[kt * 32 + col];
            A.cn = __builtin_bit_cast(mf_bf16x8, half ? make_uint4(0u, 0u, 0u, 0u) : c);
        };
        // Candidates are folded in PAIRS: with t = second smallest of {m1, u1, u2} = med3(m1, u1, u2),
        //     m2' = min(m2, t),   m1' = min3(m1, u1, u2)
        // — 3 instructions per pair instead of 2 per candidate (the values are positive, see bcn: integer min = float min,
        // and integer instructions need no canonicalisation of the bit-tagged operands).
        auto tagged = [&](const mf_f32x16& a, int r) {
            return __uint_as_float((__float_as_uint(a[r]) & 0xFFFFFFF0u) | (unsigned)r);
        };
        auto imin = [](float a, float b) {
            const int x = (int)__float_as_uint(a), y = (int)__float_as_uint(b);
            return __uint_as_float((unsigned)(x < y ? x : y));
        };
        auto scan = [&](const mf_f32x16& a, int s, int r0, int cnt) {
            const int r1 = (r0 + cnt < 16) ? r0 + cnt : 16;
#pragma unroll
            for (int r = r0; r < r1; r += 2) {
                const float u1 = tagged(a, r);
                if (r + 1 < r1) {
                    const float u2 = tagged(a, r + 1);
                    const float t = mf_med3(m1[s], u1, u2);
                    m2[s] = imin(m2[s], t);
                    m1[s] = imin(imin(m1[s], u1), u2);
                } else {
                    m2[s] = mf_med3(m1[s], m2[s], u1);
                    m1[s] = imin(m1[s], u1);
                }
            }
        };
        // W = true: issue the MFMAs of tile (A, set sw) into aw;  R = true: run the epilogue of tile (kr, set sr) from ar
        auto step = [&](auto W, auto R, mf_f32x16& aw, const afrag& A, auto sw, const mf_f32x16& ar, auto sr, int kr) {
            constexpr bool w = decltype(W)::value, rd = decltype(R)::value;
            constexpr int SW = decltype(sw)::value, SR = decltype(sr)::value;
            const float before = m1[SR];
#pragma unroll
            for (int j = 0; j < NMF; ++j) {
                if constexpr (w) {
                    if (j == 0) {
                        const mf_f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        aw = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.cn, bcn[SW], zero, 0, 0, 0);
                    } else {
                        const int ks = (j - 1) / 3, t = (j - 1) % 3;
                        aw = __builtin_amdgcn_mfma_f32_32x32x16_bf16(t == 2 ? A.l[ks] : A.h[ks],
                                                                     t == 1 ? bl[SW][ks] : bh[SW][ks], aw, 0, 0, 0);
                    }
                }
                if constexpr (rd) scan(ar, SR, j * PER, PER);
            }
            if constexpr (rd) ktb[SR] = (__float_as_uint(m1[SR]) != __float_as_uint(before)) ? kr : ktb[SR];
            if constexpr (w && rd) {
#pragma unroll
                for (int j = 0; j < NMF; ++j) {                     // issue order: 1 MFMA, then its share of the epilogue
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, PER + 3 * (PER / 2) + 2 * (PER % 2), 0);
                }
            }
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        using S0 = std::integral_constant<int, 0>;
        using S1 = std::integral_constant<int, 1>;
        mf_f32x16 acc0, acc1 = {};
        afrag A0, A1;
        load_a(A0, 0);
        step(T_{}, F_{}, acc0, A0, S0{}, acc1, S1{}, 0);            // T(0,0)
#pragma unroll 1
        for (int kt = 0; kt < RC_K / 32 - 2; kt += 2) {
            load_a(A1, kt + 1);
            step(T_{}, T_{}, acc1, A0, S1{}, acc0, S0{}, kt);       // T(kt,1)    || epilogue T(kt,0)
            step(T_{}, T_{}, acc0, A1, S0{}, acc1, S1{}, kt);       // T(kt+1,0)  || epilogue T(kt,1)
            load_a(A0, kt + 2);
            step(T_{}, T_{}, acc1, A1, S1{}, acc0, S0{}, kt + 1);   // T(kt+1,1)  || epilogue T(kt+1,0)
            step(T_{}, T_{}, acc0, A0, S0{}, acc1, S1{}, kt + 1);   // T(kt+2,0)  || epilogue T(kt+1,1)
        }
        {
            constexpr int kt = RC_K / 32 - 2;
            load_a(A1, kt + 1);
            step(T_{}, T_{}, acc1, A0, S1{}, acc0, S0{}, kt);
            step(T_{}, T_{}, acc0, A1, S0{}, acc1, S1{}, kt);
            step(T_{}, T_{}, acc1, A1, S1{}, acc0, S0{}, kt + 1);
            step(F_{}, T_{}, acc0, A1, S0{}, acc1, S1{}, kt + 1);
        }
#pragma unroll
        for (int s = 0; s < MF_SETS; ++s) {
            const int r = (int)(__float_as_uint(m1[s]) & 15u);
            int k1 = ktb[s] * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float a1 = m1[s], a2 = m2[s];
            {   // merge the two half-waves that share a document
                const float o1 = __shfl_xor(a1, 32), o2 = __shfl_xor(a2, 32);
                const int ok = __shfl_xor(k1, 32);
                const float lo = fminf(a1, o1);
                const float second = fminf(fmaxf(a1, o1), fminf(a2, o2));
                if (o1 < a1 || (o1 == a1 && ok < k1)) k1 = ok;
                a1 = lo;
                a2 = second;
            }
            // also doubtful: NaN / inf inputs (margin non-finite) and magnitudes so small that products of the bf16
            // pieces may be flushed denormals (<= 1.2e-38 per term, far below margin once the scale exceeds 1e-30)
            const float scale = xn[s] + cnmax;
            const bool doubt = !((a2 - a1) > MARGIN * scale) || !(scale > 1e-30f);
            if (half == 0) {
                tile[((wv * MF_SETS + s) * MF_COLS + col) * mc + mi] = (unsigned char)k1;
                if (brow[s] < B && doubt) {
                    const unsigned slot = atomicAdd(redo_count, 1u);
                    if (slot < redo_cap) redo[slot] = (unsigned)(brow[s] * (int64_t)M + m);   // B*M < 2^32 (host)
                }
            }
        }
        if (mi + 1 < mc) {
            if (NBUF == 2) {
                stage_wait();
                __syncthreads();
            } else {
                __syncthreads();                                    // every wave is done with this buffer
                stage(m + 1, mf_smem);
                stage_wait();
                __syncthreads();
            }
        }
    }
    __syncthreads();
    const int64_t rows = (B - row0 < MF_ROWS_PER_BLOCK) ? (B - row0) : MF_ROWS_PER_BLOCK;
    const int64_t nbytes = rows * mc;
    if (mc == M) {                                  // whole rows: the tile is the output image
        if (codes_u8) {
            unsigned char* dst = codes_u8 + row0 * M;   // row0*M is a multiple of 16 (256*M)
            const int64_t n16 = nbytes / 16;
            for (int64_t i = tid; i < n16; i += 256)
                reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(tile)[i];
            for (int64_t i = n16 * 16 + tid; i < nbytes; i += 256) dst[i] = tile[i];
        }
        if (codes_i64) {
            int64_t* dst = codes_i64 + row0 * M;
            for (int64_t i = tid; i < nbytes; i += 256) dst[i] = (int64_t)tile[i];
        }
    } else {                                        // a column chunk of the rows
        for (int64_t i = tid; i < nbytes; i += 256) {
            const int64_t r = i / mc, j = i - r * mc;
            if (codes_u8) codes_u8[(row0 + r) * M + m0 + j] = tile[i];
            if (codes_i64) codes_i64[(row0 + r) * M + m0 + j] = (int64_t)tile[i];
        }
    }
}

// exact recomputation of the doubtful (row, sub-quantiser) pairs: reference arithmetic, first minimum.  One wave per
// pair: lane l judges centroids l, l+64, l+128, l+192 (ascending, so the first minimum within the lane), then a
// butterfly keeps the smaller distance and, on equal distances, the smaller index.
template <int DSUB>
__global__ __launch_bounds__(256) void assign_redo_kernel(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ C, int M,
                                                          const unsigned* __restrict__ redo_count,
                                                          const unsigned* __restrict__ redo, unsigned redo_cap,
                                                          uint8_t* __restrict__ codes_u8, int64_t* __restrict__ codes_i64) {
    unsigned n = *redo_count;
    if (n > redo_cap) n = redo_cap;
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    // A pair is a chain of dependent loads (list entry -> row slice -> distances): the NEXT pair's entry and slice are
    // requested before this pair's 256 distances are computed (round 4; the chain was walked pair by pair: 0.21 ms for the
    // 0.2 % doubtful pairs of 2^20 rows, most of it latency).  Wide slices keep one buffer (registers).
    // The list entry is requested TWO pairs ahead and the slice one pair ahead, so no load is waited for in the iteration that
    // issues it (an entry fetched and used in the same iteration stalls the wave on the in-order vmcnt at once).
    constexpr bool DB = DSUB <= 32;
    float4 xn[DB ? DSUB / 4 : 1];
    unsigned e1 = wave < n ? redo[wave] : 0u;                                  // entry of the next pair to compute
    unsigned e2 = wave + nwaves < n ? redo[wave + nwaves] : 0u;                // and of the one after
    auto fetch_x = [&](unsigned e, bool live) {
        if constexpr (DB) {
            if (!live) return;
            const float4* xp = reinterpret_cast<const float4*>(x + (int64_t)(e / (unsigned)M) * ldx + (int)(e % (unsigned)M) * DSUB);
#pragma unroll
            for (int j = 0; j < DSUB / 4; ++j) xn[j] = xp[j];
        }
    };
    fetch_x(e1, wave < n);
    for (unsigned i = wave; i < n; i += nwaves) {
        const unsigned e = e1;
        const int64_t b = e / (unsigned)M;
        const int m = (int)(e % (unsigned)M);
        float xs[DSUB];
        if constexpr (DB) {
#pragma unroll
            for (int j = 0; j < DSUB / 4; ++j) { xs[4 * j] = xn[j].x; xs[4 * j + 1] = xn[j].y; xs[4 * j + 2] = xn[j].z; xs[4 * j + 3] = xn[j].w; }
        } else {
            const float4* xp = reinterpret_cast<const float4*>(x + b * ldx + m * DSUB);
#pragma unroll
            for (int j = 0; j < DSUB / 4; ++j) {
                const float4 v = xp[j];
                xs[4 * j] = v.x; xs[4 * j + 1] = v.y; xs[4 * j + 2] = v.z; xs[4 * j + 3] = v.w;
            }
        }
        e1 = e2;
        fetch_x(e1, i + nwaves < n);                                           // e2 arrived an iteration ago
        e2 = (i + 2 * nwaves < n) ? redo[i + 2 * nwaves] : 0u;
        const float* cm = C + (size_t)m * RC_K * DSUB;
        float best = INFINITY;
        int bi = 0;
#pragma unroll
        for (int q = 0; q < RC_K / 64; ++q) {
            const int k = q * 64 + lane;
            float cs[DSUB];
            const float4* cp = reinterpret_cast<const float4*>(cm + k * DSUB);
#pragma unroll
            for (int j = 0; j < DSUB / 4; ++j) {
                const float4 v = cp[j];
                cs[4 * j] = v.x; cs[4 * j + 1] = v.y; cs[4 * j + 2] = v.z; cs[4 * j + 3] = v.w;
            }
            const float s = mf_exact<DSUB>(xs, cs);
            if (s < best) { best = s; bi = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            if (codes_u8) codes_u8[b * M + m] = (uint8_t)bi;
            if (codes_i64) codes_i64[b * M + m] = (int64_t)bi;
        }
    }
}

// ------------------------------------------------------------------------------------------ host
// one slot per (row, sub-quantiser) pair: the doubt list cannot overflow, whatever the codebook (4 B M bytes: 201 MB for a
// 2^20-row chunk at M = 48), so no caller has to synchronise and re-run
static unsigned mf_redo_cap(int64_t B, int M) { return (unsigned)(B * M); }

#define MF_PREP_MAX_BYTES (RC_K * 96 * 4 + RC_K * 16 + 256)
extern "C" size_t rc_pq_assign_nearest_fast_ws_bytes(int64_t B, int M) {
    if (B <= 0 || M <= 0) return 0;
    // doubt list + the staged centroids (assign_prep_kernel; at most 25 KiB + 4 KiB per sub-quantiser, dsub <= 96)
    return rc_align_up(256 + (size_t)mf_redo_cap(B, M) * sizeof(unsigned), 256) + (size_t)M * MF_PREP_MAX_BYTES;
}

// Asynchronous and complete: every doubtful pair (at most B*M of them) is re-judged exactly by assign_redo_kernel.
// rc_pq_assign_nearest_fast_overflow remains for statistics (number of doubtful pairs) and always reports 0.
extern "C" int rc_pq_assign_nearest_fast(rc_handle_t h, const float* x, int64_t ldx, const float* C, int64_t B, int D,
                                         int M, int K, uint8_t* codes_u8, int64_t* codes_i64, void* ws, size_t ws_bytes,
                                         rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !x || !C || B < 0 || M <= 0 || D <= 0 || ldx < D || (!codes_u8 && !codes_i64)) return RC_EINVAL;
    if (K != RC_K || D % M != 0) return RC_ESHAPE;
    if (!rc_dsub_supported(D / M))                         // widths without a matrix-core screen: the exact kernel at run-time width
        return rc_pq_assign_nearest(h, x, ldx, C, B, D, M, K, codes_u8, codes_i64, stream);
    if (B * (int64_t)M > 0xFFFFFFFFll) return RC_ESHAPE;
    if (((uintptr_t)x & 15) || (ldx % 4) != 0) return RC_EINVAL;
    if (B == 0) return RC_OK;
    if (!ws || ws_bytes < rc_pq_assign_nearest_fast_ws_bytes(B, M)) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned* redo_count = (unsigned*)ws;
    unsigned* redo = (unsigned*)((char*)ws + 256);
    const unsigned cap = mf_redo_cap(B, M);
    unsigned char* cpre = (unsigned char*)ws + rc_align_up(256 + (size_t)cap * sizeof(unsigned), 256);
    const int dsub = D / M;
    const int64_t nblk = (B + MF_ROWS_PER_BLOCK - 1) / MF_ROWS_PER_BLOCK;
    int MC = M;                                     // sub-quantisers per block: split M while the grid is under ~3 blocks per CU
    while (MC > 1 && nblk * ((M + MC - 1) / MC) < 3 * (int64_t)h->num_cus) MC = (MC + 1) / 2;
    const unsigned nchunk = (unsigned)((M + MC - 1) / MC);
    const int kp = (dsub + 15) / 16 * 16;
    const size_t lds = (size_t)(dsub <= 32 ? 2 : 1) * ((size_t)RC_K * kp * 4 + RC_K * 16 + 32) + (size_t)MF_ROWS_PER_BLOCK * M;
    rc_prof_mark(h, RC_PROF_ASSIGN_NEAREST, s);
    switch (dsub) {
#define MF_CASE(DS)                                                                                                      \
        case DS: {                                                                                                       \
            auto kern = assign_mfma_kernel<DS>;                                                                          \
            RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            hipLaunchKernelGGL(assign_prep_kernel<DS>, dim3((unsigned)M), dim3(256), 0, s, C, cpre, redo_count);         \
            hipLaunchKernelGGL(kern, dim3((unsigned)nblk, nchunk), dim3(256), lds, s, x, ldx, C, B, M, codes_u8, codes_i64, \
                               redo_count, redo, cap, MC, (const unsigned char*)cpre);                                       \
            hipLaunchKernelGGL(assign_redo_kernel<DS>, dim3((unsigned)(h->num_cus * (DS <= 32 ? 8 : 4))), dim3(256), 0, s, x, ldx, C, M,  \
                               redo_count, redo, cap, codes_u8, codes_i64);                                              \
        } break;
        MF_CASE(8) MF_CASE(12) MF_CASE(16) MF_CASE(24) MF_CASE(32) MF_CASE(48) MF_CASE(64) MF_CASE(96)
#undef MF_CASE
        default: return RC_ESHAPE;
    }
    rc_prof_mark(h, RC_PROF_ASSIGN_NEAREST, s);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// The compiled margin of the screen for a sub-vector width (negative: no screen for that width).  Needs no GPU.
extern "C" float rc_pq_assign_nearest_fast_margin(int dsub) {
    switch (dsub) {
#define MF_CASE(DS) case DS: return mf_margin(DS);
        MF_CASE(8) MF_CASE(12) MF_CASE(16) MF_CASE(24) MF_CASE(32) MF_CASE(48) MF_CASE(64) MF_CASE(96)
#undef MF_CASE
        default: return -1.0f;
    }
}

// After the stream has drained: did the doubt list overflow?  (1 = yes: rerun with rc_pq_assign_nearest.)
extern "C" int rc_pq_assign_nearest_fast_overflow(rc_handle_t h, const void* ws, int64_t B, int M, int* doubtful_host) {
    rc_device_guard device_guard_(h);
    if (!h || !ws) return RC_EINVAL;
    unsigned n = 0;
    RC_HIP_CHECK(h, hipMemcpy(&n, ws, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (doubtful_host) *doubtful_host = (int)n;
    return n > mf_redo_cap(B, M) ? 1 : 0;
}
