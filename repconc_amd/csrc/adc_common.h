// Shared pieces of the flat ADC search (adc_search.hip with its screens adc_screen16.h and adc_screen_r1.h) and the list-centric
// IVF search (ivf_lists.hip, ivfs_*.h) that are about ADC tables and codes: limits, the supported widths, the conflict-free slot
// rule, the 16-query slot rule, the 8-bit quantiser with the per-query table summary and its record, the IVF task list, the load
// of a row's code bytes, the exact rescoring kernel and the launcher of the image kernels.  The selection stage (score keys,
// k-th largest, the candidate-list limits and the wave append to a list, top-k host interface) is topk.h.  Device functions,
// templates and static host helpers only (no -fgpu-rdc: every translation unit compiles its own copy).
#pragma once
#include "topk.h"
#include <limits.h>

#define ADC_THREADS 1024
#define ADC_TILE_DOCS 32768
#define ADC_SCREEN_MIN_N (1 << 18)
#define ADC_ID_CAP 32768

// widths M with a permuted code image: the 16-query flat screen and the list-centric IVF search are compiled for exactly these
// (every list below is generated from this one)
#define ADC_CF_WIDTHS(X) X(16) X(32) X(48) X(64) X(96)
__host__ __device__ constexpr bool adc_cf_supported(int M) {
#define ADC_CF_IS(MM) || M == MM
    return false ADC_CF_WIDTHS(ADC_CF_IS);
#undef ADC_CF_IS
}
__host__ __device__ constexpr int adc_cf_max_width() {
    int w = 0;
#define ADC_CF_MAX(MM) w = MM > w ? MM : w;
    ADC_CF_WIDTHS(ADC_CF_MAX)
#undef ADC_CF_MAX
    return w;
}
// widths the screened flat search is compiled for, as (M, queries per block of the fp32 scan): rc_adc_search* (ADC_CASE), the
// templated scores of rc_adc_search_exact (ADC_EXACT_CASE) and adc_search_supported are generated from this list; every other
// divisor of D is answered by the exact scan with a run-time width (rc_adc_search_exact, adc_scan_rt_kernel)
#define ADC_SEARCH_WIDTHS(X) X(8, 4) X(12, 4) X(16, 4) X(24, 4) X(32, 4) X(48, 2) X(64, 2) X(96, 1)
static inline bool adc_search_supported(int M) {
#define ADC_SEARCH_IS(MM, QQ) || M == MM
    return false ADC_SEARCH_WIDTHS(ADC_SEARCH_IS);
#undef ADC_SEARCH_IS
}

// ---- conflict-free slot rule (round 2; today the table phases of the IVF screen, ivf_lists.hip) ------------------
// The sum over sub-quantisers is commutative, so the lanes of a wave need not visit them in the same order: byte tables are
// laid out [code][slot][8 queries] with one 8-byte SLOT per sub-quantiser (a slot's LDS bank pair is slot mod 32 whatever the
// code) and in every step the 32 lanes the LDS services together read 32 DIFFERENT slots mod 32: lane (r, g) of a 16-row
// chunk walks block-relative sub-quantiser (r + (S/4) tau(g) + j) mod S in step j, S = 32 or 16 the size of the block of
// sub-quantisers, tau(g) = 2 (g & 1) + (g >> 1); a 16-block is stored twice (slots 16 apart), lanes 16-31 of the group use
// the second copy.  Conflict-free BY CONSTRUCTION, for any codes; a lane receives its codes in its own visiting order from a
// permuted image of the code matrix (the permutation of row n depends on n mod 16 only).
template <int PM>
struct adc_cf {
    static_assert(PM % 16 == 0 && PM >= 16 && PM <= 64, "table phase of 16/32/48/64 sub-quantisers");
    static constexpr int N32 = PM / 32, HAS16 = (PM % 32) / 16;
    static constexpr int SLOTS = 32 * (N32 + HAS16);       // 8-byte slots per code: LDS row of SLOTS * 8 bytes
    static constexpr int STEPS = PM / 4;                   // gathers per lane per 16-row chunk
    static constexpr int TABLE_BYTES = RC_K * SLOTS * 8;
};
// step s (0 .. PM/4-1) of a lane -> size of the block of sub-quantisers it falls in, the block's first sub-quantiser
// (= its first slot) and the step index inside the block.  32-blocks first, then the 16-block.
__host__ __device__ constexpr int adc_cf_bsize(int PM, int s) { return s < 8 * (PM / 32) ? 32 : 16; }
__host__ __device__ constexpr int adc_cf_bbase(int PM, int s) { return s < 8 * (PM / 32) ? 32 * (s / 8) : 32 * (PM / 32); }
__host__ __device__ constexpr int adc_cf_bstep(int PM, int s) { return s < 8 * (PM / 32) ? s % 8 : s - 8 * (PM / 32); }
// block-relative sub-quantiser that lane (r, g) reads in step j of a block of size S
__host__ __device__ inline int adc_cf_mloc(int S, int j, int r, int g) {
    return (r + (S >> 2) * (2 * (g & 1) + (g >> 1)) + j) & (S - 1);
}
// slot (within the phase's table) and sub-quantiser (within the phase) of step s for lane (r, g)
__host__ __device__ inline void adc_cf_step(int PM, int s, int r, int g, int& slot, int& m) {
    const int S = adc_cf_bsize(PM, s), base = adc_cf_bbase(PM, s), j = adc_cf_bstep(PM, s);
    const int ml = adc_cf_mloc(S, j, r, g);
    const int lam = r + 16 * (g & 1);                      // lane index inside the 32 lanes the LDS services together
    m = base + ml;
    slot = base + ml + S * (lam / S);                      // S = 16: second copy for lanes 16-31
}

// ---- the 8-bit screen's step, bytes and integer threshold (flat search: adc_qlut_kernel, adc_qstats_kernel; IVF search:
// ivfs_qprep_kernel + ivf_rank_select_kernel).  This is the one place where the bound is stated and computed.
//
// A query's tables LUT[m][c] (fp32) have lo_m = min_c, hi_m = max_c.  One step per query, delta = max_m (hi_m - lo_m) / 255
// (adc_screen_delta), bytes l_m(c) = adc_quant8(LUT[m][c], lo_m, delta), and a row n with codes c_m is kept by the screen when
// S_int(n) = sum_m l_m(c_m) >= T.  The search promises that the screen drops NO row whose exact score is >= tau, where the
// exact score is the contract's fp32 sum  s(n) = fl(...fl(fl(L_0 + L_1) + L_2)... + L_{M-1}),  L_m = LUT[m][c_m], m ascending
// from 0 (adc_rescore_row, the oracle).  Write R = sum_m L_m (real numbers), A = sum_m lo_m, B = sum_m max(|lo_m|, |hi_m|).
//  (1) bytes.  x = fl(fl(L_m - lo_m) / delta) and l = floor(fl(x + 0.5)) are three roundings of values below 256, each off by
//      at most 2^-24 of its result: l >= (L_m - lo_m) / delta - 1/2 - e with e < 1e-4.  The clamps do not enter: 0 only raises
//      l, and adc_screen_delta guarantees (hi_m - lo_m) / delta <= 255.25, which rounds to 255.  Summed over the M entries of a
//      row:  S_int >= (R - A) / delta - M / 2 - M e.
//  (2) the exact score is not R.  Its M - 1 rounded additions (0 + L_0 is exact; fp32 addition cannot underflow, a sub-normal
//      sum is exact) give  |s - R| <= g sum_m |L_m| <= g B  with g = (M - 1) u / (1 - (M - 1) u), u = 2^-24 (Higham, Accuracy
//      and Stability of Numerical Algorithms, 4.2).  The integer sum follows R, the test it stands in for is on s: when the
//      tables carry an offset that is large against their range, g B is many steps.  E = M u B >= g B + (the rounding of A and
//      B themselves, summed in double: at most M 2^-53 B each) for every M <= 128.
//  (1) + (2):  s >= tau  =>  R >= tau - E  =>  S_int >= (tau - A - E) / delta - M / 2 - M e.
//  T = ceil((tau - A - E) / delta - M / 2) - 2 is at least 1 below that; the 1 covers M e <= 0.013 and the roundings of this
//  double expression (|value| <= 2e9 or the result saturates: below 1e-6).  (S_int is an integer, so - 1 would do; - 2 is the
//  value the screens were tuned and measured with.)  So the bound is rigorous about exactly this: for
//  finite tables no row with fp32 score >= tau fails the integer test.  It says nothing about how FEW rows pass: E / delta is
//  0.02 .. 0.1 steps on zero-mean tables (ranges of a few sigma), but with an offset of 1e5 ranges the threshold falls by
//  thousands of steps, the survivor list overflows (status bit 1) and the search's repeat -> exact route answers instead.
//  delta = inf (a range that overflows fp32): every byte is 0, T < 0, every row passes — the same route.
__device__ __forceinline__ float adc_screen_delta(float maxrange) {
    float delta = maxrange / 255.0f;
    if (!(delta > 0.f)) delta = 1.0f;                       // constant tables: every byte 0
    // a sub-normal quotient has lost bits: a step rounded DOWN by 2^-4 would let the clamp at 255 cut more than half a step off
    // the largest entries.  One ulp up restores 255 delta >= maxrange (never taken by a normal quotient: it is within 2^-24).
    if ((double)maxrange > 255.25 * (double)delta) delta = __uint_as_float(__float_as_uint(delta) + 1u);
    return delta;
}
__device__ __forceinline__ unsigned adc_quant8(float v, float lo, float delta) {
    int l = (int)floorf((v - lo) / delta + 0.5f);           // nearest: (1) above costs M / 2 steps, not M
    l = l < 0 ? 0 : (l > 255 ? 255 : l);
    return (unsigned)l;
}
// t = tau, A = sum of lo_m and B = sum of max(|lo_m|, |hi_m|), both accumulated in double, m ascending
__device__ __forceinline__ int adc_screen_tint(float t, double A, double B, float delta, int M) {
    if (t == -INFINITY) return INT_MIN;                     // no threshold: every row is a candidate
    const double E = (double)M * 5.9604644775390625e-8 * B; // M 2^-24 B
    const double v = ceil(((double)t - A - E) / (double)delta - 0.5 * (double)M) - 2.0;
    return v < -2.0e9 ? INT_MIN : (v > 2.0e9 ? INT_MAX : (int)v);
}

// The summary of a query's tables: from lo_m, hi_m - lo_m and max(|lo_m|, |hi_m|) of its M sub-quantisers the step delta and the
// sums A and B above (in double, m ascending).  Called by ONE thread of the kernels that reduce the tables (adc_qlut_kernel,
// adc_qstats_kernel, ivfs_qprep_kernel).
struct adc_table_sums {
    float delta;
    double A, B;
};
__device__ __forceinline__ adc_table_sums adc_table_summary(const float* lo, const float* range, const float* absmax, int M) {
    float maxrange = 0.f;
    adc_table_sums s = {0.f, 0.0, 0.0};
    for (int m = 0; m < M; ++m) {
        maxrange = fmaxf(maxrange, range[m]);
        s.A += (double)lo[m];
        s.B += (double)absmax[m];
    }
    s.delta = adc_screen_delta(maxrange);
    return s;
}
__device__ __forceinline__ int adc_screen_tint(float t, const adc_table_sums& s, int M) {
    return adc_screen_tint(t, s.A, s.B, s.delta, M);
}
// The qstat record of a query (adc_qstats_kernel, ivfs_qprep_kernel): ADC_QSTAT_STRIDE floats, lo_m at [m], m < M, and the
// summary in the record's last six: B (a double) at [122], A (a double) at [124], delta at [127]
#define ADC_QSTAT_STRIDE 128
#define ADC_QSTAT_B (ADC_QSTAT_STRIDE - 6)
#define ADC_QSTAT_A (ADC_QSTAT_STRIDE - 4)
#define ADC_QSTAT_DELTA (ADC_QSTAT_STRIDE - 1)
static_assert(adc_cf_max_width() <= ADC_QSTAT_B, "the lo_m of the widest compiled M leave the A / B / delta fields free");
static_assert(ADC_QSTAT_B % 2 == 0 && ADC_QSTAT_A % 2 == 0 && ADC_QSTAT_B + 2 <= ADC_QSTAT_A && ADC_QSTAT_A + 2 <= ADC_QSTAT_DELTA,
              "aligned doubles that overlap nothing");
__device__ __forceinline__ float* adc_qstat_of(float* qstat, int qi) { return qstat + (size_t)qi * ADC_QSTAT_STRIDE; }
__device__ __forceinline__ const float* adc_qstat_of(const float* qstat, int qi) { return qstat + (size_t)qi * ADC_QSTAT_STRIDE; }
__device__ __forceinline__ float adc_qstat_delta(const float* st) { return st[ADC_QSTAT_DELTA]; }
__device__ __forceinline__ void adc_qstat_put_summary(float* st, const adc_table_sums& s) {
    st[ADC_QSTAT_DELTA] = s.delta;
    *reinterpret_cast<double*>(st + ADC_QSTAT_A) = s.A;
    *reinterpret_cast<double*>(st + ADC_QSTAT_B) = s.B;
}
__device__ __forceinline__ adc_table_sums adc_qstat_summary(const float* st) {
    return adc_table_sums{st[ADC_QSTAT_DELTA], *reinterpret_cast<const double*>(st + ADC_QSTAT_A),
                          *reinterpret_cast<const double*>(st + ADC_QSTAT_B)};
}

typedef int adc_i32x4v __attribute__((ext_vector_type(4)));
typedef unsigned adc_u32x2v __attribute__((ext_vector_type(2)));

// 16-query gathers (ds_read_b128; adc_screen16.h, ivfs_screen16.h): position of a lane inside its service group of 16
// lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32), and the sub-quantiser (within its phase of 16) = LDS slot
// that lane `lane` of a wave reads in step j — distinct inside every service group, the four lanes of a row cover all 16
__host__ __device__ constexpr int adc_q16_pos(int h32) {
    return (h32 < 4) ? h32 : (h32 < 12) ? h32 - 4 : (h32 < 16) ? h32 - 8 : (h32 < 20) ? h32 - 8 : (h32 < 28) ? h32 - 12 : h32 - 16;
}
__host__ __device__ constexpr int adc_q16_slot(int lane, int j) { return (adc_q16_pos(lane & 31) + j + 4 * (lane >> 5)) & 15; }

// Tasks of the list-centric IVF search: a task = (coarse cell, up to 8 | 16 of the queries that probe it: the screen's width)
struct adc_ivf_tasks {
    const int* task_list;        // [tasks] cell of the task
    const int* task_qstart;      // [tasks] first entry of the task's queries in sorted_q
    const int* task_qcnt;        // [tasks] 1 .. 8 queries (1 .. 16 for the 16-query screen)
    const int* sorted_q;         // query ids ordered by probed cell
    const int64_t* list_off;     // [nlist + 1] row ranges of the cells
    const uint8_t* qbyte;        // [nq][NP][256][PM] per-query byte tables, one byte per sub-quantiser
    const int* ntasks;           // device-side task count when the list is padded (rc_ivf_search_probes), else NULL
};

// A row's NB code bytes (cp aligned to the load width) into dwords, by the widest aligned load: 16-byte loads when NB % 16 == 0,
// 8-byte when NB % 8 == 0, else 4-byte.  The scan, the round-1 screens (the matrix-core one on half a row) and the rescorer.
template <int NB>
__device__ __forceinline__ void adc_load_code_bytes(const uint8_t* cp, unsigned (&w)[NB / 4]) {
    constexpr int W = (NB % 16 == 0) ? 16 : (NB % 8 == 0) ? 8 : 4;  // load width in bytes
#pragma unroll
    for (int j = 0; j < NB / W; ++j) {
        if constexpr (W == 16) {
            const uint4 v = reinterpret_cast<const uint4*>(cp)[j];
            w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
        } else if constexpr (W == 8) {
            const uint2 v = reinterpret_cast<const uint2*>(cp)[j];
            w[2 * j] = v.x; w[2 * j + 1] = v.y;
        } else {
            w[j] = reinterpret_cast<const unsigned*>(cp)[j];
        }
    }
}

// One block per query: exact fp32 score (m ascending, from 0) of every screened row; rows with score >= tau go
// to the key list exactly as adc_scan_kernel<FILTER> would have put them.
// A block's table is 4 M x 256 bytes of LDS and every survivor costs one dependent M-byte read from HBM, so the kernel lives
// on rows in flight: the block is as large as the LDS lets the CU hold 16+ waves (adc_rescore_threads), the table and the
// codes move in 16-byte pieces, and every thread has two rows in flight (round 4; 512 threads and 4-byte loads before:
// M = 96 ran 8 waves per CU).
template <int M>
__device__ __forceinline__ float adc_rescore_row(const uint8_t* __restrict__ cp, const float* __restrict__ tab) {
    unsigned w[M / 4];
    adc_load_code_bytes<M>(cp, w);
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) s = s + tab[m * RC_K + ((w[m >> 2] >> (8 * (m & 3))) & 0xFFu)];
    return s;
}

static int adc_rescore_threads(int M) { return M * RC_K * 4 > 80 * 1024 ? 1024 : 512; }

template <int M>
__global__ __launch_bounds__(1024) void adc_rescore_kernel(const uint8_t* __restrict__ codes,
                                                          const float* __restrict__ lut,
                                                          const float* __restrict__ thr,
                                                          const unsigned* __restrict__ id_count,
                                                          const unsigned* __restrict__ ids,
                                                          unsigned* __restrict__ cand_count,
                                                          unsigned long long* __restrict__ cand,
                                                          int* __restrict__ status,
                                                          const int64_t* __restrict__ rowmap,
                                                          int* __restrict__ qstatus = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tab = reinterpret_cast<float*>(smem);  // [M][256]
    const int qi = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const unsigned raw = id_count[qi];
    const unsigned cnt = raw > ADC_ID_CAP ? ADC_ID_CAP : raw;
    const unsigned* qids = ids + (size_t)qi * ADC_ID_CAP;
    // the first rows' ids and codes are requested before the table: their latency hides behind the staging
    unsigned n0 = 0, n1 = 0;
    if (tid < (int)cnt) n0 = qids[tid];
    if (tid + nthr < (int)cnt) n1 = qids[tid + nthr];
    {
        const float4* l4 = reinterpret_cast<const float4*>(lut + (size_t)qi * M * RC_K);
        float4* t4 = reinterpret_cast<float4*>(tab);
        for (int i = tid; i < M * RC_K / 4; i += nthr) t4[i] = l4[i];
    }
    if (tid == 0 && raw > ADC_ID_CAP) {
        atomicOr(status, 2);
        if (qstatus) atomicOr(qstatus + qi, 2);
    }
    const float tau = thr[qi];
    // this block is the only writer of the query's key list: slots come from an LDS counter, the global count is written
    // once at the end (round 3: one returning global atomic per wave and iteration, all on ONE address — 27 of 150 us)
    __shared__ unsigned s_slots;
    if (tid == 0) s_slots = 0u;
    const unsigned base0 = cand_count[qi];
    __syncthreads();
    for (unsigned i0 = 0; i0 < cnt; i0 += 2 * nthr) {
        const unsigned ia = i0 + tid, ib = ia + nthr;
        const bool la = ia < cnt, lb = ib < cnt;
        const unsigned na = n0, nb = n1;
        // next pair of ids (dependent chain: id -> codes), requested before this pair is scored
        n0 = (ia + 2 * nthr < cnt) ? qids[ia + 2 * nthr] : 0u;
        n1 = (ib + 2 * nthr < cnt) ? qids[ib + 2 * nthr] : 0u;
        // a wave whose 64 slots are all past the end of the list does nothing (the last iteration of a 2100-row list has
        // 96 live slots of 2048: without the test the kernel did 1.9 x the lookups the list needs)
        float sa = 0.f, sb = 0.f;
        if (__ballot(la)) sa = adc_rescore_row<M>(codes + (size_t)(la ? na : 0u) * M, tab);
        if (__ballot(lb)) sb = adc_rescore_row<M>(codes + (size_t)(lb ? nb : 0u) * M, tab);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool live = h ? lb : la;
            const float sc = h ? sb : sa;
            const unsigned n = h ? nb : na;
            const bool pass = live && (sc >= tau);
            const unsigned long long mask = __ballot(pass);
            if (mask) {
                const unsigned slot = base0 + adc_wave_append(mask, &s_slots);
                if (pass && slot < ADC_CAND_CAP) {
                    // IVF: rows are stored cell-major; the key carries the row's corpus position so ties order by corpus id
                    const unsigned id = rowmap ? (unsigned)rowmap[n] : n;
                    cand[(size_t)qi * ADC_CAND_CAP + slot] = adc_exact_key(sc, id);
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0 && s_slots) cand_count[qi] = base0 + s_slots;
}

// (Re)build rows [n0, n0 + n) of a permuted code image from the canonical codes [N, M]: the one launcher of the three image
// kernels (rc_adc_scan_image: the flat search's; rc_adc_scan_image_rows / _rows16: the IVF screens')
typedef void (*adc_image_kernel_t)(const uint8_t*, int64_t, int64_t, int, uint8_t*);
static int adc_launch_image(rc_handle_t h, adc_image_kernel_t kern, const uint8_t* codes, int64_t n0, int64_t n, int M,
                            uint8_t* image, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !codes || !image || n0 < 0 || n < 0) return RC_EINVAL;
    if (!adc_cf_supported(M)) return RC_ESHAPE;
    if (n == 0) return RC_OK;
    int64_t blocks = (n * M + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, codes, n0, n, M, image);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
