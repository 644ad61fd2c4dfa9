// PQ asymmetric-distance top-k search over raw uint8 codes: inner product, and the L2 metric as the same pipeline on tables
// S = 0.0f - T with one trailing negate (rc_adc_lut_l2, rc_adc_search_l2_q / _exact; the definition is at adc_lut_step).
//
// Reference: `index.search(query_embeds, topk)` on a faiss.IndexPQ(D, M, 8, METRIC_INNER_PRODUCT)
// or its 1-list IVFPQ clone — models/repconc/evaluate_repconc.py:78-135,180-185 and
// models/jpq/finetune_jpq.py:176.  Faiss is not vendored in the reference; the arithmetic restated
// here is Faiss 1.7.x's published IndexPQ behaviour: per query an
// inner-product table LUT[m][k] = <q_m, C[m,k]>, score(n) = sum_m LUT[m][code[n,m]] accumulated
// m-ascending in fp32, the k largest returned in decreasing order (ties: lower id first).
//
// Pipeline for one batch of queries (all on one stream, no host round trip):
//   1. adc_lut_kernel        LUT[nq][M][256] (fp32; 48 KiB per query at M=48)
//   2. adc_scan_kernel<SAMPLE> scores of S <= 32768 evenly spread rows -> sample[nq][S]
//   3. adc_threshold_kernel  (topk.hip) per query: the r-th largest sample score (LDS radix select) = tau_q;
//                            r is chosen so that ~ (r/S)*N >> k rows pass, i.e. the true top-k are
//                            all >= tau_q with overwhelming probability (host checks the count)
//   4. full scan, rows with score >= tau_q are appended to a per-query candidate list of 64-bit keys.  Two
//      implementations with IDENTICAL output:
//        a. adc_scan_kernel<FILTER>: exact fp32 scores for every row (small indexes);
//        b. integer screening (N >= 2^18): each query's tables are quantised to 8 bits with a common step Delta_q
//           (l = round((LUT - min_m)/Delta_q)); the screen sums the bytes and keeps every row with S_int >= T_q, where
//           T_q = ceil((tau_q - sum_m min_m - E_q)/Delta_q - M/2) - 2 is a lower bound that is RIGOROUS about this: no row
//           whose fp32 score (m ascending) is >= tau_q fails it.  M/2: every byte is off by at most half a step; E_q = M 2^-24
//           sum_m max|LUT_m|: the fp32 score is not the real-number sum the bytes follow; - 2: the float roundings of the
//           quantiser and of T_q itself.  Derivation and code: adc_screen_tint, adc_common.h;
//           adc_rescore_kernel (adc_common.h) then computes the exact fp32 score of the survivors (~1.4x the final
//           candidates) and applies the exact test.  The candidate set, hence the result, is the same as (a).
//           Screens, one unit each: adc_screen16.h holds adc_screen_q16_kernel for the M with a permuted image (16, 32, 48,
//           64, 96: 16 queries per conflict-free ds_read_b128 gather, phases of 16 sub-quantisers, i8 MFMA accumulation) with
//           its image and table kernels; adc_screen_r1.h holds, for the other M (8, 24 / 12) and as the tests' A/B partner
//           (RC_ADC_OLD_SCREEN=1), the round-1 screens on the canonical codes: adc_screen_mfma_kernel
//           (v_mfma_i32_32x32x32_i8 against a selection matrix) and adc_screen_kernel (VALU, M % 8 != 0) with adc_qlut_kernel.
//           This file keeps the LUT, scan and table-statistics kernels and the host code.  The screen generations in between
//           (round-2 8-query conflict-free screen, two-phase / two-pass M = 96 forms) were removed in round 4; the
//           list-centric IVF search lives in ivf_lists.hip.
//   5. adc_select_kernel     (topk.hip) per query: radix-select cut to the k best scores (+ties), bitonic sort in LDS, emit top-k
// Steps 3 and 5 — and the 8-pass radix select that ends the exact route below (rc_adc_search_exact) — are the selection
// stage shared with the IVF and dense searches: topk.h / topk.hip, which also state the key format and the status bits.
//
// The scan is the hot kernel.  A block keeps the LUTs of QT queries in LDS, interleaved
// [m][k][QT] so ONE ds_read_b64 / b128 gather serves QT queries, and streams a tile of codes
// (consecutive lanes = consecutive rows, 16-byte loads).  Blocks that share a code tile are
// adjacent in the grid, so a tile is fetched from HBM about once per XCD and re-read from L2.
#include "adc_common.h"
#include <stdio.h>
#include <string.h>

// ------------------------------------------------------------------------------------------ 1. LUT
// One table entry.  Inner product: j-ascending multiply then add, each rounded (no FMA).  L2 (rc_adc_lut_l2): the sub-distance
// T = sum_j (q_j - c_j)^2, j ascending from +0.0f, one rounded subtraction, product and sum each (Faiss's scalar fvec_L2sqr),
// stored as S = 0.0f - T: the pipeline keeps "largest score, lowest row", and 0.0f - T is -T for T > 0 but +0.0f for T = 0, so
// no entry is -0.0f and every scoring path (sum started from 0.f or from the first entry) gives a zero distance the same bits.
template <bool L2>
__device__ __forceinline__ float adc_lut_step(float s, float qj, float cj) {
    if constexpr (L2) {
        const float t = qj - cj;
        return s + t * t;
    } else {
        return s + qj * cj;
    }
}
template <bool L2>
__device__ __forceinline__ float adc_lut_entry(float s) { return L2 ? 0.0f - s : s; }

// grid (nq, M), block 256 (= k): any dsub.
template <bool L2>
__global__ __launch_bounds__(RC_K) void adc_lut_kernel(const float* __restrict__ C, const float* __restrict__ q,
                                                       int D, int M, float* __restrict__ lut) {
    const int qi = blockIdx.x, m = blockIdx.y, k = threadIdx.x;
    const int dsub = D / M;
    const float* qs = q + (size_t)qi * D + m * dsub;  // wave-uniform
    const float* c = C + ((size_t)m * RC_K + k) * dsub;
    float s = 0.f;
    for (int j = 0; j < dsub; ++j) s = adc_lut_step<L2>(s, qs[j], c[j]);
    lut[((size_t)qi * M + m) * RC_K + k] = adc_lut_entry<L2>(s);
}

// Same arithmetic, supported dsub: thread k keeps its centroid row in registers and walks a chunk of queries (the
// query slice is block-uniform -> scalar loads), so the 16 KiB centroid table is read once per 32 queries instead of
// once per query (0.40 ms -> per 1200 queries at M = 48 for the kernel above).
#define ADC_LUT_QCHUNK 32
template <int DSUB, bool L2>
__global__ __launch_bounds__(RC_K) void adc_lut_rows_kernel(const float* __restrict__ C, const float* __restrict__ q,
                                                            int nq, int D, int M, float* __restrict__ lut) {
    const int m = blockIdx.y, k = threadIdx.x;
    float c[DSUB];
    const float4* cp = reinterpret_cast<const float4*>(C + ((size_t)m * RC_K + k) * DSUB);
#pragma unroll
    for (int j = 0; j < DSUB / 4; ++j) {
        const float4 v = cp[j];
        c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
    }
    const int q0 = blockIdx.x * ADC_LUT_QCHUNK;
    const int q1 = (q0 + ADC_LUT_QCHUNK < nq) ? q0 + ADC_LUT_QCHUNK : nq;
    for (int qi = q0; qi < q1; ++qi) {
        const float* qs = q + (size_t)qi * D + m * DSUB;   // block-uniform
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < DSUB; ++j) s = adc_lut_step<L2>(s, qs[j], c[j]);
        lut[((size_t)qi * M + m) * RC_K + k] = adc_lut_entry<L2>(s);
    }
}

// ------------------------------------------------------------------------------------------ 2/4. scan
template <int QT> struct adc_vec;
template <> struct adc_vec<1> { using type = float; };
template <> struct adc_vec<2> { using type = float2; };
template <> struct adc_vec<4> { using type = float4; };

template <int QT>
__device__ __forceinline__ void adc_acc(float (&s)[QT], const typename adc_vec<QT>::type& v) {
    if constexpr (QT == 1) { s[0] = s[0] + v; }
    if constexpr (QT == 2) { s[0] = s[0] + v.x; s[1] = s[1] + v.y; }
    if constexpr (QT == 4) { s[0] = s[0] + v.x; s[1] = s[1] + v.y; s[2] = s[2] + v.z; s[3] = s[3] + v.w; }
}

enum { ADC_SAMPLE = 0, ADC_FILTER = 1 };

// grid (query groups, doc tiles).  SAMPLE: row n_i = floor(i*N/S), i in the tile, dense output.
// FILTER: rows of the tile, candidates with score >= thr[q] appended as keys
// (ordered(score) << 32 | ~row), so a descending key sort is (score desc, row asc).
template <int M, int QT, int MODE>
__global__ __launch_bounds__(ADC_THREADS) void adc_scan_kernel(const uint8_t* __restrict__ codes, int64_t N,
                                                               const float* __restrict__ lut, int nq, int64_t S,
                                                               float* __restrict__ sample,
                                                               const float* __restrict__ thr,
                                                               unsigned* __restrict__ cand_count,
                                                               unsigned long long* __restrict__ cand) {
    using V = typename adc_vec<QT>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    V* tab = reinterpret_cast<V*>(smem);  // [M*256]
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * QT;
    // stage the QT tables interleaved; queries past nq replicate the last valid one
    for (int i = tid; i < M * RC_K; i += ADC_THREADS) {
        float v[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int qi = (q0 + t < nq) ? q0 + t : nq - 1;
            v[t] = lut[(size_t)qi * M * RC_K + i];
        }
        if constexpr (QT == 1) tab[i] = v[0];
        if constexpr (QT == 2) tab[i] = make_float2(v[0], v[1]);
        if constexpr (QT == 4) tab[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
    float tq[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) tq[t] = (MODE == ADC_FILTER && q0 + t < nq) ? thr[q0 + t] : INFINITY;
    __syncthreads();

    const int64_t total = (MODE == ADC_SAMPLE) ? S : N;
    const int64_t t0 = (int64_t)blockIdx.y * ADC_TILE_DOCS;
    const int64_t t1 = (t0 + ADC_TILE_DOCS < total) ? t0 + ADC_TILE_DOCS : total;
    for (int64_t i0 = t0; i0 < t1; i0 += ADC_THREADS) {   // wave-uniform trip count
        const int64_t i = i0 + tid;
        const bool live = i < t1;
        const int64_t ii = live ? i : (t1 - 1);
        int64_t n = ii;
        if constexpr (MODE == ADC_SAMPLE) n = (int64_t)(((uint64_t)ii * (uint64_t)N) / (uint64_t)S);  // ii < 2^15, N < 2^32
        unsigned w[M / 4];
        adc_load_code_bytes<M>(codes + n * M, w);
        float s[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) s[t] = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const unsigned c = (w[m >> 2] >> (8 * (m & 3))) & 0xFFu;
            adc_acc<QT>(s, tab[m * RC_K + c]);
        }
        if constexpr (MODE == ADC_SAMPLE) {
            if (live) {
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    if (q0 + t < nq) sample[(size_t)(q0 + t) * S + i] = s[t];
            }
        } else {
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const bool pass = live && (s[t] >= tq[t]);
                const unsigned long long mask = __ballot(pass);
                if (mask) {  // wave-uniform
                    const unsigned slot = adc_wave_append(mask, cand_count + q0 + t);
                    if (pass && slot < ADC_CAND_CAP)
                        cand[(size_t)(q0 + t) * ADC_CAND_CAP + slot] = adc_exact_key(s[t], n);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ 4b. screening
// the round-1 screens on the canonical codes: adc_qlut_kernel, adc_screen_kernel, adc_screen_mfma_kernel
#include "adc_screen_r1.h"

// One block per query: the per-m minimum of its tables into the qstat record, the common step and the integer threshold
// (the byte tables of the 16-query screen are written from the record by adc_qlut16_write_kernel)
__global__ __launch_bounds__(RC_K) void adc_qstats_kernel(const float* __restrict__ lut, const float* __restrict__ thr,
                                                          int M, float* __restrict__ qstat, int* __restrict__ tint) {
    __shared__ float s_lo[ADC_QSTAT_STRIDE];
    __shared__ float s_rng[ADC_QSTAT_STRIDE];
    __shared__ float s_abs[ADC_QSTAT_STRIDE];
    const int qi = blockIdx.x, c = threadIdx.x, lane = c & 63, wv = c >> 6;
    const float* lq = lut + (size_t)qi * M * RC_K;
    // a wave owns sub-quantisers wv, wv + 4, ...: four codes per lane, one wave reduction per sub-quantiser
    for (int m = wv; m < M; m += 4) {
        const float4 v = reinterpret_cast<const float4*>(lq + (size_t)m * RC_K)[lane];
        float lo = fminf(fminf(v.x, v.y), fminf(v.z, v.w)), hi = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o));
            hi = fmaxf(hi, __shfl_xor(hi, o));
        }
        if (lane == 0) {
            adc_qstat_of(qstat, qi)[m] = lo;
            s_lo[m] = lo;
            s_rng[m] = hi - lo;
            s_abs[m] = fmaxf(fabsf(lo), fabsf(hi));
        }
    }
    __syncthreads();
    if (c == 0) {
        const adc_table_sums sums = adc_table_summary(s_lo, s_rng, s_abs, M);
        adc_qstat_of(qstat, qi)[ADC_QSTAT_DELTA] = sums.delta;     // (the flat search needs no A / B later: tint is made here)
        tint[qi] = adc_screen_tint(thr[qi], sums, M);
    }
}

// the 16-query screen on the permuted image: adc_q16_image_kernel, adc_qlut16_write_kernel, adc_screen_q16_kernel
#include "adc_screen16.h"

// ------------------------------------------------------------------------------------------ host
struct adc_ws_layout {
    size_t lut, sample, thr, cnt, cand, qlut, tint, qstat, idcnt, ids, image, total;
    int64_t S;
};
#define ADC_TABLE_GROUP_QUERIES 16    // table groups are sized for 16 queries (covers the 8- and 4-query kernels)
// M with a permuted image = the M of the 16-query screen (and of the IVF screen): adc_cf_supported (adc_common.h)
static bool adc_use_image(int64_t N, int M) {
    return N >= ADC_SCREEN_MIN_N && adc_cf_supported(M) && !rc_env_set("RC_ADC_VALU_SCREEN") && !rc_env_set("RC_ADC_OLD_SCREEN");
}
static adc_ws_layout adc_layout(int64_t N, int M, int nq, bool own_image = true) {
    adc_ws_layout L;
    L.S = N < ADC_SAMPLE_MAX ? N : ADC_SAMPLE_MAX;
    size_t o = 0;
    L.lut = o;    o += rc_align_up((size_t)nq * M * RC_K * sizeof(float), 256);
    L.sample = o; o += rc_align_up((size_t)nq * (size_t)L.S * sizeof(float), 256);
    L.thr = o;    o += rc_align_up((size_t)nq * sizeof(float), 256);
    L.cnt = o;    o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
    L.cand = o;   o += rc_align_up((size_t)nq * ADC_CAND_CAP * sizeof(unsigned long long), 256);
    L.qlut = L.tint = L.qstat = L.idcnt = L.ids = o;
    if (N >= ADC_SCREEN_MIN_N) {
        const int QS = ADC_TABLE_GROUP_QUERIES;
        const size_t qb = (size_t)((nq + QS - 1) / QS) * M * RC_K * QS;
        L.qlut = o;  o += rc_align_up(qb, 256);
        L.tint = o;  o += rc_align_up((size_t)nq * sizeof(int), 256);
        L.qstat = o; o += rc_align_up((size_t)nq * ADC_QSTAT_STRIDE * sizeof(float), 256);
        L.idcnt = o; o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
        L.ids = o;   o += rc_align_up((size_t)nq * ADC_ID_CAP * sizeof(unsigned), 256);
    }
    L.image = o;
    if (own_image && N >= ADC_SCREEN_MIN_N && adc_cf_supported(M)) o += rc_align_up(rc_adc_scan_image_bytes(N, M), 256);
    L.total = o;
    return L;
}

extern "C" size_t rc_adc_search_ws_bytes(int64_t N, int M, int K, int nq, int k) {
    if (N <= 0 || M <= 0 || K != RC_K || nq <= 0 || k <= 0) return 0;
    return adc_layout(N, M, nq, true).total;
}
// workspace when the caller keeps the permuted code image itself (rc_adc_search_img with image != NULL)
extern "C" size_t rc_adc_search_img_ws_bytes(int64_t N, int M, int K, int nq, int k) {
    if (N <= 0 || M <= 0 || K != RC_K || nq <= 0 || k <= 0) return 0;
    return adc_layout(N, M, nq, false).total;
}
// Where a finished search left its per-query counts inside the caller's workspace (measurement only: SURVEY 8d asks for the
// screen's survivors next to queries/s): *survivors_off = byte offset of unsigned[nq] rows that passed the 8-bit screen
// (0 when the index is too small for a screen), *candidates_off = unsigned[nq] rows kept by the exact rescoring.
// own_image: the workspace of rc_adc_search_ws_bytes (1) or rc_adc_search_img_ws_bytes (0) — the offsets are the same.
extern "C" int rc_adc_search_ws_counts(int64_t N, int M, int K, int nq, size_t* survivors_off, size_t* candidates_off) {
    if (N <= 0 || M <= 0 || K != RC_K || nq <= 0 || !survivors_off || !candidates_off) return RC_EINVAL;
    const adc_ws_layout L = adc_layout(N, M, nq, false);
    *survivors_off = (N >= ADC_SCREEN_MIN_N) ? L.idcnt : 0;
    *candidates_off = L.cnt;
    return RC_OK;
}

// bytes of the permuted code image of an N-row index (0: this M has no image — M = 8, 12, 24 run the round-1 screens on the
// canonical codes): whole tiles of ADC_Q16_TILE rows, [tile][phase][round][wave][lane][chunk][step] (adc_q16_image_at)
extern "C" size_t rc_adc_scan_image_bytes(int64_t N, int M) {
    if (N < 0 || !adc_cf_supported(M)) return 0;
    const int64_t T = ADC_Q16_TILE;
    return (size_t)((N + T - 1) / T * T) * M;
}
// Host-side description of the conflict-free slot rule (adc_common.h; no GPU involved; what tests/test_abi.py checks): for
// lane `lane` (0..63) of a wave and gather step `step` (0 .. steps_per_lane-1) of a table phase of PM sub-quantisers (PM = M,
// 48 for M = 96): the 8-byte LDS slot it reads and the phase-relative sub-quantiser that slot belongs to.  Returns the number
// of steps per lane, or RC_ESHAPE.  (The IVF screen applies the rule to phases of 32 / 16: ivfs_pm, ivf_lists.hip.)
extern "C" int rc_adc_cf_describe(int M, int lane, int step, int* slot, int* m, int* slots_per_code, int* phases) {
    if (!adc_cf_supported(M)) return RC_ESHAPE;
    const int PM = M == 96 ? 48 : M;
    if (lane < 0 || lane > 63 || step < 0 || step >= PM / 4 || !slot || !m) return RC_EINVAL;
    adc_cf_step(PM, step, lane & 15, lane >> 4, *slot, *m);
    if (slots_per_code) *slots_per_code = 32 * (PM / 32 + (PM % 32) / 16);
    if (phases) *phases = M / PM;
    return PM / 4;
}

// (Re)build rows [n0, n0 + n) of the flat-search image (what rc_adc_search_img / rc_adc_search_q take) from the canonical
// codes [N, M] (both pointers = row 0 of the index): rc_adc_scan_image_bytes(N, M) bytes
extern "C" int rc_adc_scan_image(rc_handle_t h, const uint8_t* codes, int64_t n0, int64_t n, int M, uint8_t* image,
                                 rc_stream_t stream) {
    return adc_launch_image(h, adc_q16_image_kernel, codes, n0, n, M, image, stream);
}
// ---- selections (subset search): the codes of rows[0 .. ns) compact, and their image.  Kernel and layouts: adc_select.h
#include "adc_select.h"
// the compact codes alone, byte by byte, for the M without an image (any width; the round-1 screens, the run-time-width scan and
// the exact route read canonical rows only): a block takes the same 128 rows and reads their entries of rows[] once
__global__ __launch_bounds__(ADC_SEL_THREADS) void adc_select_bytes_kernel(const uint8_t* __restrict__ codes, int M,
                                                                           const int64_t* __restrict__ rows, int64_t ns,
                                                                           uint8_t* __restrict__ sel_codes) {
    __shared__ int64_t s_rows[ADC_SEL_ROWS];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * ADC_SEL_ROWS;
    const int nv = (ns - i0) < ADC_SEL_ROWS ? (int)(ns - i0) : ADC_SEL_ROWS;
    if (tid < nv) s_rows[tid] = rows[i0 + tid];
    __syncthreads();
    for (int e = tid; e < nv * M; e += ADC_SEL_THREADS) sel_codes[i0 * M + e] = codes[s_rows[e / M] * M + e % M];
}
// layout: 0 = rc_adc_scan_image's (flat search), 1 = rc_adc_scan_image_rows', 2 = rc_adc_scan_image_rows16's (IVF screens).
// sel_codes [ns, M] and sel_image (the layout's bytes for ns rows) are written for the rows rows[0 .. ns) of codes [N, M]; either
// may be NULL, and an M without an image has none to ask for.  The order of the checks is part of the C ABI: shapes, then ns,
// then pointers (for an M with an image all three 16-byte aligned), then device work.  rows is never read on the host.
extern "C" int rc_adc_select_rows(rc_handle_t h, const uint8_t* codes, int64_t N, int M, const int64_t* rows, int64_t ns,
                                  int layout, uint8_t* sel_codes, uint8_t* sel_image, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll || M < 1 || M > 1024 || layout < 0 || layout > 2 || (sel_image && !adc_cf_supported(M))) return RC_ESHAPE;
    if (ns < 1 || ns > N) return RC_EINVAL;
    if (!h || !codes || !rows || (!sel_codes && !sel_image)) return RC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (!adc_cf_supported(M)) {
        hipLaunchKernelGGL(adc_select_bytes_kernel, dim3((unsigned)((ns + ADC_SEL_ROWS - 1) / ADC_SEL_ROWS)), dim3(ADC_SEL_THREADS),
                           0, s, codes, M, rows, ns, sel_codes);
        RC_LAUNCH_CHECK(h);
        return RC_OK;
    }
    if ((((uintptr_t)codes | (uintptr_t)sel_codes | (uintptr_t)sel_image) & 15) != 0) return RC_EINVAL;
    if (layout == 0 || !sel_image) return adc_select_launch<adc_sel_flat>(h, codes, M, rows, ns, sel_codes, sel_image, s);
    return adc_select_rows_ivf(h, codes, M, rows, ns, layout == 2, sel_codes, sel_image, s);
}
// host-side description of the 16-query screen's layout (tests): slot read by `lane` in step j, or RC_ESHAPE
extern "C" int rc_adc_q16_describe(int M, int lane, int step, int* slot) {
    if (!adc_cf_supported(M)) return RC_ESHAPE;
    if (lane < 0 || lane > 63 || step < 0 || step > 3 || !slot) return RC_EINVAL;
    *slot = adc_q16_slot(lane, step);
    return 1;                                                // every M with an image uses the layout
}
// The 16-query screen's block -> (group, tile) map for nq queries (M with an image): true = the TILES are dealt to the XCDs and
// every XCD takes all groups (kernel flag 2), false = XCD x owns the groups == x (mod 8) and walks every tile.  The limit is read
// from the environment on every call.  Why and what it measured: at the launch, adc_launch_scans.
static bool adc_q16_by_tiles(int M, int nq) {
    const int groups = (nq + 15) / 16;
    const int by_tiles_max = rc_env_int("RC_ADC_Q16_TILESPLIT_GROUPS", 64 / (M / 16));
    return groups < 8 || groups <= by_tiles_max;
}
// host-side statement of that choice (tests): 1 = tiles dealt, 0 = groups dealt, RC_ESHAPE for an M without an image
extern "C" int rc_adc_q16_by_tiles(int M, int nq) {
    if (!adc_cf_supported(M)) return RC_ESHAPE;
    if (nq < 1) return RC_EINVAL;
    return adc_q16_by_tiles(M, nq) ? 1 : 0;
}

struct adc_bufs {
    float* lut; float* sample; float* thr; unsigned* cnt; unsigned long long* cand;
    uint8_t* qlut; int* tint; unsigned* idcnt; unsigned* ids; float* qstat;
};

template <int M, int QT>
static int adc_launch_scans(rc_handle_t h, const uint8_t* codes, const uint8_t* image, int64_t N, int nq, int64_t S,
                            const adc_bufs& b, int r, int k, int* status, int* qstatus, hipStream_t s) {
    const size_t lds = (size_t)M * RC_K * QT * sizeof(float);
    const unsigned qg = (unsigned)((nq + QT - 1) / QT);
    auto ksample = adc_scan_kernel<M, QT, ADC_SAMPLE>;
    auto kfilter = adc_scan_kernel<M, QT, ADC_FILTER>;
    RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)ksample, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ksample, dim3(qg, (unsigned)((S + ADC_TILE_DOCS - 1) / ADC_TILE_DOCS)), dim3(ADC_THREADS), lds, s,
                       codes, N, b.lut, nq, S, b.sample, b.thr, b.cnt, b.cand);
    RC_LAUNCH_CHECK(h);
    const int trc = rc_adc_launch_threshold(h, b.sample, S, nq, r, b.thr, s);
    if (trc != RC_OK) return trc;
    const unsigned tiles = (unsigned)((N + ADC_TILE_DOCS - 1) / ADC_TILE_DOCS);
    // small indexes: exact scan (the screen's fixed costs do not pay)
    if (N < ADC_SCREEN_MIN_N) {
        RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)kfilter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
        hipLaunchKernelGGL(kfilter, dim3(qg, tiles), dim3(ADC_THREADS), lds, s, codes, N, b.lut, nq, S, b.sample, b.thr,
                           b.cnt, b.cand);
        rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
        RC_LAUNCH_CHECK(h);
        return RC_OK;
    }
    RC_HIP_CHECK(h, hipMemsetAsync(b.idcnt, 0, (size_t)nq * sizeof(unsigned), s));
    // Screen variant: widths with an image (ADC_CF_WIDTHS) run the 16-query screen on it; without an image (M = 8, 24, or
    // RC_ADC_OLD_SCREEN) the round-1 matrix-core screen on the canonical codes; M % 8 != 0 and RC_ADC_VALU_SCREEN the VALU one.
    const bool valu_screen = rc_env_set("RC_ADC_VALU_SCREEN");
    auto screen = [&](auto kern, int QS, size_t sl) -> int {
        hipLaunchKernelGGL(adc_qlut_kernel, dim3((unsigned)nq), dim3(RC_K), 0, s, b.lut, b.thr, M, QS, b.qlut, b.tint);
        RC_LAUNCH_CHECK(h);
        RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl));
        rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
        hipLaunchKernelGGL(kern, dim3((unsigned)((nq + QS - 1) / QS), tiles), dim3(ADC_THREADS), sl, s, codes, N, b.qlut,
                           b.tint, nq, b.idcnt, b.ids);
        rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
        RC_LAUNCH_CHECK(h);
        return RC_OK;
    };
    constexpr int QS1 = (M <= 64) ? 8 : 4;                  // one-pass kernels: M * 256 * QS bytes of LDS
    int src = RC_OK;
    constexpr bool CF = adc_cf_supported(M);
    if (CF && image != nullptr) {
        if constexpr (CF) {
            // 16 queries per ds_read_b128 gather, phases of 16 sub-quantisers, double-buffered tables (adc_screen_q16_kernel)
            auto kern = adc_screen_q16_kernel<M>;
            constexpr int TH = ADC_Q16_WAVES * 64;
            constexpr int sl = 2 * RC_K * 256 + ADC_Q16_WAVES * ADC_Q16_SCAP * 4;      // two table buffers + the survivor lists
            const int groups = (nq + 15) / 16;
            hipLaunchKernelGGL(adc_qstats_kernel, dim3((unsigned)nq), dim3(RC_K), 0, s, b.lut, b.thr, M, b.qstat, b.tint);
            RC_LAUNCH_CHECK(h);
            hipLaunchKernelGGL(adc_qlut16_write_kernel, dim3((unsigned)groups, RC_K / 64, M / 16), dim3(64, 16), 0, s, b.lut,
                               (const float*)b.qstat, M, nq, b.qlut);
            RC_LAUNCH_CHECK(h);
            RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, sl));
            const unsigned tiles16 = (unsigned)((N + ADC_Q16_TILE - 1) / ADC_Q16_TILE);
            const unsigned gpx = (unsigned)(groups + 7) / 8u;
            // block -> (group, tile).  Many groups: XCD x owns the groups == x (mod 8) and walks every tile — each XCD streams the
            // whole image (8 x N M bytes from HBM per launch: nothing beside 1200 queries' gathers).  Few groups (round 6): with
            // 8 groups that traffic IS the launch (3.4 GB per 128-query search: 1.04 ms where 8 / 75 of a full launch is 0.78), so
            // while all the groups' tables fit an XCD's L2 (groups x M / 16 x 64 KiB <= 4 MiB) the TILES are dealt to the XCDs and
            // every XCD takes all groups: the image is read once.  [MI355X] ms per search, k = 200, M = 48: 128 queries 1.27 -> 1.15,
            // 256: 1.91 -> 1.80, 384: 2.71 -> 2.63, 512: 3.30 -> 3.34 (not used there); M = 32 / 96 at 128 queries: 1.02 -> 0.94,
            // 2.20 -> 2.04 (profiles/r06s_adc_small_batches.txt).
            const bool by_tiles = adc_q16_by_tiles(M, nq);     // RC_ADC_Q16_TILESPLIT_GROUPS; what rc_adc_q16_by_tiles reports
            const unsigned nblocks = !by_tiles ? 8u * gpx * tiles16 : 8u * (unsigned)groups * ((tiles16 + 7u) / 8u);
            rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
            hipLaunchKernelGGL(kern, dim3(nblocks), dim3(TH), sl, s, image, N, b.qlut, b.tint, nq, groups, b.idcnt, b.ids,
                               (rc_env_int("RC_ADC_Q16_PRIO", 1) ? 1 : 0) | (by_tiles ? 2 : 0));
            rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
            RC_LAUNCH_CHECK(h);
        }
    } else if constexpr (M % 8 == 0) {
        // M without an image (8, 24; or RC_ADC_OLD_SCREEN=1, the tests' A/B partner): the round-1 screens on the canonical codes
        if (!valu_screen) src = screen(adc_screen_mfma_kernel<M, QS1>, QS1, (size_t)M * RC_K * QS1);
        else src = screen(adc_screen_kernel<M, QS1>, QS1, (size_t)M * RC_K * QS1);
    } else {
        src = screen(adc_screen_kernel<M, QS1>, QS1, (size_t)M * RC_K * QS1);
    }
    if (src != RC_OK) return src;
    auto krescore = adc_rescore_kernel<M>;
    const size_t rl = (size_t)M * RC_K * sizeof(float);
    RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)krescore, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rl));
    hipLaunchKernelGGL(krescore, dim3((unsigned)nq), dim3(adc_rescore_threads(M)), rl, s, codes, b.lut, b.thr, b.idcnt, b.ids, b.cnt, b.cand,
                       status, (const int64_t*)nullptr, qstatus);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

#define ADC_CASE(MM, QQ) \
    case MM: rc = adc_launch_scans<MM, QQ>(h, codes, image, N, nq, L.S, bufs, r, k, status, qstatus, s); break;

template <bool L2>
static int adc_launch_lut(rc_handle_t h, const float* C, const float* q, int nq, int D, int M, int K, float* lut,
                          rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !C || !q || !lut || nq < 0 || M <= 0 || D <= 0) return RC_EINVAL;
    if (K != RC_K || D % M != 0) return RC_ESHAPE;
    if (nq == 0) return RC_OK;
    const dim3 cg((unsigned)((nq + ADC_LUT_QCHUNK - 1) / ADC_LUT_QCHUNK), (unsigned)M);
    switch (D / M) {
#define ADC_LUT_CASE(DS)                                                                                                  \
        case DS:                                                                                                          \
            hipLaunchKernelGGL((adc_lut_rows_kernel<DS, L2>), cg, dim3(RC_K), 0, (hipStream_t)stream, C, q, nq, D, M, lut); \
            break;
        ADC_LUT_CASE(8) ADC_LUT_CASE(12) ADC_LUT_CASE(16) ADC_LUT_CASE(24) ADC_LUT_CASE(32) ADC_LUT_CASE(48)
        ADC_LUT_CASE(64) ADC_LUT_CASE(96)
#undef ADC_LUT_CASE
        default:
            hipLaunchKernelGGL(adc_lut_kernel<L2>, dim3((unsigned)nq, (unsigned)M), dim3(RC_K), 0, (hipStream_t)stream, C, q, D,
                               M, lut);
    }
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
extern "C" int rc_adc_lut(rc_handle_t h, const float* C, const float* q, int nq, int D, int M, int K, float* lut,
                          rc_stream_t stream) {
    return adc_launch_lut<false>(h, C, q, nq, D, M, K, lut, stream);
}
// the L2 tables S = 0.0f - T (adc_lut_step): what rc_adc_search_l2_q / _exact and the IVF entries of an L2 index score with
extern "C" int rc_adc_lut_l2(rc_handle_t h, const float* C, const float* q, int nq, int D, int M, int K, float* lut,
                             rc_stream_t stream) {
    return adc_launch_lut<true>(h, C, q, nq, D, M, K, lut, stream);
}

// L2 metric, the one trailing kernel: the searches ran on s = -d; d = 0.0f - s over the nq * k outputs (+0.0f for a zero
// distance, +inf for the -inf of the slots past N)
__global__ __launch_bounds__(256) void adc_l2_distances_kernel(float* __restrict__ v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = 0.0f - v[i];
}
static int adc_finish(rc_handle_t h, bool l2, float* scores, int64_t n, hipStream_t s) {
    if (!l2) return RC_OK;
    hipLaunchKernelGGL(adc_l2_distances_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scores, n);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// The search proper.  scan_image: the index's permuted code image (rc_adc_scan_image) or NULL — then, where the
// conflict-free screen applies, the image is rebuilt in the workspace on every call (one extra pass over the codes).
// qstatus: NULL, or nq ints (zeroed by the caller) that receive the status bits PER QUERY (bit0 too few candidates, bit1 a
// list overflowed), so that a caller repeats or re-routes only the queries concerned (rc_adc_search_exact never fails).
// l2: the metric selects the table builder and the trailing adc_l2_distances_kernel, nothing in between.
static int adc_search_body(bool l2, rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                           const float* C, int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                           float* scores, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                           rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !codes || !C || !q || !scores || !ids || !status || N <= 0 || nq < 0 || k <= 0 || M <= 0 || D <= 0)
        return RC_EINVAL;
    if (K != RC_K || D % M != 0 || N > 0xFFFFFFFFll || k > ADC_CAND_CAP / 2) return RC_ESHAPE;
    if (nq == 0) return RC_OK;
    const adc_ws_layout L = adc_layout(N, M, nq, scan_image == nullptr);
    if (!ws || ws_bytes < L.total) return RC_EWORKSPACE;
    char* w = (char*)ws;
    const uint8_t* image = nullptr;
    if (adc_use_image(N, M)) {
        image = scan_image;
        if (!image) {
            const int irc = rc_adc_scan_image(h, codes, 0, N, M, (uint8_t*)(w + L.image), stream);
            if (irc != RC_OK) return irc;
            image = (const uint8_t*)(w + L.image);
        }
    }
    float* lut = (float*)(w + L.lut);
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    const adc_bufs bufs = {lut, (float*)(w + L.sample), (float*)(w + L.thr), cnt, cand, (uint8_t*)(w + L.qlut),
                           (int*)(w + L.tint), (unsigned*)(w + L.idcnt), (unsigned*)(w + L.ids), (float*)(w + L.qstat)};
    hipStream_t s = (hipStream_t)stream;
    int rc = l2 ? rc_adc_lut_l2(h, C, q, nq, D, M, K, lut, stream) : rc_adc_lut(h, C, q, nq, D, M, K, lut, stream);
    if (rc != RC_OK) return rc;
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    // rank of the sample score used as the filter threshold
    const int r = rc_adc_sample_rank(N, L.S, k, sel_slack);
    switch (M) {
        ADC_SEARCH_WIDTHS(ADC_CASE)
        default: return RC_ESHAPE;
    }
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_select(h, cand, cnt, nq, N, k, id_offset, scores, ids, status, s, qstatus);
    if (rc != RC_OK) return rc;
    return adc_finish(h, l2, scores, (int64_t)nq * k, s);
}

extern "C" int rc_adc_search_q(rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                               const float* C, int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                               float* scores, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                               rc_stream_t stream) {
    return adc_search_body(false, h, codes, scan_image, N, M, K, C, D, q, nq, k, id_offset, sel_slack, scores, ids, status,
                           qstatus, ws, ws_bytes, stream);
}
// The same search under the L2 metric (include/repconc_hip.h): distances ascending, ties by the lower id, +inf / -1 past N
extern "C" int rc_adc_search_l2_q(rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                                  const float* C, int D, const float* q, int nq, int k, int64_t id_offset, double sel_slack,
                                  float* scores, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                                  rc_stream_t stream) {
    return adc_search_body(true, h, codes, scan_image, N, M, K, C, D, q, nq, k, id_offset, sel_slack, scores, ids, status,
                           qstatus, ws, ws_bytes, stream);
}

extern "C" int rc_adc_search_img(rc_handle_t h, const uint8_t* codes, const uint8_t* scan_image, int64_t N, int M, int K,
                                 const float* C, int D, const float* q, int nq, int k, int64_t id_offset,
                                 double sel_slack, float* scores, int64_t* ids, int* status, void* ws, size_t ws_bytes,
                                 rc_stream_t stream) {
    return rc_adc_search_q(h, codes, scan_image, N, M, K, C, D, q, nq, k, id_offset, sel_slack, scores, ids, status, nullptr,
                           ws, ws_bytes, stream);
}

extern "C" int rc_adc_search(rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C, int D,
                             const float* q, int nq, int k, int64_t id_offset, double sel_slack, float* scores,
                             int64_t* ids, int* status, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    return rc_adc_search_img(h, codes, nullptr, N, M, K, C, D, q, nq, k, id_offset, sel_slack, scores, ids, status, ws,
                             ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------ exact search (never fails)
// evaluate_repconc.py:180-185 relies on Faiss's IndexPQ.search, which returns for ANY index content.  The fast path above
// places a candidate threshold from a sample and can, on degenerate data (thousands of rows with identical codes, all rows
// tied), keep too few or too many candidates however the slack is set.  This path has no such failure mode: exact fp32
// scores of every row (adc_scan_kernel<SAMPLE> with the sample = the whole index), then the k-th largest 64-bit key
// (ordered(score) << 32 | ~row: distinct for distinct rows, so "the k best in (score desc, id asc) order" is a unique set)
// by an 8-pass byte-wise radix select over all rows, then a compaction of the keys >= that key (exactly min(k, N) of them)
// and the ordinary sort + emit.  Cost: N x 4 bytes of scores per query and ~10 passes over them — for the handful of
// queries the fast path hands over, not for whole batches.
#define ADC_EXACT_QX 8             // queries per round (scores [QX][N] fp32 in the workspace)

struct adc_exact_layout { size_t lut, sc; topk_exact_layout sel; };      // sel.total = bytes of the whole workspace
static adc_exact_layout adc_exact_ws(int64_t N, int M, int nq) {
    adc_exact_layout L;
    size_t o = 0;
    const int qx = nq < ADC_EXACT_QX ? nq : ADC_EXACT_QX;
    L.lut = o;    o += rc_align_up((size_t)nq * M * RC_K * sizeof(float), 256);
    L.sc = o;     o += rc_align_up((size_t)qx * (size_t)N * sizeof(float), 256);
    L.sel = topk_exact_ws(o, qx);
    return L;
}
extern "C" size_t rc_adc_search_exact_ws_bytes(int64_t N, int M, int K, int nq, int k) {
    if (N <= 0 || M <= 0 || K != RC_K || nq <= 0 || k <= 0) return 0;
    return adc_exact_ws(N, M, nq).sel.total;
}

// Any other M (the reference's IndexPQ takes every divisor of the hidden size: modeling_repconc.py:41, evaluate_repconc.py:81):
// exact scores with a run-time width — thread = row, the row's codes walked once for up to ADC_EXACT_QX queries, tables read
// through the caches (M x 1 KiB per query: no LDS size fits every M), m-ascending fp32 sums like every other scoring path.
__global__ __launch_bounds__(256) void adc_scan_rt_kernel(const uint8_t* __restrict__ codes, int64_t N, int M,
                                                          const float* __restrict__ lut, int nq, float* __restrict__ sc) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const uint8_t* cp = codes + n * M;
    float s[ADC_EXACT_QX];
#pragma unroll
    for (int t = 0; t < ADC_EXACT_QX; ++t) s[t] = 0.f;
    for (int m = 0; m < M; ++m) {
        const unsigned c = cp[m];
#pragma unroll
        for (int t = 0; t < ADC_EXACT_QX; ++t)
            if (t < nq) s[t] = s[t] + lut[((size_t)t * M + m) * RC_K + c];
    }
#pragma unroll
    for (int t = 0; t < ADC_EXACT_QX; ++t)
        if (t < nq) sc[(size_t)t * N + n] = s[t];
}

template <int M, int QT>
static int adc_exact_scores(rc_handle_t h, const uint8_t* codes, int64_t N, const float* lut, int nq, float* sc, hipStream_t s) {
    const size_t lds = (size_t)M * RC_K * QT * sizeof(float);
    auto kern = adc_scan_kernel<M, QT, ADC_SAMPLE>;
    RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((nq + QT - 1) / QT), (unsigned)((N + ADC_TILE_DOCS - 1) / ADC_TILE_DOCS)),
                       dim3(ADC_THREADS), lds, s, codes, N, lut, nq, N, sc, (const float*)nullptr, (unsigned*)nullptr,
                       (unsigned long long*)nullptr);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

static int adc_search_exact_body(bool l2, rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C, int D,
                                 const float* q, int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                 size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !codes || !C || !q || !scores || !ids || N <= 0 || nq < 0 || k <= 0 || M <= 0 || D <= 0) return RC_EINVAL;
    if (K != RC_K || D % M != 0 || N > 0xFFFFFFFFll || k > ADC_CAND_CAP / 2) return RC_ESHAPE;
    if (nq == 0) return RC_OK;
    const adc_exact_layout L = adc_exact_ws(N, M, nq);
    if (!ws || ws_bytes < L.sel.total) return RC_EWORKSPACE;
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    float* lut = (float*)(w + L.lut);
    float* sc = (float*)(w + L.sc);
    int rc = l2 ? rc_adc_lut_l2(h, C, q, nq, D, M, K, lut, stream) : rc_adc_lut(h, C, q, nq, D, M, K, lut, stream);
    if (rc != RC_OK) return rc;
    for (int q0 = 0; q0 < nq; q0 += ADC_EXACT_QX) {
        const int nx = nq - q0 < ADC_EXACT_QX ? nq - q0 : ADC_EXACT_QX;
        const float* lq = lut + (size_t)q0 * M * RC_K;
        switch (M) {
#define ADC_EXACT_CASE(MM, QQ) case MM: rc = adc_exact_scores<MM, QQ>(h, codes, N, lq, nx, sc, s); break;
            ADC_SEARCH_WIDTHS(ADC_EXACT_CASE)
#undef ADC_EXACT_CASE
            default:
                hipLaunchKernelGGL(adc_scan_rt_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, codes, N, M, lq, nx, sc);
                RC_LAUNCH_CHECK(h);
                rc = RC_OK;
        }
        if (rc != RC_OK) return rc;
        rc = topk_exact_select(h, sc, N, nx, k, id_offset, w, L.sel, scores + (size_t)q0 * k, ids + (size_t)q0 * k, s);
        if (rc != RC_OK) return rc;
    }
    return adc_finish(h, l2, scores, (int64_t)nq * k, s);
}

extern "C" int rc_adc_search_exact(rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C, int D,
                                   const float* q, int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                   size_t ws_bytes, rc_stream_t stream) {
    return adc_search_exact_body(false, h, codes, N, M, K, C, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream);
}
extern "C" int rc_adc_search_l2_exact(rc_handle_t h, const uint8_t* codes, int64_t N, int M, int K, const float* C, int D,
                                      const float* q, int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                      size_t ws_bytes, rc_stream_t stream) {
    return adc_search_exact_body(true, h, codes, N, M, K, C, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream);
}
