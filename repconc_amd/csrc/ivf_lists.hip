// List-centric IVF search (BASELINE configs[3]: nlist = 5000, M = 96): the per-query tables, sample / rank-select thresholds,
// the bucket kernel, the device-side plan, the launch and the entry points rc_ivf_search_lists / rc_ivf_search_probes*.  The two
// pipelined screens over the cells' rows are headers included here: ivfs_screen8.h (8 queries per task and gather,
// ivfs_screen_kernel) and ivfs_screen16.h (16, ivfs_screen16_kernel), with what they share in ivfs_common.h; the caller
// (IVFPQIndex.search) picks the width per call.  Split from adc_search.hip in round 4; shares adc_common.h with the flat search.
#include "adc_common.h"
#include "ivf_plan.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#include <type_traits>

// =============================================================================================== IVF, list-centric
// Search of the cell-major IVF index (csrc/ivf_search.hip; a build-side extension, the reference has one list) with the
// machinery of the flat search.  Round 1 scanned every probed cell once per query (one block per query slice, fp32
// tables, dense score write-out + radix select over it).  Here the work is organised by CELL: all queries probing a cell
// are split into groups of up to W = 8 or 16 (the screen's width), one (cell, group) TASK runs the 8-bit screen over the
// cell's rows — W queries share every gather, the cell's codes are read once per group — and the survivors are re-scored
// exactly and selected like in the flat search:
//   1. adc_lut                     fp32 tables of every query (caller)
//   2. ivf_sample_scan_kernel      exact scores of every SS-th row of the query's probed cells -> sample[q][..]
//   3. ivfs_qprep_kernel           per query: table statistics + 8-bit tables
//   4. ivf_rank_select_kernel      tau_q = rank_q-th largest sample score (rank 0: -inf, every probed row is a candidate)
//                                  and the integer threshold from tau_q and the statistics of step 3
//   5. ivfs_screen_kernel | ivfs_screen16_kernel   persistent blocks walk the tasks: tables transposed into LDS by loader
//                                  waves, 8-bit screen, survivors to per-wave streams; ivfs_bucket_kernel deals them per query
//   6. adc_rescore_kernel          exact fp32 score of the survivors, keys carry the corpus position of the row
//   7. adc_select_kernel           top-k, (score desc, corpus id asc) — the tie rule of the flat search
// The task list (cells sorted, W queries per task) and the sample ranks come from the host (rc_ivf_search_lists) or from
// the ivf_plan_* kernels (rc_ivf_search_probes*); status bit0 = a query kept fewer than min(k, rows probed) candidates (retry
// with more slack), bit1 = a list overflowed (less slack), bit2 = a survivor stream filled up.
#include "ivfs_screen8.h"
#include "ivfs_screen16.h"

// ------------------------------------------------------------------------------------ the screens' images
// bytes of the IVF image of N rows (whole chunks of 16 rows)
extern "C" size_t rc_adc_scan_image_rows_bytes(int64_t N, int M) {
    if (!adc_cf_supported(M) || N < 0) return 0;
    return (size_t)((N + 15) / 16 * 16) * M;
}
// host-side description of that image (no GPU involved): byte offset of codes[n][m], or -1
extern "C" int64_t rc_adc_scan_image_rows_at(int M, int64_t n, int m) {
    if (!adc_cf_supported(M) || n < 0 || m < 0 || m >= M) return -1;
    const int p = m / 32, PM = (M - 32 * p) >= 32 ? 32 : 16;
    for (int g = 0; g < 4; ++g)
        for (int st = 0; st < PM / 4; ++st) {
            int slot, mm;
            adc_cf_step(PM, st, (int)(n & 15), g, slot, mm);
            if (mm == m - 32 * p) return (n >> 4) * (int64_t)(16 * M) + 16 * 32 * p + (g * 16 + (int)(n & 15)) * (PM / 4) + st;
        }
    return -1;
}
extern "C" int rc_adc_scan_image_rows(rc_handle_t h, const uint8_t* codes, int64_t n0, int64_t n, int M, uint8_t* image,
                                      rc_stream_t stream) {
    return adc_launch_image(h, ivfs_image_kernel, codes, n0, n, M, image, stream);
}
// the same three for the 16-query screen's image (ivfs16_image_at)
extern "C" size_t rc_adc_scan_image_rows16_bytes(int64_t N, int M) {
    if (!adc_cf_supported(M) || N < 0) return 0;
    return (size_t)((N + 15) / 16 * 16) * M;
}
// host-side description of that image (no GPU involved): byte offset of codes[n][m], or -1
extern "C" int64_t rc_adc_scan_image_rows16_at(int M, int64_t n, int m) {
    if (!adc_cf_supported(M) || n < 0 || m < 0 || m >= M) return -1;
    const int p16 = m / 16;
    for (int g = 0; g < 4; ++g)
        for (int j = 0; j < 4; ++j)
            if (adc_q16_slot((int)(n & 15) + 16 * g, j) == m % 16) return ivfs16_image_at(M, n, p16, g, j);
    return -1;
}
extern "C" int rc_adc_scan_image_rows16(rc_handle_t h, const uint8_t* codes, int64_t n0, int64_t n, int M, uint8_t* image,
                                        rc_stream_t stream) {
    return adc_launch_image(h, ivfs16_image_kernel, codes, n0, n, M, image, stream);
}
// a selection's compact codes and their image in one of the two layouts above (rc_adc_select_rows, adc_search.hip, has checked
// the arguments)
#include "adc_select.h"
int adc_select_rows_ivf(rc_handle_t h, const uint8_t* codes, int M, const int64_t* rows, int64_t ns, int wide, uint8_t* sel_codes,
                        uint8_t* sel_image, hipStream_t s) {
    return wide ? adc_select_launch<adc_sel_rows16>(h, codes, M, rows, ns, sel_codes, sel_image, s)
                : adc_select_launch<adc_sel_rows>(h, codes, M, rows, ns, sel_codes, sel_image, s);
}

// per-query byte tables, [phase][code][PMp] one biased byte per sub-quantiser (phase p starts at byte 256 * 32 p):
// Round 4: adc_qstats_kernel + ivfs_qbyte_write_kernel in one pass over the query's LUT.  Block (256 codes, M / 16): thread
// (c, b) keeps lut[16 b + j][c], j < 16, in registers; lo / hi per sub-quantiser by wave reductions + LDS, delta = the
// largest range / 255 (adc_screen_delta), then the bytes are quantised from the registers.  The integer
// threshold needs tau and is computed where tau is (ivf_rank_select_kernel).  One read of the LUT instead of two, one launch
// instead of two, 6 x the threads (26 + 42 -> ~25 us per 1200 queries at M = 96).
__global__ __launch_bounds__(1024) void ivfs_qprep_kernel(const float* __restrict__ lut, int M, float* __restrict__ qstat,
                                                          uint8_t* __restrict__ qbyte) {
    __shared__ float s_lo[16][ADC_QSTAT_STRIDE], s_hi[16][ADC_QSTAT_STRIDE];
    __shared__ float s_mlo[ADC_QSTAT_STRIDE];
    __shared__ float s_delta;
    // block (256 codes, ceil(M / 32)): thread (c, y) holds the 16-blocks b = 2 y and 2 y + 1 (= table phase y of the screen)
    const int qi = blockIdx.x, c = threadIdx.x, y = threadIdx.y, lane = c & 63, wc = c >> 6;
    const float* lq = lut + (size_t)qi * M * RC_K;
    const int nb = (M / 16 - 2 * y) < 2 ? (M / 16 - 2 * y) : 2;       // 16-blocks of this thread row: 1 or 2
    float v[2][16];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 16; ++j) v[h][j] = (h < nb) ? lq[(32 * y + 16 * h + j) * RC_K + c] : 0.f;
    // min / max over the 256 codes: DPP rotations inside each row of 16 lanes (plain VALU; a butterfly of __shfl_xor is 12
    // LDS-crossbar operations per value), then 16 partials per sub-quantiser through LDS
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h < nb) {                                                  // uniform over the thread row
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float lo = v[h][j], hi = v[h][j];
                lo = fminf(lo, __int_as_float(rc_dpp_row_ror<8>(__float_as_int(lo))));
                hi = fmaxf(hi, __int_as_float(rc_dpp_row_ror<8>(__float_as_int(hi))));
                lo = fminf(lo, __int_as_float(rc_dpp_row_ror<4>(__float_as_int(lo))));
                hi = fmaxf(hi, __int_as_float(rc_dpp_row_ror<4>(__float_as_int(hi))));
                lo = fminf(lo, __int_as_float(rc_dpp_row_ror<2>(__float_as_int(lo))));
                hi = fmaxf(hi, __int_as_float(rc_dpp_row_ror<2>(__float_as_int(hi))));
                lo = fminf(lo, __int_as_float(rc_dpp_row_ror<1>(__float_as_int(lo))));
                hi = fmaxf(hi, __int_as_float(rc_dpp_row_ror<1>(__float_as_int(hi))));
                if ((lane & 15) == 0) {
                    s_lo[4 * wc + (lane >> 4)][32 * y + 16 * h + j] = lo;
                    s_hi[4 * wc + (lane >> 4)][32 * y + 16 * h + j] = hi;
                }
            }
        }
    }
    __syncthreads();
    const int t = y * RC_K + c;
    if (t < M) {
        float lo = s_lo[0][t], hi = s_hi[0][t];
#pragma unroll
        for (int r = 1; r < 16; ++r) { lo = fminf(lo, s_lo[r][t]); hi = fmaxf(hi, s_hi[r][t]); }
        s_mlo[t] = lo;
        adc_qstat_of(qstat, qi)[t] = lo;
        s_lo[0][t] = hi - lo;
        s_hi[0][t] = fmaxf(fabsf(lo), fabsf(hi));
    }
    __syncthreads();
    if (t == 0) {
        const adc_table_sums sums = adc_table_summary(s_mlo, s_lo[0], s_hi[0], M);
        adc_qstat_put_summary(adc_qstat_of(qstat, qi), sums);
        s_delta = sums.delta;
    }
    __syncthreads();
    const float delta = s_delta;
    const int PM = ivfs_pm(M, y);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h < nb) {
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                w[j >> 2] |= (adc_quant8(v[h][j], s_mlo[32 * y + 16 * h + j], delta) ^ 0x80u) << (8 * (j & 3));
            *reinterpret_cast<uint4*>(qbyte + (size_t)qi * M * RC_K + (size_t)RC_K * 32 * y + (size_t)c * PM + 16 * h) =
                make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// the integer threshold of a query from tau and the statistics ivfs_qprep_kernel left of its tables (adc_screen_tint, adc_common.h)
__device__ __forceinline__ int adc_tint_from(float t, const float* __restrict__ st, int M) {
    return adc_screen_tint(t, adc_qstat_summary(st), M);
}

// Deal the waves' (query, row) streams to the per-query id lists.  An atomic on one address takes ~0.2 us and the atomics
// of one address do not overlap: 2.4 M runs (one per wave, task and query) on 1200 counters cost 0.44 ms however many waves
// issue them.  The sixteen streams of ONE screen block hold the same (task, query) pairs, so one bucket block takes them
// all: a histogram over the queries in LDS (pass 1), ONE global atomic per query present (~600 of 1200 per block: 128 per
// counter over the whole grid), then every pair finds its slot with an LDS atomic (pass 2).
#define IVFS_BUCKET_THREADS 1024
__global__ __launch_bounds__(IVFS_BUCKET_THREADS) void ivfs_bucket_kernel(const unsigned* __restrict__ stream_cnt,
                                                                          const unsigned* __restrict__ stream, unsigned stream_cap,
                                                                          int nq, unsigned* __restrict__ id_count,
                                                                          unsigned* __restrict__ ids) {
    extern __shared__ unsigned bk_hist[];                     // [nq] pairs of the query in this block's streams, then its first slot
    const unsigned tid = threadIdx.x, wv = tid >> 6, l = tid & 63u;
    for (int q = (int)tid; q < nq; q += IVFS_BUCKET_THREADS) bk_hist[q] = 0u;
    __syncthreads();
    const unsigned sidx = blockIdx.x * IVFS_WAVES + wv;       // wave w of the bucket block reads stream w of the screen block
    const unsigned n = stream_cnt[sidx];
    const uint2* st = reinterpret_cast<const uint2*>(stream) + (size_t)sidx * stream_cap;
    for (unsigned i = l; i < n; i += 64u) atomicAdd(&bk_hist[st[i].x], 1u);
    __syncthreads();
    for (int q = (int)tid; q < nq; q += IVFS_BUCKET_THREADS) {
        const unsigned c = bk_hist[q];
        if (c) bk_hist[q] = atomicAdd(id_count + q, c);
    }
    __syncthreads();
    for (unsigned i = l; i < n; i += 64u) {
        const uint2 e = st[i];
        const unsigned slot = atomicAdd(&bk_hist[e.x], 1u);
        if (slot < ADC_ID_CAP) ids[(size_t)e.x * ADC_ID_CAP + slot] = e.y;
    }
}

// grid (nq, slices): the query's sample entries 0 .. scount[qi] are dealt to the threads of its blocks; an entry finds its
// cell by binary search over the query's sbase row (no per-cell loop: a probed cell contributes only a few dozen sampled
// rows, and walking the cells one after the other would serialise two dependent loads per cell).
// 1024 threads: the 4 M 256-byte table takes the CU's LDS, so the block is also the CU's whole occupancy.
// Round 4: the query's plan (sbase, first row of every probed cell) is staged in LDS beside the table — the binary search
// was log2(nprobe) DEPENDENT global loads per entry, most of a block's 12 us —, table and codes move in 16-byte pieces, two
// entries per thread are in flight, and a query gets one slice (one staging of its 4 M 256 bytes) unless the grid would
// not fill the chip.
#define IVF_SAMPLE_THREADS 1024
#define IVF_SAMPLE_PLAN_MAX 2048     // probes whose plan fits in LDS beside a 96 KiB table
template <int M>
__global__ __launch_bounds__(IVF_SAMPLE_THREADS) void ivf_sample_scan_kernel(const uint8_t* __restrict__ codes,
                                                              const int64_t* __restrict__ list_off,
                                                              const float* __restrict__ lut, const int* __restrict__ probes,
                                                              const int* __restrict__ sbase, const int* __restrict__ scount,
                                                              int nprobe, int64_t sstride, int ss,
                                                              float* __restrict__ sample) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tab = reinterpret_cast<float*>(smem);   // [M][256]
    int64_t* s_lo = reinterpret_cast<int64_t*>(smem + (size_t)M * RC_K * sizeof(float));   // [nprobe] first row of the cell
    int* s_sb = reinterpret_cast<int*>(s_lo + nprobe);                                      // [nprobe]
    const int qi = blockIdx.x, tid = threadIdx.x;
    const int n = scount[qi];
    const int* sb = sbase + (size_t)qi * nprobe;
    const int* pr = probes + (size_t)qi * nprobe;
    const bool plan_lds = nprobe <= IVF_SAMPLE_PLAN_MAX;     // block-uniform
    if (plan_lds)
        for (int p = tid; p < nprobe; p += IVF_SAMPLE_THREADS) { s_sb[p] = sb[p]; s_lo[p] = list_off[pr[p]]; }
    {
        const float4* l4 = reinterpret_cast<const float4*>(lut + (size_t)qi * M * RC_K);
        float4* t4 = reinterpret_cast<float4*>(tab);
        for (int i = tid; i < M * RC_K / 4; i += IVF_SAMPLE_THREADS) t4[i] = l4[i];
    }
    __syncthreads();
    const int step = gridDim.y * IVF_SAMPLE_THREADS;
    for (int i = blockIdx.y * IVF_SAMPLE_THREADS + tid; i < n; i += 2 * step) {
        int64_t row[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ih = (i + h * step < n) ? i + h * step : i;
            int lo = 0, hi = nprobe - 1;                              // last probe p with sbase[p] <= ih
            if (plan_lds) {
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_sb[mid] <= ih) lo = mid; else hi = mid - 1;
                }
                const int off = ih - s_sb[lo];
                // the sample of a cell: runs of 16 consecutive rows (coalesced reads), one run every 16 * ss rows
                row[h] = s_lo[lo] + (int64_t)(off >> 4) * 16 * ss + (off & 15);
            } else {
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (sb[mid] <= ih) lo = mid; else hi = mid - 1;
                }
                const int off = ih - sb[lo];
                row[h] = list_off[pr[lo]] + (int64_t)(off >> 4) * 16 * ss + (off & 15);
            }
        }
        const float s0 = adc_rescore_row<M>(codes + row[0] * M, tab);
        const float s1 = adc_rescore_row<M>(codes + row[1] * M, tab);
        sample[(size_t)qi * sstride + i] = s0;
        if (i + step < n) sample[(size_t)qi * sstride + i + step] = s1;
    }
}

// thr[qi] = rank[qi]-th largest of sample[qi][0 .. scount[qi]); rank <= 0 or > scount: -inf.  One block per query,
// 8 bits per pass over global memory (the sample is 1/SS of the probed rows).
__global__ __launch_bounds__(1024) void ivf_rank_select_kernel(const float* __restrict__ sample, const int* __restrict__ scount,
                                                               const int* __restrict__ rank, int64_t sstride,
                                                               float* __restrict__ thr, const float* __restrict__ qstat = nullptr,
                                                               int M = 0, int* __restrict__ tint = nullptr) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_aux[8];
    __shared__ unsigned s_scan[4];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const int n = scount[qi], k = rank[qi];
    if (k <= 0 || k > n) {
        if (tid == 0) {
            thr[qi] = -INFINITY;
            if (tint) tint[qi] = INT_MIN;
        }
        return;
    }
    // a few thousand scores in global memory: four plain passes (the value-space cut of adc_kth_largest_v costs more barriers
    // and one more pass than it saves at this length: 18 -> 26 us per 1200 queries at nprobe 8)
    const float* row = sample + (size_t)qi * sstride;
    unsigned* s_sel = s_aux;
    if (tid == 0) { s_sel[0] = 0u; s_sel[1] = (unsigned)k; }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = s_sel[0], need = s_sel[1];
        const unsigned himask = (pass == 0) ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < n; i += 1024) {
            const unsigned key = adc_order_key(row[i]);
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFFu], 1u);
        }
        __syncthreads();
        adc_pick_bin(hist, need, prefix, shift, s_scan, &s_sel[0], &s_sel[1]);
    }
    const unsigned kth = s_sel[0];
    if (tid == 0) {
        const float t = adc_unorder_key(kth);
        thr[qi] = t;
        if (tint) tint[qi] = adc_tint_from(t, adc_qstat_of(qstat, qi), M);
    }
}

__global__ void ivf_check_kernel(const unsigned* __restrict__ cand_count, const int* __restrict__ rows, int nq, int k,
                                 int* __restrict__ status, int* __restrict__ qstatus) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const int want = rows[qi] < k ? rows[qi] : k;
    if ((int)cand_count[qi] < want) {
        atomicOr(status, 1);
        if (qstatus) atomicOr(qstatus + qi, 1);
    }
}

namespace {
struct ivfl_ws {
    size_t sample, thr, tint, qstat, qbyte, idcnt, ids, cnt, cand, stream_cnt, counters_end, stream, stream_cap, total;
};
ivfl_ws ivfl_layout(int M, int nq, int64_t sstride) {
    ivfl_ws L;
    size_t o = 0;
    L.sample = o; o += rc_align_up((size_t)nq * (size_t)sstride * sizeof(float), 256);
    L.thr = o;    o += rc_align_up((size_t)nq * sizeof(float), 256);
    L.tint = o;   o += rc_align_up((size_t)nq * sizeof(int), 256);
    L.qstat = o;  o += rc_align_up((size_t)nq * ADC_QSTAT_STRIDE * sizeof(float), 256);
    L.qbyte = o;  o += rc_align_up((size_t)nq * M * RC_K, 256);                 // compact per-query byte tables
    // the three counter arrays sit side by side: ONE memset clears them (idcnt | cnt | stream_cnt)
    L.idcnt = o;  o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
    L.cnt = o;    o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
    L.stream_cnt = o; o += rc_align_up((size_t)IVFS_MAX_BLOCKS * IVFS_WAVES * sizeof(unsigned), 256);
    L.counters_end = o;
    L.ids = o;    o += rc_align_up((size_t)nq * ADC_ID_CAP * sizeof(unsigned), 256);
    L.cand = o;   o += rc_align_up((size_t)nq * ADC_CAND_CAP * sizeof(unsigned long long), 256);
    // (query, row) streams of the pipelined screen: one per wave of its <= IVFS_MAX_BLOCKS persistent blocks
    size_t cap = (size_t)nq * (ADC_ID_CAP / 2) / (IVFS_MAX_BLOCKS * IVFS_WAVES);
    if (cap < 4096) cap = 4096;
    if (const char* e = getenv("RC_IVF_STREAM_CAP")) {      // tests: provoke the overflow path (status bit 2 -> less slack -> scan)
        const long v = atol(e);
        if (v > 0) cap = (size_t)v;
    }
    L.stream_cap = cap;
    L.stream = o;     o += rc_align_up((size_t)IVFS_MAX_BLOCKS * IVFS_WAVES * cap * 8, 256);
    L.total = o;
    return L;
}

// what a search hands to ivfl_launch<M>: the index, the queries' tables, the plan (by the host or by ivf_plan_*), the outputs
struct ivfl_args {
    rc_handle_t h;
    const uint8_t* codes; const uint8_t* image; const int64_t* list_off; const int64_t* rowmap;
    const float* lut; int nq;
    const int* probes; const int* sbase; const int* scount; const int* rows; const int* rank;
    int nprobe; int64_t sstride; int ss;
    adc_ivf_tasks T; int ntasks;          // ntasks: the length of the task arrays when T.ntasks holds the count on the device
    int k; float* scores; int64_t* out_ids; int* status; int* qstatus;      // qstatus may be NULL
    char* w; ivfl_ws L; hipStream_t s;
    int width;                            // 8 | 16: the screen; `image` and the tasks are the ones of that width
};
template <int M>
int ivfl_launch(const ivfl_args& a) {
    float* sample = (float*)(a.w + a.L.sample);
    float* thr = (float*)(a.w + a.L.thr);
    int* tint = (int*)(a.w + a.L.tint);
    float* qstat = (float*)(a.w + a.L.qstat);
    uint8_t* qbyte = (uint8_t*)(a.w + a.L.qbyte);
    unsigned* idcnt = (unsigned*)(a.w + a.L.idcnt);
    unsigned* ids = (unsigned*)(a.w + a.L.ids);
    unsigned* cnt = (unsigned*)(a.w + a.L.cnt);
    unsigned long long* cand = (unsigned long long*)(a.w + a.L.cand);
    {
        auto kern = ivf_sample_scan_kernel<M>;
        const size_t lds = (size_t)M * RC_K * sizeof(float) + (a.nprobe <= IVF_SAMPLE_PLAN_MAX ? (size_t)a.nprobe * 12 : 0);
        RC_HIP_CHECK(a.h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)((size_t)M * RC_K * sizeof(float) + IVF_SAMPLE_PLAN_MAX * 12)));
        // every block stages the query's 4 M 256-byte fp32 table: one slice per query unless the grid would not fill the chip
        int64_t slices = (a.sstride + 2047) / 2048;
        const int64_t fill = (2 * (int64_t)(a.h->num_cus > 0 ? a.h->num_cus : 256) + a.nq - 1) / a.nq;
        if (slices > fill) slices = fill;
        if (slices > 16) slices = 16;
        hipLaunchKernelGGL(kern, dim3((unsigned)a.nq, (unsigned)(slices < 1 ? 1 : slices)), dim3(IVF_SAMPLE_THREADS), lds, a.s,
                           a.codes, a.list_off, a.lut, a.probes, a.sbase, a.scount, a.nprobe, a.sstride, a.ss, sample);
        RC_LAUNCH_CHECK(a.h);
    }
    // tables first (they need no threshold), then tau and the integer threshold in one kernel
    hipLaunchKernelGGL(ivfs_qprep_kernel, dim3((unsigned)a.nq), dim3(RC_K, (M + 31) / 32), 0, a.s, a.lut, M, qstat, qbyte);
    RC_LAUNCH_CHECK(a.h);
    hipLaunchKernelGGL(ivf_rank_select_kernel, dim3((unsigned)a.nq), dim3(1024), 0, a.s, (const float*)sample, a.scount, a.rank,
                       a.sstride, thr, (const float*)qstat, M, tint);
    RC_LAUNCH_CHECK(a.h);
    RC_HIP_CHECK(a.h, hipMemsetAsync(a.w + a.L.idcnt, 0, a.L.counters_end - a.L.idcnt, a.s));      // idcnt, cnt, stream_cnt
    {
        // four loader waves (DESIGN_HISTORY 7: without them 1.04 vs 0.95 ms at nprobe 128); width 16: the 16-query screen
        // (ivfs_screen16.h; `image` is then the rows16 image and the tasks hold up to 16 queries)
        auto kern = a.width == 16 ? ivfs_screen16_kernel<M, 4> : ivfs_screen_kernel<M, 4>;
        constexpr int sl = 2 * IVFS_BUF;
        RC_HIP_CHECK(a.h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, sl));
        adc_ivf_tasks TT = a.T;
        TT.qbyte = qbyte;
        int blocks = a.h->num_cus > 0 ? a.h->num_cus : 256;       // persistent: one block per CU
        if (blocks > IVFS_MAX_BLOCKS) blocks = IVFS_MAX_BLOCKS;
        if (!a.T.ntasks && a.ntasks < blocks) blocks = a.ntasks;
        unsigned* stream_cnt = (unsigned*)(a.w + a.L.stream_cnt);
        unsigned* stream = (unsigned*)(a.w + a.L.stream);
        rc_prof_mark(a.h, RC_PROF_ADC_SCAN, a.s);
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(IVFS_THREADS), sl, a.s, a.image, (const int*)tint, stream_cnt, stream,
                           (unsigned)a.L.stream_cap, a.status, TT, a.ntasks);
        rc_prof_mark(a.h, RC_PROF_ADC_SCAN, a.s);
        RC_LAUNCH_CHECK(a.h);
        {
            const size_t bl = (size_t)a.nq * sizeof(unsigned);
            RC_HIP_CHECK(a.h, hipFuncSetAttribute((const void*)ivfs_bucket_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bl));
            hipLaunchKernelGGL(ivfs_bucket_kernel, dim3((unsigned)blocks), dim3(IVFS_BUCKET_THREADS), bl, a.s, (const unsigned*)stream_cnt,
                               (const unsigned*)stream, (unsigned)a.L.stream_cap, a.nq, idcnt, ids);
        }
        RC_LAUNCH_CHECK(a.h);
    }
    {
        auto krescore = adc_rescore_kernel<M>;
        const size_t rl = (size_t)M * RC_K * sizeof(float);
        RC_HIP_CHECK(a.h, hipFuncSetAttribute((const void*)krescore, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rl));
        hipLaunchKernelGGL(krescore, dim3((unsigned)a.nq), dim3(adc_rescore_threads(M)), rl, a.s, a.codes, a.lut, (const float*)thr,
                           (const unsigned*)idcnt, (const unsigned*)ids, cnt, cand, a.status, a.rowmap, a.qstatus);
        RC_LAUNCH_CHECK(a.h);
    }
    hipLaunchKernelGGL(ivf_check_kernel, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, a.s, (const unsigned*)cnt, a.rows, a.nq,
                       a.k, a.status, a.qstatus);
    RC_LAUNCH_CHECK(a.h);
    if (rc_env_set("RC_IVF_DEBUG")) {                          // development: list lengths of this search (synchronises)
        std::vector<unsigned> va(a.nq), vb(a.nq);
        (void)hipStreamSynchronize(a.s);
        (void)hipMemcpy(va.data(), idcnt, a.nq * sizeof(unsigned), hipMemcpyDeviceToHost);
        (void)hipMemcpy(vb.data(), cnt, a.nq * sizeof(unsigned), hipMemcpyDeviceToHost);
        double sa = 0, sb = 0; unsigned ma = 0, mb = 0;
        for (int i = 0; i < a.nq; ++i) { sa += va[i]; sb += vb[i]; ma = va[i] > ma ? va[i] : ma; mb = vb[i] > mb ? vb[i] : mb; }
        fprintf(stderr, "[ivf debug] nq %d nprobe %d ss %d sstride %lld: screened ids mean %.0f max %u, candidates mean %.0f max %u\n",
                a.nq, a.nprobe, a.ss, (long long)a.sstride, sa / a.nq, ma, sb / a.nq, mb);
    }
    // N = 0: fewer than k rows is legitimate (small cells); too FEW CANDIDATES is what ivf_check_kernel reports
    return rc_adc_launch_select(a.h, cand, cnt, a.nq, 0, a.k, 0, a.scores, a.out_ids, a.status, a.s, a.qstatus);
}
int ivfl_dispatch(int M, const ivfl_args& a) {
    switch (M) {
#define IVFL_WIDTH(MM) case MM: return ivfl_launch<MM>(a);
        ADC_CF_WIDTHS(IVFL_WIDTH)
#undef IVFL_WIDTH
        default: return RC_ESHAPE;
    }
}
}  // namespace

extern "C" size_t rc_ivf_search_lists_ws_bytes(int M, int nq, int64_t sstride) {
    if (!adc_cf_supported(M) || nq <= 0 || sstride <= 0) return 0;
    return ivfl_layout(M, nq, sstride).total;
}

// codes / image: [N,M] cell-major canonical codes and their permuted image; list_off [nlist+1]; rowmap [N] corpus position
// of every row; lut [nq,M,256] (rc_adc_lut); probes / sbase [nq,nprobe]: probed cells and the position of each probe's
// first SAMPLED row in the query's sample array (a cell of n rows is sampled in runs of 16 rows every 16 ss rows:
// 16 floor(n / (16 ss)) + min(16, n mod (16 ss)) entries);
// scount [nq] sampled rows, rows [nq] probed rows, rank [nq] rank of the sample score used as threshold (0: keep all);
// tasks: task_list / task_qstart / task_qcnt [ntasks] and sorted_q (query ids ordered by probed cell).
extern "C" int rc_ivf_search_lists(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                                   const int64_t* rowmap, int64_t N, int M, int K, const float* lut, int nq,
                                   const int* probes, const int* sbase, const int* scount, const int* rows, const int* rank,
                                   int nprobe, int64_t sstride, int ss, const int* task_list, const int* task_qstart,
                                   const int* task_qcnt, const int* sorted_q, int ntasks, int k, float* scores,
                                   int64_t* out_ids, int* status, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !codes || !image || !list_off || !rowmap || !lut || !probes || !sbase || !scount || !rows || !rank ||
        !task_list || !task_qstart || !task_qcnt || !sorted_q || !scores || !out_ids || !status || N <= 0 || nq < 0 ||
        nprobe <= 0 || sstride <= 0 || ss <= 0 || ntasks < 0 || k <= 0)
        return RC_EINVAL;
    if (K != RC_K || !adc_cf_supported(M) || k > ADC_CAND_CAP / 2 || N > 0xFFFFFFFFll || nq > 32768) return RC_ESHAPE;
    if (nq == 0) return RC_OK;
    const ivfl_ws L = ivfl_layout(M, nq, sstride);
    if (!ws || ws_bytes < L.total) return RC_EWORKSPACE;
    adc_ivf_tasks T = {task_list, task_qstart, task_qcnt, sorted_q, list_off, nullptr, nullptr};
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    if (ntasks == 0) {                                        // nothing probed: empty results through the select kernel
        RC_HIP_CHECK(h, hipMemsetAsync(w + L.cnt, 0, (size_t)nq * sizeof(unsigned), s));
        return rc_adc_launch_select(h, (unsigned long long*)(w + L.cand), (const unsigned*)(w + L.cnt), nq, 0, k, 0, scores,
                                    out_ids, status, s);
    }
    return ivfl_dispatch(M, ivfl_args{h, codes, image, list_off, rowmap, lut, nq, probes, sbase, scount, rows, rank, nprobe, sstride,
                                      ss, T, ntasks, k, scores, out_ids, status, nullptr, w, L, s, 8});
}

// ------------------------------------------------------------------------------------ device-side plan of the search
// rc_ivf_search_probes: everything rc_ivf_search_lists expects from its caller (sample layout, ranks, the task list) is
// derived on the device from the probes alone - four small kernels instead of ~40 framework launches and two host
// synchronisations (task count, sample stride) per search.
namespace {
struct ivfp_ws {
    size_t sbase, scount, rows, rank, per_cell, cell_start, first_task, cursor, ntasks, sorted_q, task_list, task_qstart,
        task_qcnt, total;
    int64_t ub;
};
ivfp_ws ivfp_layout(size_t base, int nq, int nprobe, int nlist) {
    ivfp_ws P;
    const size_t pairs = (size_t)nq * nprobe;
    const size_t ub = ivf_plan_task_bound(nq, nprobe, nlist, 8);      // sized for the 8-query tasks: the 16-query form has fewer
    P.ub = (int64_t)ub;
    size_t o = base;
    auto take = [&](size_t n) { const size_t at = o; o += rc_align_up(n * sizeof(int), 256); return at; };
    P.sbase = take(pairs); P.scount = take(nq); P.rows = take(nq); P.rank = take(nq);
    P.per_cell = take(nlist); P.cursor = take(nlist);         // adjacent: one memset clears both
    P.cell_start = take(nlist); P.first_task = take(nlist); P.ntasks = take(1);
    P.sorted_q = take(pairs); P.task_list = take(ub); P.task_qstart = take(ub); P.task_qcnt = take(ub);
    P.total = o;
    return P;
}
}  // namespace

// (ivfp_block_scan256 and the cell / scatter / task kernels of the plan: ivf_plan.h, shared with ivf_flat.hip)
// One block per query: sample layout of its probes, totals, threshold rank; counts the queries probing every cell.
__global__ __launch_bounds__(256) void ivf_plan_query_kernel(const int64_t* __restrict__ list_off, const int* __restrict__ probes,
                                                             int nprobe, int ss, int k, double slack, int keep_all_rows,
                                                             int* __restrict__ sbase, int* __restrict__ scount,
                                                             int* __restrict__ rows, int* __restrict__ rank,
                                                             int* __restrict__ per_cell) {
    __shared__ int s_wave[4];
    __shared__ long long s_rows[4];
    const int qi = blockIdx.x, tid = threadIdx.x;
    int carry = 0;
    long long rsum = 0;
    for (int b0 = 0; b0 < nprobe; b0 += 256) {                // block-uniform
        const int p = b0 + tid;
        int ssz = 0;
        long long size = 0;
        if (p < nprobe) {
            const int c = probes[(size_t)qi * nprobe + p];
            size = list_off[c + 1] - list_off[c];
            const long long run = 16ll * ss, rem = size % run;
            ssz = (int)(16ll * (size / run) + (rem < 16 ? rem : 16));
            atomicAdd(per_cell + c, 1);
        }
        int total;
        const int ex = ivfp_block_scan256(ssz, s_wave, total);
        if (p < nprobe) sbase[(size_t)qi * nprobe + p] = carry + ex;
        carry += total;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) size += __shfl_xor(size, o);
        if ((tid & 63) == 0) s_rows[tid >> 6] = size;             // per-wave totals of the row counts
        __syncthreads();
        rsum += s_rows[0] + s_rows[1] + s_rows[2] + s_rows[3];
        __syncthreads();
    }
    if (tid == 0) {
        const long long r = rsum > 0x7FFFFFFFll ? 0x7FFFFFFFll : rsum;
        scount[qi] = carry;
        rows[qi] = (int)r;
        // rank of the sample score used as threshold: mu = expected number of the k best among the sampled rows; queries
        // whose probed rows fit the candidate list comfortably keep every row (rank 0 -> threshold -inf)
        const double den = (double)(r > 0 ? r : 1);
        const double mu = (double)k * (double)carry / den;
        double rk = floor(mu + slack * sqrt(mu + 1.0) + 4.0) + 1.0;
        const double cap = floor(0.8 * (double)ADC_CAND_CAP * (double)carry / den);
        if (rk > cap && cap >= mu + 2.5 * sqrt(mu + 1.0) + 2.0) rk = cap;
        if (rk > (double)carry) rk = (double)carry;
        if (rk < 0.0) rk = 0.0;
        rank[qi] = (r <= keep_all_rows) ? 0 : (int)rk;
    }
}

// Probe selection: the nprobe cells with the largest coarse score of every query (ties at the boundary: lower cell id),
// written in ascending cell order — the search needs the SET of probed cells, not their ranking.  One block per query: the
// nlist scores as order-preserving keys in LDS, 4-pass radix select of the nprobe-th largest key, ordered compaction.
// (The framework's topk + sort + gather + argsort chain cost 0.15 ms per 1200 queries, a tenth of a search at nprobe 32.)
__global__ __launch_bounds__(1024) void ivf_probe_select_kernel(const float* __restrict__ scores, int nlist, int nprobe,
                                                                int* __restrict__ probes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem);  // [nlist]
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_rank;
    __shared__ unsigned s_scan[4];
    __shared__ int s_gt[16], s_eq[16];
    const int qi = blockIdx.x, tid = threadIdx.x;
    // + 0.0f turns -0.0 into +0.0 (and changes no other number): the two zeros tie, as they do for every comparison of the
    // scores themselves, and the lower cell wins.  adc_order_key alone orders the raw bits, -0.0 below +0.0.
    for (int i = tid; i < nlist; i += 1024) keys[i] = adc_order_key(scores[(size_t)qi * nlist + i] + 0.0f);
    if (tid == 0) { sel_prefix = 0u; sel_rank = (unsigned)nprobe; }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = sel_prefix;
        const unsigned himask = (pass == 0) ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < nlist; i += 1024) {
            const unsigned k = keys[i];
            if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 0xFFu], 1u);
        }
        __syncthreads();
        adc_pick_bin(hist, sel_rank, prefix, shift, s_scan, &sel_prefix, &sel_rank);
    }
    const unsigned T = sel_prefix;
    const int need = (int)sel_rank;                        // how many of the cells tied at T belong to the selection
    const int chunk = (nlist + 1023) / 1024;
    const int c0 = tid * chunk, c1 = (c0 + chunk < nlist) ? c0 + chunk : nlist;
    int gt = 0, eq = 0;
    for (int c = c0; c < c1; ++c) {
        const unsigned k = keys[c];
        gt += (k > T) ? 1 : 0;
        eq += (k == T) ? 1 : 0;
    }
    // exclusive prefix sums of (gt, eq) over the 1024 threads
    const int lane = tid & 63, wv = tid >> 6;
    int igt = gt, ieq = eq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(igt, o), b = __shfl_up(ieq, o);
        if (lane >= o) { igt += a; ieq += b; }
    }
    if (lane == 63) { s_gt[wv] = igt; s_eq[wv] = ieq; }
    __syncthreads();
    int bgt = 0, beq = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        bgt += (j < wv) ? s_gt[j] : 0;
        beq += (j < wv) ? s_eq[j] : 0;
    }
    const int gt_before = bgt + igt - gt;
    int eq_seen = beq + ieq - eq;
    int pos = gt_before + (eq_seen < need ? eq_seen : need);
    int* out = probes + (size_t)qi * nprobe;
    for (int c = c0; c < c1; ++c) {
        const unsigned k = keys[c];
        if (k > T) {
            out[pos++] = c;
        } else if (k == T) {
            if (eq_seen < need) out[pos++] = c;
            ++eq_seen;
        }
    }
}

// scores: [nq, nlist] fp32 coarse scores (larger = closer); probes: [nq, nprobe] int32, ascending cell ids.
extern "C" int rc_ivf_select_probes(rc_handle_t h, const float* scores, int nq, int nlist, int nprobe, int* probes,
                                    rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !scores || !probes || nq < 0 || nlist <= 0 || nprobe <= 0 || nprobe > nlist) return RC_EINVAL;
    if (nlist > 16384) return RC_ESHAPE;                    // the keys of a query live in 64 KiB of LDS
    if (nq == 0) return RC_OK;
    const size_t lds = (size_t)nlist * sizeof(unsigned);
    RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)ivf_probe_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ivf_probe_select_kernel, dim3((unsigned)nq), dim3(1024), lds, (hipStream_t)stream, scores, nlist, nprobe,
                       probes);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

extern "C" size_t rc_ivf_search_probes_ws_bytes(int M, int nq, int nprobe, int nlist, int64_t sstride) {
    if (!adc_cf_supported(M) || nq <= 0 || nprobe <= 0 || nlist <= 0 || sstride <= 0) return 0;
    return ivfp_layout(ivfl_layout(M, nq, sstride).total, nq, nprobe, nlist).total;
}

// rc_ivf_search_lists with the plan made on the device.  probes [nq, nprobe]: distinct cells per query; sstride: capacity of
// a query's sample array, >= the largest possible number of sampled rows of nprobe cells (a cell of n rows contributes
// 16 floor(n / 16 ss) + min(16, n mod 16 ss)); sel_slack: standard deviations of head-room in the threshold rank;
// keep_all_rows: queries probing no more rows than this re-score every row.  Same status bits, same results.
extern "C" int rc_ivf_search_probes(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                                    const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                                    const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                                    int keep_all_rows, float* scores, int64_t* out_ids, int* status, void* ws,
                                    size_t ws_bytes, rc_stream_t stream) {
    return rc_ivf_search_probes_q(h, codes, image, list_off, rowmap, N, nlist, M, K, lut, nq, probes, nprobe, sstride, ss, k,
                                  sel_slack, keep_all_rows, scores, out_ids, status, nullptr, ws, ws_bytes, stream);
}
// ... with per-query status words (qstatus [nq] int32, zeroed by the caller; may be NULL): bit 0 = the query kept fewer than
// min(k, rows probed) candidates, bit 1 = its id list overflowed.  The other queries' results stand: a caller answers only
// the flagged ones again (IVFPQIndex.search: by the per-query exact scan).  A survivor STREAM that filled up (status bit 2)
// is not attributable to a query and may have dropped anybody's rows: repeat the call with less slack.
static int ivf_search_probes_w(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                               const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                               const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                               int keep_all_rows, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws,
                               size_t ws_bytes, rc_stream_t stream, int width) {
    rc_device_guard device_guard_(h);
    if (!h || !codes || !image || !list_off || !rowmap || !lut || !probes || !scores || !out_ids || !status || N <= 0 ||
        nq < 0 || nprobe <= 0 || nlist <= 0 || nprobe > nlist || sstride <= 0 || ss <= 0 || k <= 0)
        return RC_EINVAL;
    if (K != RC_K || !adc_cf_supported(M) || k > ADC_CAND_CAP / 2 || N > 0xFFFFFFFFll || nq > 32768) return RC_ESHAPE;
    if (nq == 0) return RC_OK;
    const ivfl_ws L = ivfl_layout(M, nq, sstride);
    const ivfp_ws P = ivfp_layout(L.total, nq, nprobe, nlist);
    if (!ws || ws_bytes < P.total) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    auto I = [&](size_t off) { return (int*)(w + off); };
    const int64_t pairs = (int64_t)nq * nprobe;
    RC_HIP_CHECK(h, hipMemsetAsync(w + P.per_cell, 0, P.cell_start - P.per_cell, s));      // per_cell and cursor
    hipLaunchKernelGGL(ivf_plan_query_kernel, dim3((unsigned)nq), dim3(256), 0, s, list_off, probes, nprobe, ss, k, sel_slack,
                       keep_all_rows, I(P.sbase), I(P.scount), I(P.rows), I(P.rank), I(P.per_cell));
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(ivf_plan_cells_kernel, dim3(1), dim3(256), 0, s, (const int*)I(P.per_cell), nlist, I(P.cell_start),
                       I(P.first_task), I(P.ntasks), width);
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(ivf_plan_scatter_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, probes, pairs, nprobe, nlist,
                       (const int*)I(P.cell_start), I(P.cursor), I(P.sorted_q));
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(ivf_plan_tasks_kernel, dim3((unsigned)((P.ub + 255) / 256)), dim3(256), 0, s, (const int*)I(P.per_cell),
                       (const int*)I(P.cell_start), (const int*)I(P.first_task), (const int*)I(P.ntasks), nlist, P.ub,
                       I(P.task_list), I(P.task_qstart), I(P.task_qcnt), width);
    RC_LAUNCH_CHECK(h);
    adc_ivf_tasks T = {I(P.task_list), I(P.task_qstart), I(P.task_qcnt), I(P.sorted_q), list_off, nullptr, I(P.ntasks)};
    return ivfl_dispatch(M, ivfl_args{h, codes, image, list_off, rowmap, lut, nq, probes, I(P.sbase), I(P.scount), I(P.rows),
                                      I(P.rank), nprobe, sstride, ss, T, (int)P.ub, k, scores, out_ids, status, qstatus, w, L, s,
                                      width});
}
extern "C" int rc_ivf_search_probes_q(rc_handle_t h, const uint8_t* codes, const uint8_t* image, const int64_t* list_off,
                                      const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                                      const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                                      int keep_all_rows, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws,
                                      size_t ws_bytes, rc_stream_t stream) {
    return ivf_search_probes_w(h, codes, image, list_off, rowmap, N, nlist, M, K, lut, nq, probes, nprobe, sstride, ss, k, sel_slack,
                               keep_all_rows, scores, out_ids, status, qstatus, ws, ws_bytes, stream, 8);
}
// The same search on the 16-QUERY screen (round 6, ivfs_screen16.h): tasks of up to 16 queries per probed cell, one
// ds_read_b128 gather per (16 rows, 4 sub-quantisers, 16 queries).  `image16`: rc_adc_scan_image_rows16 of the cell-major codes
// (rc_adc_scan_image_rows16_bytes(N, M) bytes).  Same workspace, status bits and RESULTS as rc_ivf_search_probes_q; pays when a
// probed cell is shared by more than ~8 queries of the call (nq x nprobe / nlist; IVFPQIndex.search decides).
extern "C" int rc_ivf_search_probes_q16(rc_handle_t h, const uint8_t* codes, const uint8_t* image16, const int64_t* list_off,
                                        const int64_t* rowmap, int64_t N, int nlist, int M, int K, const float* lut, int nq,
                                        const int* probes, int nprobe, int64_t sstride, int ss, int k, double sel_slack,
                                        int keep_all_rows, float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws,
                                        size_t ws_bytes, rc_stream_t stream) {
    return ivf_search_probes_w(h, codes, image16, list_off, rowmap, N, nlist, M, K, lut, nq, probes, nprobe, sstride, ss, k,
                               sel_slack, keep_all_rows, scores, out_ids, status, qstatus, ws, ws_bytes, stream, 16);
}
