// The top-k selection stage shared by the flat ADC search (adc_search.hip), the IVF searches (ivf_search.hip, ivf_lists.hip)
// and the exact dense search (dense_search.hip): the limits that producers of candidate keys and the select agree on, the
// order-preserving score key and the k-th-largest selection (device functions: every translation unit compiles its own
// copy, no -fgpu-rdc), and the host interface of topk.hip, where the contract is written down.
#pragma once
#include "rc_common.h"

#define ADC_SAMPLE_MAX 32768         // sample scores per query (adc_threshold_kernel keeps them as keys in LDS)
#define ADC_KTH_LIST 4096            // members of the selected value bin kept in LDS by adc_kth_largest_v
#define ADC_CAND_CAP 16384           // 64-bit keys per query's candidate list: cand[nq][ADC_CAND_CAP]

__device__ __forceinline__ unsigned adc_order_key(float s) {
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float adc_unorder_key(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// One step of the 8-bit radix select: from the 256-bin histogram of the keys that match `prefix`, the bin that holds the
// need-th largest key, i.e. the largest b with sum_{j >= b} hist[j] >= need — computed by 256 threads with a wave scan.
// (One thread walking down from bin 255 is a chain of dependent LDS reads: ~10 us per pass, 40 of the 46 us a threshold
// block took.)  Called by every thread of a block of >= 256 threads; `need` must have been read before; ends in a barrier.
__device__ __forceinline__ void adc_pick_bin(const unsigned* hist, unsigned need, unsigned prefix, int shift, unsigned* s_scan,
                                             unsigned* sel_prefix, unsigned* sel_rank) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned v = 0u, incl = 0u;
    if (tid < 256) {
        v = hist[255 - tid];                                  // thread t owns bin 255 - t: prefix over t = suffix over bins
        incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = (unsigned)__shfl_up((int)incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_scan[wv] = incl;
    }
    __syncthreads();
    if (tid < 256) {
#pragma unroll
        for (int w = 0; w < 3; ++w) incl += (w < wv) ? s_scan[w] : 0u;
        const unsigned excl = incl - v;
        if (incl >= need && excl < need) {
            *sel_prefix = prefix | ((unsigned)(255 - tid) << shift);
            *sel_rank = need - excl;
        } else if (tid == 255 && incl < need) {               // fewer matching keys than asked for: what the walk did
            *sel_prefix = prefix;
            *sel_rank = need - incl;
        }
    }
    __syncthreads();
}

// rank-th largest of n 32-bit keys (key_at(i), i < n; rank in [1, n]) by radix select, 8 bits per pass — but only over the
// bits in which the keys DIFFER: a block min / max first, the common leading bits are the result's.  Scores of one query's
// candidates share their sign / exponent byte (often the next one too): a pass over such a byte sends every key to ONE
// histogram bin, i.e. n LDS atomics on one address, one after the other (round 3: two of the four passes of the 32 768-key
// threshold kernel, ~100 of its 130 us per 1200 queries).  Called by every thread of a block of >= 256 threads; `hist`
// [256], `s_scan` [4], `s_sel` [2], `s_mm` [2] in LDS.
template <typename KeyAt>
__device__ __forceinline__ unsigned adc_kth_largest(KeyAt key_at, int64_t n, unsigned rank, unsigned* hist, unsigned* s_scan,
                                                    unsigned* s_sel, unsigned* s_mm) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) { s_mm[0] = 0xFFFFFFFFu; s_mm[1] = 0u; }
    __syncthreads();
    unsigned mn = 0xFFFFFFFFu, mx = 0u;
    for (int64_t i = tid; i < n; i += nthr) {
        const unsigned k = key_at(i);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = (unsigned)__shfl_xor((int)mn, o), b = (unsigned)__shfl_xor((int)mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((tid & 63) == 0) { atomicMin(&s_mm[0], mn); atomicMax(&s_mm[1], mx); }
    __syncthreads();
    const unsigned lo = s_mm[0], hi_key = s_mm[1];
    if (lo == hi_key) return hi_key;                          // all keys equal (block-uniform)
    const int top = 31 - __clz((int)(lo ^ hi_key));          // highest bit in which two keys differ
    int undecided = top + 1;                                  // bits [0, undecided)
    if (tid == 0) { s_sel[0] = hi_key & ~((2u << top) - 1u); s_sel[1] = rank; }
    __syncthreads();
    while (undecided > 0) {
        const int width = undecided < 8 ? undecided : 8, shift = undecided - width;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = s_sel[0], need = s_sel[1];
        const unsigned himask = undecided >= 32 ? 0u : (0xFFFFFFFFu << undecided), dmask = (1u << width) - 1u;
        for (int64_t i = tid; i < n; i += nthr) {
            const unsigned k = key_at(i);
            if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & dmask], 1u);
        }
        __syncthreads();
        adc_pick_bin(hist, need, prefix, shift, s_scan, &s_sel[0], &s_sel[1]);
        undecided = shift;
    }
    return s_sel[0];
}

// The same answer, faster on real score distributions: bit-radix passes see a float's sign / exponent structure — a
// near-Gaussian sample puts half of its keys into one or two bins of the first pass whatever window of bits it uses
// (measured: skipping the common leading bits alone made the kernels SLOWER, the min / max pass cost more than it saved).
// So the first cut is made in VALUE space: 256 equal bins over [min, max] of the scores (a monotone function of the key:
// bin(s) = min(255, int((s - smin) scale)), so "the bin that holds the rank-th largest" is well defined) — the fullest bin of
// a Gaussian sample holds ~1.3 % of it — then the members of that one bin (a few dozen in the tail where the thresholds
// live) are collected into `list` and the bit-radix select above runs on them.  Non-finite extremes, a degenerate range
// (256 / (smax - smin) inf or 0: a sub-normal or an overflowing range) or a bin longer than list_cap: the plain bit-radix
// select over everything.  `s_aux`: 8 words of LDS.
// MM_READY: the caller has already reduced the keys' minimum / maximum into s_aux[2] / s_aux[3] (e.g. while loading them),
// zeroed hist and s_aux[4], and synchronised.
template <bool MM_READY = false, typename KeyAt>
__device__ __forceinline__ unsigned adc_kth_largest_v(KeyAt key_at, int64_t n, unsigned rank, unsigned* hist, unsigned* s_scan,
                                                      unsigned* s_aux, unsigned* list, int list_cap) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    unsigned* s_sel = s_aux, *s_mm = s_aux + 2, *s_cnt = s_aux + 4;
    if constexpr (!MM_READY) {
        if (tid == 0) { s_mm[0] = 0xFFFFFFFFu; s_mm[1] = 0u; *s_cnt = 0u; }
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        unsigned mn = 0xFFFFFFFFu, mx = 0u;
        for (int64_t i = tid; i < n; i += nthr) {
            const unsigned k = key_at(i);
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned a = (unsigned)__shfl_xor((int)mn, o), b = (unsigned)__shfl_xor((int)mx, o);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((tid & 63) == 0) { atomicMin(&s_mm[0], mn); atomicMax(&s_mm[1], mx); }
        __syncthreads();
    }
    const unsigned lo = s_mm[0], hi_key = s_mm[1];
    if (lo == hi_key) return hi_key;
    const float smin = adc_unorder_key(lo), smax = adc_unorder_key(hi_key);
    const float scale = 256.0f / (smax - smin);
    // all finite (block-uniform); scale == 0: smax - smin overflowed, s - smin can be inf and inf * 0 has no bin
    const bool linear = (smin - smin == 0.f) && (smax - smax == 0.f) && (scale - scale == 0.f) && scale > 0.f;
    if (!linear) {
        __syncthreads();
        return adc_kth_largest(key_at, n, rank, hist, s_scan, s_sel, s_mm);
    }
    auto bin_of = [&](unsigned k) {
        const int b = (int)((adc_unorder_key(k) - smin) * scale);
        return b > 255 ? 255 : b;
    };
    for (int64_t i = tid; i < n; i += nthr) atomicAdd(&hist[bin_of(key_at(i))], 1u);
    __syncthreads();
    adc_pick_bin(hist, rank, 0u, 0, s_scan, &s_sel[0], &s_sel[1]);    // s_sel[0] = bin, s_sel[1] = rank inside it (ends in a barrier)
    const int b = (int)s_sel[0];
    const unsigned inside = s_sel[1], members = hist[b];
    __syncthreads();
    if ((int)members > list_cap)
        return adc_kth_largest(key_at, n, rank, hist, s_scan, s_sel, s_mm);
    for (int64_t i = tid; i < n; i += nthr) {
        const unsigned k = key_at(i);
        if (bin_of(k) == b) list[atomicAdd(s_cnt, 1u)] = k;
    }
    __syncthreads();
    return adc_kth_largest([&](int64_t i) { return list[i]; }, (int64_t)members, inside, hist, s_scan, s_sel, s_mm);
}

// the 64-bit candidate key of row i (i < 2^32) with score s: ordered score << 32 | ~row
__device__ __forceinline__ unsigned long long adc_exact_key(float s, int64_t i) {
    return ((unsigned long long)adc_order_key(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

// Append by the lanes of a wave to a list whose length is `counter` (global or LDS): `mask` = __ballot of the lanes that have an
// entry (not 0; every lane of the wave calls, in a block of whole waves whose x index numbers the lanes).  The lowest set lane
// adds popcount(mask) with ONE atomic, the old length is broadcast, and a lane's slot is that base + its rank among the set
// lanes below it.  The capacity test and the store are the caller's.
__device__ __forceinline__ unsigned adc_wave_append(unsigned long long mask, unsigned* counter) {
    const int lane = threadIdx.x & 63, leader = (int)__builtin_ctzll(mask);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(mask));
    base = __shfl(base, leader);
    return base + rank;
}

// ---- host interface (topk.hip) ---------------------------------------------------------------------------------------
// rank of the sample score used as the candidate threshold (header text at rc_adc_search)
int rc_adc_sample_rank(int64_t N, int64_t S, int k, double sel_slack);
// threshold stage: thr[q] = r-th largest of sample[q][0..S)
int rc_adc_launch_threshold(rc_handle_t h, const float* sample, int64_t S, int nq, int r, float* thr, hipStream_t s);
// sort + emit stage: the k best of the cnt[q] keys of cand[q][ADC_CAND_CAP] -> scores / ids [nq][k]
int rc_adc_launch_select(rc_handle_t h, unsigned long long* cand, const unsigned* cnt, int nq, int64_t N, int k,
                         int64_t id_offset, float* scores, int64_t* ids, int* status, hipStream_t s, int* qstatus = nullptr);
// The select stage of the exact route for nx queries whose full score rows sc[nx][N] are written: the min(k, N) best
// 64-bit keys by the 8-pass radix select, compacted and sorted + emitted.
// hist [nx][256], prefix [nx], rank [nx], cnt [nx], cand [nx][ADC_CAND_CAP]; status: a device int.
int rc_adc_launch_exact_select(rc_handle_t h, const float* sc, int64_t N, int nx, int k, int64_t id_offset, unsigned* hist,
                               unsigned long long* prefix, unsigned* rank, unsigned* cnt, unsigned long long* cand,
                               int* status, float* scores, int64_t* ids, hipStream_t s);

// Workspace of rc_adc_launch_exact_select for rounds of up to qx queries: byte offsets of its six blocks, laid out after the
// caller's own `base` bytes (tables, score rows), every block aligned to 256 bytes; total = end of the last block.
struct topk_exact_layout { size_t hist, prefix, rank, cnt, cand, status, total; };
static inline topk_exact_layout topk_exact_ws(size_t base, int qx) {
    topk_exact_layout L;
    size_t o = base;
    L.hist = o;   o += rc_align_up((size_t)qx * 256 * sizeof(unsigned), 256);
    L.prefix = o; o += rc_align_up((size_t)qx * sizeof(unsigned long long), 256);
    L.rank = o;   o += rc_align_up((size_t)qx * sizeof(unsigned), 256);
    L.cnt = o;    o += rc_align_up((size_t)qx * sizeof(unsigned), 256);
    L.cand = o;   o += rc_align_up((size_t)qx * ADC_CAND_CAP * sizeof(unsigned long long), 256);
    L.status = o; o += 256;
    L.total = o;
    return L;
}
// rc_adc_launch_exact_select on the workspace `w` laid out that way (sc: the caller's score rows); the launcher itself keeps
// its six-pointer signature, it is a symbol of the shared library
static inline int topk_exact_select(rc_handle_t h, const float* sc, int64_t N, int nx, int k, int64_t id_offset, char* w,
                                    const topk_exact_layout& L, float* scores, int64_t* ids, hipStream_t s) {
    return rc_adc_launch_exact_select(h, sc, N, nx, k, id_offset, (unsigned*)(w + L.hist), (unsigned long long*)(w + L.prefix),
                                      (unsigned*)(w + L.rank), (unsigned*)(w + L.cnt), (unsigned long long*)(w + L.cand),
                                      (int*)(w + L.status), scores, ids, s);
}
