// The top-k selection stage of every search of the library: the flat ADC search (adc_search.hip), the IVF searches
// (ivf_search.hip, ivf_lists.hip) and the exact dense search (dense_search.hip) produce scores or candidate keys, the
// kernels here turn them into the k best (score, id) pairs per query.
//
// Contract between the producers and this stage (limits and device helpers: topk.h):
//   key        64 bits per candidate row: adc_order_key(score) << 32 | ~id (adc_exact_key), id < 2^32 the row's corpus
//              position.  adc_order_key maps fp32 scores to unsigned integers of the same order, so a DESCENDING sort of the
//              keys is (score descending, id ascending) — the tie rule of every search: equal scores, lower id first.
//              The order is TOTAL on the bit patterns, which "score descending" does not say: -0.0 sorts directly below
//              +0.0 (two different keys: a row scoring +0.0 precedes every row scoring -0.0 whatever their ids, and the
//              emitted score keeps its sign bit), +inf above and -inf below every finite score, a NaN with the sign bit
//              clear above +inf and one with it set below -inf.  Sub-normal scores are ordinary keys.  The dense producer
//              never emits -0.0 for a corpus whose rows hold no tiny values: its fmaf chain starts at +0.0 and x + (+0.0) is
//              never -0.0; only a product that underflows to zero from below leaves -0.0 in the chain, and it survives
//              only if every later term q[d] x[n][d] is -0.0 as well.
//   lists      cand[nq][ADC_CAND_CAP] keys and cnt[nq] (zeroed by the caller) per query.  A producer appends by an atomic add
//              on cnt[q] and stores only slots < ADC_CAND_CAP: cnt[q] may exceed the capacity, the list never does.
//   status     one device int per call, qstatus (optional) one per query, both OR-ed into, never cleared here:
//              bit 0 = fewer than min(k, N) candidates were collected (the threshold was too high: more slack),
//              bit 1 = a list overflowed, cnt[q] > ADC_CAND_CAP (too low: less slack).  k <= ADC_CAND_CAP / 2.
//   output     scores / ids [nq][k], best first; positions past the query's candidate count hold (-inf, -1).
//   environment  RC_ADC_SELECT_CAP = keys adc_select_kernel holds in LDS (a power of two >= 1024; tests: 1024 forces the cut
//              and the global-memory sort), read on every call like every RC_ADC_* switch.
//
// Fast routes:  sample scores -> adc_threshold_kernel (tau_q = the r-th largest, r = rc_adc_sample_rank) -> the producer's
//               filter pass appends the keys of the rows with score >= tau_q -> adc_select_kernel.
// Exact route:  full score rows -> adc_exact_{init,hist,pick,collect}_kernel (the min(k, N) largest KEYS by an 8-pass radix
//               select: no sample, no failure mode) -> adc_select_kernel.
#include "topk.h"

// ------------------------------------------------------------------------------------------ 3. threshold
// One block per query: r-th largest of S sample scores by an 8-bit-per-pass radix select on the
// order-preserving key, everything in LDS.  r <= 0 or r > S: tau = -inf (keep every row).
__global__ __launch_bounds__(1024) void adc_threshold_kernel(const float* __restrict__ sample, int64_t S, int r,
                                                             float* __restrict__ thr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem);  // [S]
    __shared__ unsigned hist[256];
    __shared__ unsigned s_aux[8];
    __shared__ unsigned s_scan[4];
    __shared__ unsigned s_list[ADC_KTH_LIST];
    const int qi = blockIdx.x, tid = threadIdx.x;
    if (r <= 0 || r > S) {
        if (tid == 0) thr[qi] = -INFINITY;
        return;
    }
    if (tid == 0) { s_aux[2] = 0xFFFFFFFFu; s_aux[3] = 0u; s_aux[4] = 0u; }
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    unsigned mn = 0xFFFFFFFFu, mx = 0u;                       // minimum / maximum on the way into the LDS
    for (int64_t i = tid; i < S; i += 1024) {
        const unsigned k = adc_order_key(sample[(size_t)qi * S + i]);
        keys[i] = k;
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = (unsigned)__shfl_xor((int)mn, o), b = (unsigned)__shfl_xor((int)mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((tid & 63) == 0) { atomicMin(&s_aux[2], mn); atomicMax(&s_aux[3], mx); }
    __syncthreads();
    const unsigned kth = adc_kth_largest_v<true>([&](int64_t i) { return keys[i]; }, S, (unsigned)r, hist, s_scan, s_aux, s_list,
                                                 ADC_KTH_LIST);
    if (tid == 0) thr[qi] = adc_unorder_key(kth);
}

// threshold stage: thr[q] = r-th largest of sample[q][0..S)
int rc_adc_launch_threshold(rc_handle_t h, const float* sample, int64_t S, int nq, int r, float* thr, hipStream_t s) {
    const size_t tl = (size_t)S * sizeof(unsigned);
    RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)adc_threshold_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)tl));
    hipLaunchKernelGGL(adc_threshold_kernel, dim3((unsigned)nq), dim3(1024), tl, s, sample, S, r, thr);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// rank of the sample score used as the candidate threshold (header text at rc_adc_search)
int rc_adc_sample_rank(int64_t N, int64_t S, int k, double sel_slack) {
    if (N <= ADC_CAND_CAP) return 0;   // tau = -inf: every row is a candidate, the select kernel sorts them all
    if (S == N) return k;              // the sample is the whole index: tau is the exact k-th score
    const double mu = (double)k * (double)S / (double)N;
    int r = (int)(mu + sel_slack * sqrt(mu + 1.0) + 4.0) + 1;
    // large k: keep the expected candidate count (r N / S) below ~80 % of the list capacity as long as that still
    // leaves 2.5 sigma of head-room over k
    const double r_cap = 0.8 * (double)ADC_CAND_CAP * (double)S / (double)N;
    if ((double)r > r_cap && r_cap >= mu + 2.5 * sqrt(mu + 1.0) + 2.0) r = (int)r_cap;
    if (r > S) r = (int)S;
    if (r < 1) r = 1;       // a (hugely) negative slack: the best sample score
    return r;
}

// ---- bitonic sort of P keys (descending) in LDS, register-blocked ----------------------------------------------------
// The plain network makes one LDS round trip (read 2, write 2 keys per pair) and one barrier per (size, stride) stage: 66
// stages for 2048 keys = 4.2 MB of LDS traffic per query — at four blocks per CU the LDS pipe, not latency, was the
// kernel's whole time (round 4 measurement: 138 us per 1200 queries with one block per CU, 150 us with four).  Here a
// work item takes the 2^NB keys that differ in NB consecutive index bits, runs the NB stages of those strides in
// registers and writes the keys back: ceil(c / 3) round trips for the c strides of a merge, and the merges of sizes 2, 4, 8
// in ONE pass: 24 round trips for 2048 keys.  Keys live at padded positions i + i / 32 so that the stride-1 / 2 / 4
// passes (a lane's keys 8, 16, 32 apart from its neighbour's) do not fall on the same banks.
__device__ __forceinline__ int adc_sp(int i) { return i + (i >> 5); }
__device__ __forceinline__ void adc_cmpx(unsigned long long& a, unsigned long long& b, bool desc) {
    const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
    a = desc ? hi : lo;
    b = desc ? lo : hi;
}
template <int NB>
__device__ __forceinline__ void adc_bitonic_pass(unsigned long long* keys, int P, int size, int L, int tid, int nthr) {
    constexpr int NK = 1 << NB;
    const int lsh = 31 - __clz(L);
    for (int t = tid; t < (P >> NB); t += nthr) {
        const int base = ((t >> lsh) << (lsh + NB)) | (t & (L - 1));
        const bool desc = (base & size) == 0;
        unsigned long long v[NK];
#pragma unroll
        for (int j = 0; j < NK; ++j) v[j] = keys[adc_sp(base + j * L)];
#pragma unroll
        for (int b = NB - 1; b >= 0; --b)
#pragma unroll
            for (int j = 0; j < NK; ++j)
                if (!(j & (1 << b))) adc_cmpx(v[j], v[j | (1 << b)], desc);
#pragma unroll
        for (int j = 0; j < NK; ++j) keys[adc_sp(base + j * L)] = v[j];
    }
    __syncthreads();
}
// keys[adc_sp(0 .. P)) sorted descending; P a power of two >= 8; called by every thread of the block, ends in a barrier
__device__ __forceinline__ void adc_bitonic_sort_lds(unsigned long long* keys, int P, int tid, int nthr) {
    // sizes 2, 4, 8 on 8 consecutive keys
    for (int t = tid; t < (P >> 3); t += nthr) {
        const int base = t << 3;
        unsigned long long v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = keys[adc_sp(base + j)];
#pragma unroll
        for (int sz = 2; sz <= 8; sz <<= 1)
#pragma unroll
            for (int st = sz >> 1; st > 0; st >>= 1)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (!(j & st)) adc_cmpx(v[j], v[j | st], ((base + j) & sz) == 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) keys[adc_sp(base + j)] = v[j];
    }
    __syncthreads();
    for (int size = 16; size <= P; size <<= 1) {
        int c = 31 - __clz(size);                             // strides size/2 .. 1: c of them, the first chunk takes c mod 3
        int s = size >> 1;
        while (c > 0) {
            const int nb = (c % 3) ? (c % 3) : 3;
            const int L = s >> (nb - 1);
            if (nb == 3) adc_bitonic_pass<3>(keys, P, size, L, tid, nthr);
            else if (nb == 2) adc_bitonic_pass<2>(keys, P, size, L, tid, nthr);
            else adc_bitonic_pass<1>(keys, P, size, L, tid, nthr);
            c -= nb;
            s = L >> 1;
        }
    }
}

// ------------------------------------------------------------------------------------------ 5. select
// One block per query.  Sort the candidate keys descending (bitonic, LDS), emit the first k.
// status |= 1 if fewer than min(k,N) candidates were collected, |= 2 if the list overflowed.
// Round 4: the block's LDS holds `cap` keys, cap = the power of two >= max(4096, 2 k) (host, adc_select_cap): lists longer
// than max(2048, 2 k) are first cut down to the k best scores (+ every tie at the k-th score) by a radix select over the
// list in global memory (L2), so what is sorted always fits — 32 KiB and 512 threads per block at k = 1000, four blocks
// per CU, where round 3 reserved 128 KiB (one 1024-thread block per CU: 27 us of barrier-to-barrier latency per query with
// nothing to overlap it; 138 -> 60 us per 1200 queries).  Only a tie group at the k-th score that does not fit takes the
// sort in global memory (same network, same result).
__global__ __launch_bounds__(1024) void adc_select_kernel(unsigned long long* __restrict__ cand,
                                                          const unsigned* __restrict__ cand_count, int64_t N, int k,
                                                          int64_t id_offset, float* __restrict__ scores,
                                                          int64_t* __restrict__ ids, int* __restrict__ status,
                                                          int* __restrict__ qstatus, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int qi = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const unsigned raw = cand_count[qi];
    const int cnt = raw > ADC_CAND_CAP ? ADC_CAND_CAP : (int)raw;
    unsigned long long* gk = cand + (size_t)qi * ADC_CAND_CAP;
    unsigned long long* lk = reinterpret_cast<unsigned long long*>(smem);
    const int64_t want = (k < N) ? k : N;
    if (tid == 0) {
        int st = 0;
        if ((int64_t)cnt < want) st |= 1;
        if (raw > ADC_CAND_CAP) st |= 2;
        if (st) {
            atomicOr(status, st);
            if (qstatus) atomicOr(qstatus + qi, st);          // which query: the caller repeats only those
        }
    }
    __shared__ unsigned hist[256];
    __shared__ unsigned s_aux[8], survivors;
    __shared__ unsigned s_scan[4];
    int n = cnt;
    bool in_lds = cnt <= cap;                                 // block-uniform
    if ((cnt > 2048 && cnt > 2 * k) || !in_lds) {
        if (tid == 0) survivors = 0u;
        // k-th largest score key (barriers inside); the bin list borrows the (still unused) key buffer
        const unsigned kth = adc_kth_largest_v([&](int64_t i) { return (unsigned)(gk[i] >> 32); }, cnt, (unsigned)(k < cnt ? k : cnt),
                                               hist, s_scan, s_aux, reinterpret_cast<unsigned*>(lk), 2 * cap);
        __syncthreads();
        for (int i = tid; i < cnt; i += nthr) {
            const unsigned long long key = gk[i];
            if ((unsigned)(key >> 32) >= kth) {
                const unsigned slot = atomicAdd(&survivors, 1u);
                if ((int)slot < cap) lk[adc_sp((int)slot)] = key;
            }
        }
        __syncthreads();
        in_lds = (int)survivors <= cap;
        if (in_lds) n = (int)survivors;                       // >= min(k, cnt)
    }
    int P = 1024;
    while (P < n) P <<= 1;
    if (!in_lds) {
        for (int i = cnt + tid; i < P; i += nthr) gk[i] = 0ull;           // P <= ADC_CAND_CAP
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += nthr) {
                    const int lo = ((t / stride) * (stride << 1)) + (t % stride);
                    const int hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const unsigned long long a = gk[lo], b = gk[hi];
                    if ((a < b) == desc) { gk[lo] = b; gk[hi] = a; }
                }
                __syncthreads();
            }
        }
    } else {
        if (n != cnt) {
            for (int i = n + tid; i < P; i += nthr) lk[adc_sp(i)] = 0ull;
        } else {
            for (int i = tid; i < P; i += nthr) lk[adc_sp(i)] = (i < cnt) ? gk[i] : 0ull;
        }
        __syncthreads();
        adc_bitonic_sort_lds(lk, P, tid, nthr);
    }
    for (int j = tid; j < k; j += nthr) {
        float sc = -INFINITY;
        int64_t id = -1;
        if (j < n) {
            const unsigned long long key = in_lds ? lk[adc_sp(j)] : gk[j];
            sc = adc_unorder_key((unsigned)(key >> 32));
            id = (int64_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) + id_offset;
        }
        scores[(size_t)qi * k + j] = sc;
        ids[(size_t)qi * k + j] = id;
    }
}

// sort + emit stage: the k best of the cnt[q] keys of cand[q][ADC_CAND_CAP] -> scores / ids [nq][k]
int rc_adc_launch_select(rc_handle_t h, unsigned long long* cand, const unsigned* cnt, int nq, int64_t N, int k,
                         int64_t id_offset, float* scores, int64_t* ids, int* status, hipStream_t s, int* qstatus) {
    int cap = 4096;                                            // keys held in LDS: >= max(2048, 2 k), see adc_select_kernel
    while (cap < 2 * k && cap < ADC_CAND_CAP) cap <<= 1;
    if (const int e = rc_env_int("RC_ADC_SELECT_CAP", 0)) cap = e;        // tests: 1024 forces the global-memory sort
    const size_t ss = (size_t)(cap + cap / 32) * sizeof(unsigned long long);       // padded positions, adc_sp
    const int nthr = cap <= 8192 ? 512 : 1024;
    RC_HIP_CHECK(h, hipFuncSetAttribute((const void*)adc_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)((ADC_CAND_CAP + ADC_CAND_CAP / 32) * sizeof(unsigned long long))));
    hipLaunchKernelGGL(adc_select_kernel, dim3((unsigned)nq), dim3(nthr), ss, s, cand, cnt, N, k, id_offset, scores, ids,
                       status, qstatus, cap);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ------------------------------------------------------------------------------------------ exact select
// The k-th largest 64-bit key (adc_exact_key: distinct for distinct rows, so "the k best in (score desc, id asc) order" is a
// unique set) of a query's full score row by an 8-pass byte-wise radix select over all rows, then a compaction of the keys
// >= that key (exactly min(k, N) of them) and the ordinary sort + emit.
// grid (slices, queries of the round): histogram of byte `pass` (0 = most significant) over the keys whose higher bytes
// equal prefix[q]
__global__ __launch_bounds__(256) void adc_exact_hist_kernel(const float* __restrict__ sc, int64_t N,
                                                             const unsigned long long* __restrict__ prefix, int pass,
                                                             unsigned* __restrict__ hist) {
    __shared__ unsigned h[256];
    const int qx = blockIdx.y, tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const unsigned long long pf = prefix[qx];
    const int shift = 56 - 8 * pass;
    const unsigned long long himask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    const float* row = sc + (size_t)qx * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < N; i += (int64_t)gridDim.x * 256) {
        const unsigned long long key = adc_exact_key(row[i], i);
        if ((key & himask) == pf) atomicAdd(&h[(unsigned)(key >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(hist + (size_t)qx * 256 + tid, h[tid]);
}
// one block of 256 threads per query: the bin that holds the rank-th largest key; prefix and rank move on, hist is zeroed
__global__ __launch_bounds__(256) void adc_exact_pick_kernel(unsigned* __restrict__ hist, unsigned long long* __restrict__ prefix,
                                                             unsigned* __restrict__ rank, int pass) {
    __shared__ unsigned s_scan[4];
    __shared__ unsigned sel_prefix, sel_rank;
    const int qx = blockIdx.x, tid = threadIdx.x;
    unsigned* hq = hist + (size_t)qx * 256;
    const unsigned need = rank[qx];
    if (tid == 0) { sel_prefix = 0u; sel_rank = need; }
    __syncthreads();
    adc_pick_bin(hq, need, 0u, 0, s_scan, &sel_prefix, &sel_rank);     // bin index lands in sel_prefix (shift 0, prefix 0)
    if (tid == 0) {
        prefix[qx] |= (unsigned long long)(sel_prefix & 0xFFu) << (56 - 8 * pass);
        rank[qx] = sel_rank;
    }
    hq[tid] = 0u;
}
__global__ __launch_bounds__(256) void adc_exact_init_kernel(unsigned* __restrict__ hist, unsigned long long* __restrict__ prefix,
                                                             unsigned* __restrict__ rank, unsigned* __restrict__ cnt, unsigned want) {
    const int qx = blockIdx.x, tid = threadIdx.x;
    hist[(size_t)qx * 256 + tid] = 0u;
    if (tid == 0) { prefix[qx] = 0ull; rank[qx] = want; cnt[qx] = 0u; }
}
// keys >= the selected key (= the min(k, N) best rows) go to the candidate list
__global__ __launch_bounds__(256) void adc_exact_collect_kernel(const float* __restrict__ sc, int64_t N,
                                                                const unsigned long long* __restrict__ prefix,
                                                                unsigned* __restrict__ cand_count,
                                                                unsigned long long* __restrict__ cand) {
    const int qx = blockIdx.y, tid = threadIdx.x;
    const unsigned long long kth = prefix[qx];
    const float* row = sc + (size_t)qx * N;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < N; i0 += (int64_t)gridDim.x * 256) {      // wave-uniform trip count
        const int64_t i = i0 + tid;
        const unsigned long long key = i < N ? adc_exact_key(row[i], i) : 0ull;
        const bool pass = i < N && key >= kth;
        const unsigned long long mask = __ballot(pass);
        if (mask) {
            const unsigned slot = adc_wave_append(mask, cand_count + qx);
            if (pass && slot < ADC_CAND_CAP) cand[(size_t)qx * ADC_CAND_CAP + slot] = key;
        }
    }
}

// The select stage of the exact route for nx queries whose full score rows sc[nx][N] are written: the min(k, N) best
// 64-bit keys by the 8-pass radix select, compacted and sorted + emitted (callers: rc_adc_search_exact,
// the dense search).  hist [nx][256], prefix [nx], rank [nx], cnt [nx], cand [nx][ADC_CAND_CAP] (topk_exact_ws); status: a device int.
int rc_adc_launch_exact_select(rc_handle_t h, const float* sc, int64_t N, int nx, int k, int64_t id_offset, unsigned* hist,
                               unsigned long long* prefix, unsigned* rank, unsigned* cnt, unsigned long long* cand,
                               int* status, float* scores, int64_t* ids, hipStream_t s) {
    const unsigned want = (unsigned)((int64_t)k < N ? (int64_t)k : N);
    unsigned slices = (unsigned)((N + 256 * 64 - 1) / (256 * 64));
    if (slices > 2048) slices = 2048;
    hipLaunchKernelGGL(adc_exact_init_kernel, dim3((unsigned)nx), dim3(256), 0, s, hist, prefix, rank, cnt, want);
    RC_LAUNCH_CHECK(h);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(adc_exact_hist_kernel, dim3(slices, (unsigned)nx), dim3(256), 0, s, sc, N,
                           (const unsigned long long*)prefix, pass, hist);
        RC_LAUNCH_CHECK(h);
        hipLaunchKernelGGL(adc_exact_pick_kernel, dim3((unsigned)nx), dim3(256), 0, s, hist, prefix, rank, pass);
        RC_LAUNCH_CHECK(h);
    }
    hipLaunchKernelGGL(adc_exact_collect_kernel, dim3(slices, (unsigned)nx), dim3(256), 0, s, sc, N,
                       (const unsigned long long*)prefix, cnt, cand);
    RC_LAUNCH_CHECK(h);
    return rc_adc_launch_select(h, cand, cnt, nx, N, k, id_offset, scores, ids, status, s);
}
