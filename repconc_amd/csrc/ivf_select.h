// What the IVF searches that write a dense score row per query do after their scan (rc_ivf_search over PQ codes in
// ivf_search.hip, rc_ivf_flat_search over dense rows in ivf_flat.hip): the exact k-th largest score of every query and the
// keys of the rows at or above it; rc_adc_launch_select (topk.hip) sorts and emits them.  No sampling and no slack: the only
// query this cannot answer is one with more than ADC_CAND_CAP rows tied at its k-th score (status bit 1 of the select).
// Device code: every unit compiles its own copy (static kernels, no -fgpu-rdc).
#pragma once
#include "topk.h"

// thr[qi] = k-th largest of dense[qi][0..count[qi]) (or -inf when count < k).  One block per query.
static __global__ __launch_bounds__(1024) void ivf_kth_kernel(const float* __restrict__ dense, const int* __restrict__ count,
                                                              int64_t stride, int k, float* __restrict__ thr) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_rank;
    const int qi = blockIdx.x, tid = threadIdx.x;
    const int n = count[qi];
    if (n < k || k <= 0) {
        if (tid == 0) thr[qi] = -INFINITY;
        return;
    }
    const float* row = dense + (size_t)qi * stride;
    if (tid == 0) { sel_prefix = 0u; sel_rank = (unsigned)k; }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = sel_prefix;
        const unsigned himask = (pass == 0) ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < n; i += 1024) {
            const unsigned key = adc_order_key(row[i]);
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFFu], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned need = sel_rank, b = 255;
            for (;; --b) {
                if (hist[b] >= need) break;
                need -= hist[b];
                if (b == 0) break;
            }
            sel_prefix = prefix | (b << shift);
            sel_rank = need;
        }
        __syncthreads();
    }
    if (tid == 0) thr[qi] = adc_unorder_key(sel_prefix);
}

// grid (nq, chunks).  Keys of the rows with score >= thr[qi]; id = ids[rowid] (the corpus position of the row; rowid holds
// the 32 bits of a row number < 2^32).
static __global__ __launch_bounds__(256) void ivf_filter_kernel(const float* __restrict__ dense, const int* __restrict__ rowid,
                                                                const int* __restrict__ count, int64_t stride,
                                                                const float* __restrict__ thr, const int64_t* __restrict__ ids,
                                                                unsigned* __restrict__ cand_count,
                                                                unsigned long long* __restrict__ cand) {
    const int qi = blockIdx.x;
    const int n = count[qi];
    const float tau = thr[qi];
    const float* row = dense + (size_t)qi * stride;
    const int* rid = rowid + (size_t)qi * stride;
    const int per = (n + gridDim.y - 1) / gridDim.y;
    const int i0 = blockIdx.y * per, i1 = (i0 + per < n) ? i0 + per : n;
    for (int ib = i0; ib < i1; ib += 256) {
        const int i = ib + threadIdx.x;
        const bool live = i < i1;
        const float s = live ? row[i] : -INFINITY;
        const bool pass = live && (s >= tau);
        const unsigned long long mask = __ballot(pass);
        if (mask) {
            const unsigned slot = adc_wave_append(mask, cand_count + qi);
            if (pass && slot < ADC_CAND_CAP) {
                const unsigned id = (unsigned)ids[(unsigned)rid[i]];
                cand[(size_t)qi * ADC_CAND_CAP + slot] = adc_exact_key(s, id);
            }
        }
    }
}

// the two launches between a scan and rc_adc_launch_select; cnt [nq] is cleared here
static inline int ivf_launch_kth_filter(rc_handle_t h, const float* dense, const int* rowid, const int* count, int nq,
                                        int64_t stride, int k, const int64_t* ids, float* thr, unsigned* cnt,
                                        unsigned long long* cand, hipStream_t s) {
    hipLaunchKernelGGL(ivf_kth_kernel, dim3((unsigned)nq), dim3(1024), 0, s, dense, count, stride, k, thr);
    RC_LAUNCH_CHECK(h);
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    int chunks = (int)((stride + 16383) / 16384);
    if (chunks < 1) chunks = 1;
    if (chunks > 64) chunks = 64;
    hipLaunchKernelGGL(ivf_filter_kernel, dim3((unsigned)nq, (unsigned)chunks), dim3(256), 0, s, dense, rowid, count, stride,
                       (const float*)thr, ids, cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
