// What the two pipelined IVF screens share (ivfs_screen8.h: ivfs_screen_kernel, 8 queries per gather; ivfs_screen16.h:
// ivfs_screen16_kernel, 16 queries per gather; both included by ivf_lists.hip): the block geometry, the block's share of the
// task list, the rows of a task's cell, a wave's chunks of a round, the integer threshold of a lane's column, the barrier, the
// priority ladder of a stage and the survivor stream.  Everything is __device__ __forceinline__: the kernels sit at the 128
// VGPRs that give them 4 waves per SIMD, and a call must cost what the text written out in the kernel did.
#pragma once
#include "adc_common.h"
#include <type_traits>

#define IVFS_WAVES 16
#define IVFS_THREADS (64 * IVFS_WAVES)
#define IVFS_BUF 65536           // one table buffer; a kernel holds two
#define IVFS_MAX_BLOCKS 256      // persistent blocks (one per CU); sizes the survivor streams of the workspace
#ifndef IVFS_PRIO
#define IVFS_PRIO 1
#endif
// the per-query byte tables are stored in phases of 32 sub-quantisers (+ one of 16 for M = 16 / 48): ivfs_qprep_kernel
__host__ __device__ constexpr int ivfs_phases(int M) { return (M + 31) / 32; }
__host__ __device__ constexpr int ivfs_pm(int M, int p) { return (M - 32 * p) >= 32 ? 32 : 16; }

// (block-uniform values; the loads are vector loads - the kernels also store - so pin them to scalars)
__device__ __forceinline__ int ivfs_sc(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- the block's share of the task list: XCD x owns a contiguous eighth of the cell-ordered list, its blocks take the tasks
// round-robin so that the tasks of one cell run side by side in one L2
struct ivfs_share {
    unsigned lo, cnt;         // the XCD's tasks: [lo, lo + cnt)
    unsigned jb, pxb;         // this block is number jb of the pxb blocks of its XCD
};
__device__ __forceinline__ ivfs_share ivfs_block_share(const adc_ivf_tasks& T, int ntasks_arg) {
    const unsigned total = (unsigned)__builtin_amdgcn_readfirstlane(T.ntasks ? *T.ntasks : ntasks_arg);
    const unsigned xcd = blockIdx.x % 8u, tq8 = total / 8u, tr8 = total % 8u;
    ivfs_share s;
    s.jb = blockIdx.x / 8u;
    s.pxb = (gridDim.x - xcd + 7u) / 8u;
    s.lo = xcd < tr8 ? xcd * (tq8 + 1u) : tr8 * (tq8 + 1u) + (xcd - tr8) * tq8;
    s.cnt = tq8 + (xcd < tr8 ? 1u : 0u);
    return s;
}
// the block's k-th task: its index in the task list, or false when the block has fewer
__device__ __forceinline__ bool ivfs_share_task(const ivfs_share& s, unsigned k, unsigned& task) {
    const unsigned at = s.jb + k * s.pxb;
    task = s.lo + at;
    return at < s.cnt;
}

// ---- the rows of a task: the cell's range, counted from the 16-row chunk its first row falls in
struct ivfs_rows {
    unsigned t0;              // first (16-aligned) row of the range
    unsigned row_lo, nrows;   // rows [row_lo, nrows) counted from t0 are the cell's (nrows = 0: nothing to scan)
};
__device__ __forceinline__ ivfs_rows ivfs_cell_rows(const adc_ivf_tasks& T, int cell, int qc) {
    ivfs_rows d = {0u, 0u, 0u};
    const unsigned a = (unsigned)ivfs_sc((int)T.list_off[cell]), b = (unsigned)ivfs_sc((int)T.list_off[cell + 1]);   // N < 2^32
    if (qc > 0 && b > a) {
        const unsigned t0 = a & ~15u;
        d.t0 = t0; d.row_lo = a - t0; d.nrows = b - t0;
    }
    return d;
}
// rounds of ROUND = GW * R * 16 rows that cover the task's rows (an empty task still takes one pass through the stages)
template <int ROUND>
__device__ __forceinline__ int ivfs_rounds_of(const ivfs_rows& d) { return d.nrows ? (int)((d.nrows + ROUND - 1) / ROUND) : 1; }
// chunks wave wv owns in round rd (wave-uniform, 0 .. R): chunk c of wave wv is chunk GW c + wv of the round (the waves share a
// short cell evenly: a cell of 1770 rows = 111 chunks costs every gathering wave 9 or 10 chunks, not the first eleven 10)
template <int GW, int R>
__device__ __forceinline__ int ivfs_chunks_of(unsigned nrows, int rd, int wv) {
    constexpr unsigned ROUND = GW * R * 16;
    const unsigned done = (unsigned)rd * ROUND;
    if (nrows <= done) return 0;
    unsigned nc = (nrows - done + 15u) / 16u;                 // chunks of the round that hold rows of the cell
    if (nc > ROUND / 16u) nc = ROUND / 16u;
    if (wv >= GW) return 0;                                    // a loader wave
    const int mine = ((int)nc - wv + GW - 1) / GW;
    return mine < 0 ? 0 : mine;
}
// integer threshold of a lane's query column against the BIASED byte sums (b ^ 0x80 per sub-quantiser); no query: nothing passes
template <int M>
__device__ __forceinline__ int ivfs_lane_thr(const int* __restrict__ tint, int q) {
    if (q < 0) return INT_MAX;
    const int t = tint[q];
    return (t == INT_MIN) ? INT_MIN : t - 128 * M;
}

__device__ __forceinline__ void ivfs_block_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// progress-proportional priority: a wave that is behind in its stage (chunk c of R) outranks one that is ahead
template <int R>
__device__ __forceinline__ void ivfs_prio_at(int c) {
#if IVFS_PRIO
    if (c == 0) __builtin_amdgcn_s_setprio(3);
    else if (c == R / 4) __builtin_amdgcn_s_setprio(2);
    else if (c == R / 2) __builtin_amdgcn_s_setprio(1);
    else if (c == 3 * R / 4) __builtin_amdgcn_s_setprio(0);
#endif
}
__device__ __forceinline__ void ivfs_prio_done() {
#if IVFS_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
}

// ---- survivors
// No atomics here: a returning atomic costs the wave its round trip at the next vmcnt wait on anything older (the
// counter is in-order), ~1-3 us per task with sixteen waves meeting at the next barrier.  Every wave appends (query, row)
// pairs to its OWN stream in global memory (stream_cap pairs, running offset woff in a scalar); ivfs_bucket_kernel deals the
// streams to the per-query id lists afterwards.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ivfs_stream_rsrc(unsigned* stream, unsigned stream_cap, int wv) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(stream + (size_t)(blockIdx.x * IVFS_WAVES + (unsigned)wv) * stream_cap * 2u), 0, -1,
                                             0x00020000);
}
// One round of a task, after its last phase: acc[c][e] = the sum of row 4 g + e of the wave's chunk c for query column r
// (l = 16 g + r; the columns QW .. 15 hold nothing), tq / myq = threshold and query of the lane's column, reff = the wave's
// chunks of the round.  One branch-free pass over the lane's 4 R sums builds a bit mask of its survivors (a divergent branch per
// sum cost 3 us per task); the lanes' counts give the positions (query column major: a stream holds runs of equal query
// ids), then the lanes write out one survivor per trip of a wave-uniform loop (max count over the lanes: 1-3 trips).
template <int R, int GW, int QW>
__device__ __forceinline__ void ivfs_survivors(const adc_i32x4v (&acc)[R], const ivfs_rows& rows, int rd, int tq, int myq, int reff,
                                               int wv, int l, unsigned stream_cap, int* __restrict__ status,
                                               const __amdgpu_buffer_rsrc_t strsrc, unsigned& woff) {
    static_assert(R * 4 <= 64, "one mask bit per sum");
    static_assert(QW == 8 || QW == 16, "query columns of a task");
    typedef typename std::conditional<(R * 4 <= 32), unsigned, unsigned long long>::type mask_t;
    typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
    if (reff <= 0) return;                                    // wave-uniform: no rows of the cell in this wave's share
    const int r = l & 15, g = l >> 4;
    const unsigned rb = (unsigned)rd * (unsigned)(GW * R * 16) + (unsigned)(wv * 16);      // first row of the wave's chunk 0
    mask_t m = 0;                                             // bit 4 c + e: D[row 4 g + e of chunk c][column r] survives
#pragma unroll
    for (int c = 0; c < R; ++c) {
        if (c < reff) {
#pragma unroll
            for (int e = 0; e < 4; ++e) m |= (acc[c][e] >= tq) ? ((mask_t)1 << (4 * c + e)) : (mask_t)0;
        }
    }
    // rows outside the cell (before its first row in the first chunk, after its last in the last): never survivors
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const unsigned cb = rb + (unsigned)(16 * GW * c);
        if (c < reff && (cb < rows.row_lo || cb + 16u > rows.nrows)) {        // wave-uniform, rare
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned n = cb + 4u * g + e;
                if (n < rows.row_lo || n >= rows.nrows) m &= ~((mask_t)1 << (4 * c + e));
            }
        }
    }
    const unsigned cnt = (unsigned)__popcll((unsigned long long)m);
    if (!__ballot(cnt != 0)) return;
    const unsigned c0 = __shfl(cnt, r), c1 = __shfl(cnt, r + 16), c2 = __shfl(cnt, r + 32), c3 = __shfl(cnt, r + 48);
    const unsigned tot = c0 + c1 + c2 + c3;
    const unsigned lane_first = (g > 0 ? c0 : 0u) + (g > 1 ? c1 : 0u) + (g > 2 ? c2 : 0u);
    unsigned inc = tot;                                       // inclusive prefix over the QW query columns r of the lane's row
#pragma unroll
    for (int o = 1; o < QW; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 16);
        if (r >= o) inc += t;
    }
    const unsigned wtotal = (unsigned)__builtin_amdgcn_readlane((int)inc, QW - 1);
    if (woff + wtotal > stream_cap) {                         // wave-uniform; status bit 2: a stream filled up (no query to blame)
        if (l == 0) atomicOr(status, 4);
        return;
    }
    unsigned at = (woff + (inc - tot) + lane_first) * 8u;      // byte offset of the lane's first pair
    const unsigned row0 = rows.t0 + rb + 4u * (unsigned)g;
    while (__ballot(m != 0)) {                                 // wave-uniform
        if (m) {
            const unsigned idx = (unsigned)__builtin_ctzll((unsigned long long)m);
            m &= m - (mask_t)1;
            const u32x2s v = {(unsigned)myq, row0 + (idx >> 2) * (unsigned)(16 * GW) + (idx & 3u)};
            __builtin_amdgcn_raw_buffer_store_b64(v, strsrc, at, 0, 0);
            at += 8u;
        }
    }
    woff += wtotal;
}
