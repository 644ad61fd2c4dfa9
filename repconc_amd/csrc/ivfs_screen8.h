// 8-query form of the pipelined IVF screen (round 3; included by ivf_lists.hip; its 16-query sibling is ivfs_screen16.h, what
// the two share is ivfs_common.h): the image of the cell-major codes, its kernel, and ivfs_screen_kernel.
//
// A wall-clock trace of the round-2 screen on the BASELINE configs[3] shape (M = 96, 5000 cells of ~1770 rows, nprobe 128:
// 19 k tasks of 8 queries) showed where a task's 15.9 us went: 1.6 us of dependent scalar loads
// (task -> queries -> thresholds), 2.9 + 4.3 us for the two synchronous table fills (128 KiB each: loads from the
// memory-side cache, byte transposes, a block-wide barrier either side), 2.2 + 1.6 us of gathers and 3.1 us for the
// returning atomics of the survivor slots — with one 128 KiB block per CU nothing overlaps any of it.  Two blocks per CU
// (three 64 KiB phases) measured the same: more fills and barriers eat what the overlap gives.
// This kernel keeps ONE persistent block per CU and overlaps by construction:
//   * table phases of 32 sub-quantisers (+ one of 16 for M = 16 / 48): 64 KiB, TWO buffers.  The block's last LW = 4 waves do
//     nothing but fetch, transpose and store the NEXT stage's tables into the other buffer while the other twelve gather: one
//     barrier per stage, no load latency on the critical path;
//   * the block walks its share of the tasks (ivfs_block_share); task descriptors are read one task ahead;
//   * the codes of the next stage are requested right after the current stage's last gather (same registers);
//   * survivors go to the wave's own stream without atomics (ivfs_survivors).
// The per-query byte tables are stored biased (b ^ 0x80) by ivfs_qprep_kernel.
#include "ivfs_common.h"

// Image of the list-centric IVF search, blocked by chunks of 16 rows (the unit a wave gathers for): chunk n / 16 holds
// [phase p][lane quarter g][row n mod 16][step s] = codes[n][32 p + m(s; n mod 16, g)], i.e. a wave's load of one chunk and
// phase is 64 lanes x PMp / 4 bytes of CONTIGUOUS memory (with row-major rows it was sixteen 32-byte pieces 96 bytes apart:
// 12-16 cache lines per instruction, and the sixteen waves of a block issue theirs at the same moment).
__host__ __device__ inline int64_t ivfs_image_at(int M, int64_t n, int p, int g, int st) {
    const int PM = ivfs_pm(M, p);
    return (n >> 4) * (int64_t)(16 * M) + (int64_t)(16 * 32 * p) + (int64_t)((g * 16 + (int)(n & 15)) * (PM / 4) + st);
}
__global__ __launch_bounds__(256) void ivfs_image_kernel(const uint8_t* __restrict__ codes, int64_t n0, int64_t cnt, int M,
                                                         uint8_t* __restrict__ image) {
    const int64_t total = cnt * M;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t n = n0 + i / M;
        const int pos = (int)(i % M);
        const int p = pos / 32, rem = pos % 32, PM = ivfs_pm(M, p);
        const int g = rem / (PM / 4), st = rem % (PM / 4);
        int slot, m;
        adc_cf_step(PM, st, (int)(n & 15), g, slot, m);
        image[ivfs_image_at(M, n, p, g, st)] = codes[n * M + 32 * p + m];
    }
}
// The same image read the other way, in 16-byte pieces (adc_select.h): a chunk of 16 rows owns 16 M contiguous bytes, phases of
// 512 bytes (the last one of M = 16 / 48: 256), [lane quarter g][row][step]; piece o = (chunk o / M of the block, piece o % M)
struct adc_sel_rows {
    __host__ __device__ static int64_t dest(int M, int64_t i0, int o) {
        return ((i0 >> 4) + o / M) * (int64_t)(16 * M) + (int64_t)(o % M) * 16;
    }
    __host__ __device__ static void src(int M, int o, int b, int& row, int& m) {
        const int x = 16 * (o % M) + b, p = x >> 9, rem = x & 511, PM = ivfs_pm(M, p);
        const int lane = rem / (PM / 4), st = rem % (PM / 4);
        int slot;
        adc_cf_step(PM, st, lane & 15, lane >> 4, slot, m);
        m += 32 * p;
        row = 16 * (o / M) + (lane & 15);
    }
};

struct ivfs_task {
    int valid;
    int qid[8];
    ivfs_rows rows;
};

// 8 x 8 byte transpose: d[j] = dword i of query j's phase table (four sub-quantisers of one code) -> o[2 t + hq] = byte t of
// queries 4 hq .. 4 hq + 3, i.e. o[2 t], o[2 t + 1] = the 8-byte LDS entry of sub-quantiser t; o[0 .. 3] / o[4 .. 7] = the
// lo / hi 16 bytes of the code's 32-byte piece
__device__ __forceinline__ void ivfs_transpose8(const unsigned (&d)[8], unsigned (&o)[8]) {
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
        const unsigned a0 = d[4 * hq], a1 = d[4 * hq + 1], a2 = d[4 * hq + 2], a3 = d[4 * hq + 3];
        const unsigned t0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), t1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
        const unsigned u0 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), u1 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
        o[0 + hq] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
        o[2 + hq] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
        o[4 + hq] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
        o[6 + hq] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
    }
}

// LW loader waves (4 in the shipped library): the block's last LW waves do nothing but fetch, transpose and store the NEXT
// stage's tables while the other 16 - LW gather — the fill runs beside the gathers instead of after them.
// Development aid (tools/ivf_timeline.py builds a variant library with -DRC_IVF_TRACE): wall-clock stamps of every wave at the
// stage boundaries of the first tasks of every block, read back with rc_debug_ivfs_trace.  Off in the shipped library.
#ifdef RC_IVF_TRACE
__device__ unsigned long long ivfs_trace[256 * 8 * 3 * 16 * 4];
extern "C" int rc_debug_ivfs_trace(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ivfs_trace), sizeof(ivfs_trace));
}
#define IVFS_TSTAMP(i)                                                                                                 \
    do {                                                                                                               \
        if (l == 0 && k < 8u && rd == 0 && blockIdx.x < 256u)                                                          \
            ivfs_trace[(((blockIdx.x * 8u + k) * 3u + (unsigned)P) * 16u + (unsigned)wv) * 4u + (i)] = wall_clock64(); \
    } while (0)
#else
#define IVFS_TSTAMP(i) do { } while (0)
#endif
template <int M, int LW>
__global__ __launch_bounds__(IVFS_THREADS, 4) void ivfs_screen_kernel(const uint8_t* __restrict__ image,
                                                                      const int* __restrict__ tint,
                                                                      unsigned* __restrict__ stream_cnt,
                                                                      unsigned* __restrict__ stream, unsigned stream_cap,
                                                                      int* __restrict__ status, adc_ivf_tasks T,
                                                                      int ntasks_arg) {
    static_assert(LW > 0, "loader waves");
    constexpr int GW = IVFS_WAVES - LW;                       // gathering waves
    constexpr int R = 10;                                     // twelve gathering waves: ten chunks each cover a 1920-row round
    constexpr int NPH = ivfs_phases(M), ROUND = GW * R * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned tid = threadIdx.x;
    const int l = (int)(tid & 63u), wv = __builtin_amdgcn_readfirstlane((int)(tid >> 6)), r = l & 15, g = l >> 4;
    const ivfs_share share = ivfs_block_share(T, ntasks_arg);
    auto load_task = [&](unsigned k) {
        ivfs_task d;
        unsigned task;
        d.valid = ivfs_share_task(share, k, task) ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) d.qid[j] = -1;
        d.rows = ivfs_rows{0u, 0u, 0u};
        if (d.valid) {
            const int qs = ivfs_sc(T.task_qstart[task]), qc = ivfs_sc(T.task_qcnt[task]), cell = ivfs_sc(T.task_list[task]);
#pragma unroll
            for (int j = 0; j < 8; ++j) d.qid[j] = (j < qc) ? ivfs_sc(T.sorted_q[qs + j]) : -1;
            d.rows = ivfs_cell_rows(T, cell, qc);
        }
        return d;
    };
    // query id of this lane's column (r < 8) for a task
    auto lane_q = [&](const ivfs_task& d) {
        int q = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) q = (r == j) ? d.qid[j] : q;
        return q;
    };
    // ---- tables: global -> registers -> (byte transpose) -> LDS
    // dword i of a query's phase table ([code][PM] bytes) = sub-quantisers 4 u .. 4 u + 3 of code i / (PM / 4); its LDS
    // entries are slots 4 u .. 4 u + 3 of that code's row (256 bytes = 32 slots x 8 queries; a 16-block is stored twice)
    constexpr int DD = 2;                                     // 2048 dwords per query and 32-phase / 1024 threads (the prologue)
    // Buffer loads: ONE vector offset (tid * 4) for all eight queries, the query's table comes in through the scalar offset
    // (with flat pointers the compiler forms eight 64-bit vector addresses, hoists them and spills)
    const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)T.qbyte, 0, -1, 0x00020000);
    auto load_tables = [&](auto PMc, int p, const ivfs_task& d, unsigned (&dd)[DD][8]) {
        constexpr int PM = decltype(PMc)::value;
        constexpr int FI = RC_K * PM / 4 / IVFS_THREADS;      // 2 (PM = 32) or 1
        // (an empty slot reads query 0's table: its column is masked by the threshold INT_MAX)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned so = (unsigned)(d.qid[j] < 0 ? 0 : d.qid[j]) * (unsigned)(M * RC_K) + (unsigned)(RC_K * 32 * p);
            if constexpr (FI == 2) {                           // dwords 2 tid, 2 tid + 1 of the query's phase table in one load
                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(qrsrc, tid * 8u, so, 0);
                dd[0][j] = v.x; dd[1][j] = v.y;
            } else {
                dd[0][j] = __builtin_amdgcn_raw_buffer_load_b32(qrsrc, tid * 4u, so, 0);
            }
        }
    };
    // byte transpose of dword i of the eight queries' phase tables -> the 32 bytes of LDS entries 4 u .. 4 u + 3 of its code
    auto emit_entry = [&](auto PMc, const unsigned (&d)[8], unsigned i, unsigned bufoff) {
        constexpr int PM = decltype(PMc)::value;
        unsigned o[8];                                       // o[2 t] = queries 0-3 of entry t, o[2 t + 1] = queries 4-7
        ivfs_transpose8(d, o);
        const uint4 lo4 = make_uint4(o[0], o[1], o[2], o[3]), hi4 = make_uint4(o[4], o[5], o[6], o[7]);
        if constexpr (PM == 32) {
            uint4* e = reinterpret_cast<uint4*>(smem + (bufoff + i * 32u));
            e[0] = lo4;
            e[1] = hi4;
        } else {
            uint4* e = reinterpret_cast<uint4*>(smem + (bufoff + (i >> 2) * 256u + (i & 3u) * 32u));
            e[0] = lo4;
            e[1] = hi4;
            e[8] = lo4;                                      // second copy, 16 slots further
            e[9] = hi4;
        }
    };
    auto write_tables = [&](auto PMc, const unsigned (&dd)[DD][8], unsigned bufoff) {
        constexpr int PM = decltype(PMc)::value;
        constexpr int FI = RC_K * PM / 4 / IVFS_THREADS;
#pragma unroll
        for (int f = 0; f < FI; ++f) emit_entry(PMc, dd[f], FI == 2 ? 2u * tid + (unsigned)f : tid, bufoff);
    };
    // loader waves: the whole phase by LW * 64 threads, 64 table registers per batch.
    // 32-phase: consecutive lanes take consecutive dwords (4-byte loads), so lane l's entry is 32 bytes at 32 i, i = l (mod 64).
    // Written as lo half then hi half by every lane, the 16 lanes the LDS serves together ({0-3, 12-15, 20-27}, ...) hit 8
    // bank quads twice (and with the 8-byte loads of the first version, 64 bytes per lane, four times: PMC showed 39 % of
    // the kernel's LDS cycles as bank conflicts).  Lanes with bit 3 set write their HI half first: the two lanes of a group that
    // share i mod 8 then differ in the half, 16 distinct quads per group.
    auto loader_fill = [&](auto PMc, int p, const ivfs_task& d, unsigned bufoff) {
        constexpr int PM = decltype(PMc)::value;
        constexpr int LT = LW * 64;
        const unsigned lt = tid - (unsigned)(GW * 64);
        unsigned so[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) so[j] = (unsigned)(d.qid[j] < 0 ? 0 : d.qid[j]) * (unsigned)(M * RC_K) + (unsigned)(RC_K * 32 * p);
        if constexpr (PM == 32) {
            constexpr int NDW = RC_K * PM / 4, ITER = NDW / LT, BATCH = ITER < 8 ? ITER : 8;
            static_assert(NDW % LT == 0 && ITER % BATCH == 0, "whole batches");
            const bool hi_first = ((lt >> 3) & 1u) != 0;
#pragma unroll
            for (int b0 = 0; b0 < ITER; b0 += BATCH) {
                unsigned dq[BATCH][8];
#pragma unroll
                for (int it = 0; it < BATCH; ++it)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        dq[it][j] = __builtin_amdgcn_raw_buffer_load_b32(qrsrc, ((unsigned)((b0 + it) * LT) + lt) * 4u, so[j], 0);
#pragma unroll
                for (int it = 0; it < BATCH; ++it) {
                    const unsigned i = (unsigned)((b0 + it) * LT) + lt;
                    unsigned o[8];
                    ivfs_transpose8(dq[it], o);
                    const uint4 first = hi_first ? make_uint4(o[4], o[5], o[6], o[7]) : make_uint4(o[0], o[1], o[2], o[3]);
                    const uint4 second = hi_first ? make_uint4(o[0], o[1], o[2], o[3]) : make_uint4(o[4], o[5], o[6], o[7]);
                    unsigned char* e = smem + (bufoff + i * 32u);
                    *reinterpret_cast<uint4*>(e + (hi_first ? 16 : 0)) = first;
                    *reinterpret_cast<uint4*>(e + (hi_first ? 0 : 16)) = second;
                }
            }
        } else {
            constexpr int NPAIR = RC_K * PM / 8, ITER = NPAIR / LT, BATCH = ITER < 4 ? ITER : 4;
            static_assert(NPAIR % LT == 0 && ITER % BATCH == 0, "whole batches");
#pragma unroll
            for (int b0 = 0; b0 < ITER; b0 += BATCH) {
                unsigned dq[BATCH][2][8];
#pragma unroll
                for (int it = 0; it < BATCH; ++it)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(qrsrc, ((unsigned)((b0 + it) * LT) + lt) * 8u, so[j], 0);
                        dq[it][0][j] = v.x; dq[it][1][j] = v.y;
                    }
#pragma unroll
                for (int it = 0; it < BATCH; ++it)
#pragma unroll
                    for (int f = 0; f < 2; ++f) emit_entry(PMc, dq[it][f], 2u * ((unsigned)((b0 + it) * LT) + lt) + (unsigned)f, bufoff);
            }
        }
    };
    // ---- codes of one stage: the wave's chunks of the round (ivfs_chunks_of); PM / 16 dwords per lane and chunk
    auto chunks_of = [&](unsigned nrows, int rd) { return ivfs_chunks_of<GW, R>(nrows, rd, wv); };
    auto load_codes = [&](auto PMc, int p, unsigned t0, unsigned nrows, int rd, unsigned (&w)[R][2]) {
        constexpr int PM = decltype(PMc)::value;
        constexpr int NW = PM / 16;
        const int reff = chunks_of(nrows, rd);
        if (reff == 0) return;
        // t0 is a multiple of 16: the cell's first chunk; a chunk and phase = 64 lanes x PM / 4 contiguous bytes.  Rows of the
        // last chunk past the cell's end are another cell's (or, past the index, the padding of the last chunk): masked later
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(image + (size_t)t0 * M), 0, -1, 0x00020000);
        const unsigned lane_at = (unsigned)((g * 16 + r) * (PM / 4));
        const unsigned first = ((unsigned)rd * (unsigned)(ROUND / 16) + (unsigned)wv) * (unsigned)(16 * M) + (unsigned)(16 * 32 * p);
#pragma unroll
        for (int c = 0; c < R; ++c) {
            if (c < reff) {                                    // wave-uniform
                const unsigned so = first + (unsigned)(c * GW * 16 * M);
                if constexpr (NW == 2) {
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_at, so, 0);
                    w[c][0] = v.x; w[c][1] = v.y;
                } else {
                    w[c][0] = __builtin_amdgcn_raw_buffer_load_b32(rs, lane_at, so, 0);
                }
            }
        }
    };
    adc_i32x4v bsel = {0, 0, 0, 0};                          // B[k][j = r] = [k % 8 == r]
    if (r < 8) {
        const int one = 1 << (8 * (r & 3));
        bsel[r >> 2] = one;
        bsel[2 + (r >> 2)] = one;
    }
    const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(smem));
    if (lds0 & 0xFFFFu) __builtin_trap();                    // the one-instruction gather address needs 64 KiB-aligned table buffers
    adc_i32x4v acc[R];
    // ---- gathers + folds of one stage
    auto gathers = [&](auto PMc, bool first, const unsigned (&w)[R][2], unsigned bufoff, int reff) {
        constexpr int PM = decltype(PMc)::value;
        constexpr int STEPS = PM / 4;
        unsigned off[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            int slot, m;
            adc_cf_step(PM, s, r, g, slot, m);
            off[s] = lds0 + bufoff + (unsigned)slot * 8u;
        }
        // units of 4 gathers (half a chunk of a 32-phase, a chunk of a 16-phase) = 2 MFMAs; the gathers of the next unit are
        // issued before the MFMAs of the current one (8 gathers per wave in flight; 16 did not fit the 128 registers of 4 waves/SIMD)
        constexpr int UPC = STEPS / 4;
        uint2 ea[4], eb[4];
        auto gather = [&](int c, int hh, uint2 (&e)[4]) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                // buffer base (0 / 64 KiB: bytes 2-3) | code << 8 | slot offset (< 256): one v_perm_b32 (see the 16-query screen)
                const unsigned addr = __builtin_amdgcn_perm(w[c][hh], off[4 * hh + s4], 0x03020000u | ((4u + (unsigned)s4) << 8));
                typedef unsigned adc_u32x2 __attribute__((ext_vector_type(2)));
                const adc_u32x2 v = *reinterpret_cast<const adc_u32x2 __attribute__((address_space(3)))*>(addr);
                e[s4] = make_uint2(v.x, v.y);
            }
        };
        auto fold = [&](int c, int hh, const uint2 (&e)[4]) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const adc_i32x4v a = {(int)e[2 * s2].x, (int)e[2 * s2].y, (int)e[2 * s2 + 1].x, (int)e[2 * s2 + 1].y};
                if (hh == 0 && s2 == 0 && first) acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bsel, adc_i32x4v{0, 0, 0, 0}, 0, 0, 0);
                else acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bsel, acc[c], 0, 0, 0);
            }
        };
        if (reff <= 0) return;                                // wave-uniform
        gather(0, 0, ea);
#pragma unroll
        for (int c = 0; c < R; ++c) {
            if (c < reff) {                                   // wave-uniform
                ivfs_prio_at<R>(c);
                if constexpr (UPC == 2) {
                    __builtin_amdgcn_sched_barrier(0);
                    gather(c, 1, eb);
                    __builtin_amdgcn_sched_barrier(0);
                    fold(c, 0, ea);
                    __builtin_amdgcn_sched_barrier(0);
                    if (c + 1 < R && c + 1 < reff) gather(c + 1, 0, ea);
                    __builtin_amdgcn_sched_barrier(0);
                    fold(c, 1, eb);
                } else {
                    __builtin_amdgcn_sched_barrier(0);
                    if (c + 1 < R && c + 1 < reff) gather(c + 1, 0, (c & 1) ? ea : eb);
                    __builtin_amdgcn_sched_barrier(0);
                    fold(c, 0, (c & 1) ? eb : ea);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        ivfs_prio_done();
    };
    // ---- survivors: (query, row) pairs appended to the wave's own stream (ivfs_survivors); 8 query columns here
    const __amdgpu_buffer_rsrc_t strsrc = ivfs_stream_rsrc(stream, stream_cap, wv);
    unsigned woff = 0;                                        // wave-uniform: pairs in the wave's stream

    // ---- prologue: every thread helps with the first tables
    const ivfs_task first = load_task(0);
    if (!first.valid) return;                                 // block-uniform
    using P0 = std::integral_constant<int, ivfs_pm(M, 0)>;
    {
        unsigned dd[DD][8];
        load_tables(P0{}, 0, first, dd);
        write_tables(P0{}, dd, 0u);
    }
    // ---- the walk over (task, round, phase) stages, once per role: a loader wave runs its own copy of the loop — it meets the
    // gathering waves at every barrier but never holds their sums / codes (as one loop with a branch per stage, the compiler
    // keeps those 60 registers live through the loader's branch and spills 300 bytes per lane)
    auto walk = [&](auto ROLEc) {
        constexpr bool LOADER = decltype(ROLEc)::value == 1;
        ivfs_task cur = first;
        int myq = -1, tq = INT_MAX;
        unsigned w[R][2];
        if constexpr (!LOADER) {
            myq = lane_q(cur); tq = ivfs_lane_thr<M>(tint, myq);
            load_codes(P0{}, 0, cur.rows.t0, cur.rows.nrows, 0, w);
        }
        unsigned bufoff = 0;
        unsigned k = 0;
        for (;;) {                                            // tasks of this block
            const ivfs_task nxt = load_task(k + 1);           // used in this task's LAST stage (and for its thresholds after)
            const int nrounds = ivfs_rounds_of<ROUND>(cur.rows);
            for (int rd = 0; rd < nrounds; ++rd) {
                const bool more = rd + 1 < nrounds;           // block-uniform
                auto stage = [&](auto Pc) {
                    constexpr int P = decltype(Pc)::value;
                    constexpr bool LASTP = (P == NPH - 1);
                    constexpr int PN = LASTP ? 0 : P + 1;     // phase of the next stage
                    using PMc = std::integral_constant<int, ivfs_pm(M, P)>;
                    using PMn = std::integral_constant<int, ivfs_pm(M, PN)>;
                    IVFS_TSTAMP(3);                               // arrival at the barrier that ends the previous stage
                    ivfs_block_sync();
                    IVFS_TSTAMP(0);
                    // the next stage: same task (next phase / next round) or the next task's first
                    const bool to_next = LASTP && !more;      // block-uniform
                    const bool has_next = !to_next || nxt.valid;
                    ivfs_task nd;
#pragma unroll
                    for (int j = 0; j < 8; ++j) nd.qid[j] = to_next ? nxt.qid[j] : cur.qid[j];
                    nd.rows.t0 = to_next ? nxt.rows.t0 : cur.rows.t0;
                    nd.rows.nrows = to_next ? nxt.rows.nrows : cur.rows.nrows;
                    const int nrd = to_next ? 0 : (LASTP ? rd + 1 : rd);
                    if constexpr (LOADER) {
                        if (has_next) loader_fill(PMn{}, PN, nd, bufoff ^ (unsigned)IVFS_BUF);
                    } else {
                        const int reff = chunks_of(cur.rows.nrows, rd);
                        gathers(PMc{}, P == 0, w, bufoff, reff);
                        IVFS_TSTAMP(1);
                        // the codes of the next stage go into the registers the gathers just released (last phase: after the
                        // survivor pass, whose few waits would otherwise also wait for them)
                        if constexpr (LASTP)
                            ivfs_survivors<R, GW, 8>(acc, cur.rows, rd, tq, myq, reff, wv, l, stream_cap, status, strsrc, woff);
                        if (has_next) load_codes(PMn{}, PN, nd.rows.t0, nd.rows.nrows, nrd, w);
                    }
                    IVFS_TSTAMP(2);
                    bufoff ^= (unsigned)IVFS_BUF;
                };
                stage(std::integral_constant<int, 0>{});
                if constexpr (NPH > 1) stage(std::integral_constant<int, 1>{});
                if constexpr (NPH > 2) stage(std::integral_constant<int, 2>{});
            }
            if (!nxt.valid) break;
            cur = nxt;
            if constexpr (!LOADER) { myq = lane_q(cur); tq = ivfs_lane_thr<M>(tint, myq); }
            ++k;
        }
    };
    if (wv >= GW) {                                           // wave-uniform
        walk(std::integral_constant<int, 1>{});
        return;                                               // (its stream stays empty: stream_cnt was cleared by the host)
    }
    walk(std::integral_constant<int, 0>{});
    if (l == 0) stream_cnt[blockIdx.x * IVFS_WAVES + (unsigned)wv] = woff;
}
