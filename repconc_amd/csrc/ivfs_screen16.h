// 16-query form of the pipelined IVF screen (round 6; included by ivf_lists.hip; what it shares with the 8-query form,
// ivfs_screen8.h, is ivfs_common.h).
//
// The 8-query screen (ivfs_screen_kernel) gathers with ds_read_b64: 8 queries per gather at ~5 cycles per gather in the real
// kernel, and its loader waves need as long for a 64 KiB table phase (2.4-3.1 us) as the twelve gathering waves for its
// gathers (2.1 us + 0.7 us of code loads; profiles/r03g_ivf_timeline.txt).  With whole-query-set calls a probed cell is
// shared by tens of queries (6 980 queries x nprobe 32 / 5000 cells = 45), so the flat search's 16-query gather applies:
// tables [code][16 slots][16 queries] (a code's row = 256 B = all 64 banks once, conflict-free whatever the codes), phases of
// 16 sub-quantisers (64 KiB), ONE ds_read_b128 + ONE i8 MFMA per (16 rows, 4 sub-quantisers, 16 queries).  Per query a task
// moves the same table bytes as before and issues half the gathers.
//   * tasks hold up to 16 queries (ivf_plan_*_kernel with width 16); the queries of a task are read from sorted_q when needed
//     (the loader's 16 table offsets, the gathering lanes' own column) instead of living in 2 x 16 scalar registers;
//   * image: chunk n / 16 holds [phase p16][lane = (n mod 16) + 16 g][step j] = codes[n][16 p16 + slot(lane, j)]
//     (adc_q16_slot): a wave's code load for one chunk and phase is 64 lanes x 4 B = 256 contiguous bytes;
//   * tables: a loader thread takes item (code c, quad u): one dword (4 sub-quantisers) from each of the 16 queries' byte tables
//     (consecutive lanes = consecutive dwords), byte-transposes them with v_perm_b32 into the four 16-byte entries
//     (c, 4 u .. 4 u + 3) and stores them with ds_write_b128.  A wave-instruction of b128 stores is served 8 lanes at a time over a
//     128-byte window, and a code's row is 256 B: lanes that stored "entry i of my item" together would hit two windows' worth of
//     banks four times over.  Lane l therefore stores entry (j + (l >> 1)) mod 4 in step j — eight distinct 16-byte slots per
//     group — and gets that rotation for free: the selector of the first transposition step is a per-lane register.
#include "ivfs_common.h"

#define IVFS16_R 10              // chunks of 16 rows per gathering wave and round
typedef unsigned adc_u32x4s __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t ivfs16_image_at(int M, int64_t n, int p16, int g, int j) {
    return (n >> 4) * (int64_t)(16 * M) + (int64_t)(256 * p16) + (int64_t)((((int)(n & 15)) + 16 * g) * 4 + j);
}
__global__ __launch_bounds__(256) void ivfs16_image_kernel(const uint8_t* __restrict__ codes, int64_t n0, int64_t cnt, int M,
                                                           uint8_t* __restrict__ image) {
    const int64_t total = cnt * M;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t n = n0 + i / M;
        const int pos = (int)(i % M);
        const int p16 = pos >> 4, g = (pos >> 2) & 3, j = pos & 3;
        const int m = 16 * p16 + adc_q16_slot((int)(n & 15) + 16 * g, j);
        image[ivfs16_image_at(M, n, p16, g, j)] = codes[n * M + m];
    }
}
// The same image read the other way, in 16-byte pieces (adc_select.h): a chunk of 16 rows owns 16 M contiguous bytes, phases of
// 256 bytes, [lane][step]; piece o = (chunk o / M of the block, piece o % M = four lanes of a phase)
struct adc_sel_rows16 {
    __host__ __device__ static int64_t dest(int M, int64_t i0, int o) {
        return ((i0 >> 4) + o / M) * (int64_t)(16 * M) + (int64_t)(o % M) * 16;
    }
    __host__ __device__ static void src(int M, int o, int b, int& row, int& m) {
        const int w = o % M, lane = 4 * (w & 15) + (b >> 2);
        row = 16 * (o / M) + (lane & 15);
        m = 16 * (w >> 4) + adc_q16_slot(lane, b & 3);
    }
};

// Development aid (tools/ivf16_timeline.py builds a variant library with -DRC_IVF_TRACE): wall-clock stamps of every wave at
// three points of each of a block's first 64 stages.  Off in the shipped library.
#ifdef RC_IVF_TRACE
__device__ unsigned long long ivfs16_trace[256 * 64 * 16 * 4];
extern "C" int rc_debug_ivfs16_trace(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ivfs16_trace), sizeof(ivfs16_trace));
}
#define IVFS16_TSTAMP(stage, i)                                                                                          \
    do {                                                                                                                 \
        if (l == 0 && (stage) < 64u && blockIdx.x < 256u)                                                                 \
            ivfs16_trace[((blockIdx.x * 64u + (stage)) * 16u + (unsigned)wv) * 4u + (i)] = wall_clock64();               \
    } while (0)
#else
#define IVFS16_TSTAMP(stage, i) do { } while (0)
#endif

struct ivfs_task16 {
    int valid;
    int qs, qc;               // the task's queries: sorted_q[qs .. qs + qc), 1 <= qc <= 16
    ivfs_rows rows;
};

template <int M, int LW>
__global__ __launch_bounds__(IVFS_THREADS, 4) void ivfs_screen16_kernel(const uint8_t* __restrict__ image,
                                                                        const int* __restrict__ tint,
                                                                        unsigned* __restrict__ stream_cnt,
                                                                        unsigned* __restrict__ stream, unsigned stream_cap,
                                                                        int* __restrict__ status, adc_ivf_tasks T,
                                                                        int ntasks_arg) {
    static_assert(LW > 0 && M % 16 == 0, "loader waves; whole phases of 16 sub-quantisers");
    constexpr int GW = IVFS_WAVES - LW;                       // gathering waves
    constexpr int R = IVFS16_R;
    constexpr int NPH = M / 16, ROUND = GW * R * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned tid = threadIdx.x;
    const int l = (int)(tid & 63u), wv = __builtin_amdgcn_readfirstlane((int)(tid >> 6)), r = l & 15;
    const ivfs_share share = ivfs_block_share(T, ntasks_arg);
    auto load_task = [&](unsigned k) {
        ivfs_task16 d;
        unsigned task;
        d.valid = ivfs_share_task(share, k, task) ? 1 : 0;
        d.qs = 0; d.qc = 0;
        d.rows = ivfs_rows{0u, 0u, 0u};
        if (d.valid) {
            d.qs = ivfs_sc(T.task_qstart[task]);
            d.qc = ivfs_sc(T.task_qcnt[task]);
            d.rows = ivfs_cell_rows(T, ivfs_sc(T.task_list[task]), d.qc);
        }
        return d;
    };
    auto lane_q = [&](const ivfs_task16& d) { return (r < d.qc) ? T.sorted_q[d.qs + r] : -1; };
    // ---- tables: phase p16 of a task, in two halves (request, then transpose and store) so that a loader
    // can request a phase one stage before it transposes it (the loads' ~1 us from the L2 / memory-side cache is then nobody's
    // critical path: with request, wait, transposition and stores inside one stage the four loader waves needed ~3 us per 64 KiB
    // phase and set the stage period — the 16-query gathers, half as many per query, gained 2 %)
    const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)T.qbyte, 0, -1, 0x00020000);
    const unsigned rot = ((unsigned)l >> 1) & 3u;
    // the task's 16 table offsets: lane j < 16 reads query j's id, the wave reads them back lane by lane
    // (an empty slot reads query 0's table: its column is masked by the threshold INT_MAX)
    auto task_offsets = [&](const ivfs_task16& d, unsigned (&so)[16]) {
        int qv = 0;
        if (l < 16 && l < d.qc) qv = T.sorted_q[d.qs + l];
#pragma unroll
        for (int j = 0; j < 16; ++j) so[j] = (unsigned)__builtin_amdgcn_readlane(qv, j) * (unsigned)(M * RC_K);
    };
    // The prologue's form (all 1024 threads): thread = item (code c, quad u), one dword per query
    auto fill_load = [&](int p16, const unsigned (&so)[16], unsigned (&a)[16]) {
        const int y = p16 >> 1, hh = p16 & 1;
        const unsigned PM = (unsigned)ivfs_pm(M, y);          // the byte tables are stored in phases of 32 (last one: 16)
        const unsigned c = tid >> 2, u = tid & 3u;
        const unsigned voff = (unsigned)(RC_K * 32 * y) + c * PM + 16u * (unsigned)hh + 4u * u;
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = __builtin_amdgcn_raw_buffer_load_b32(qrsrc, voff, so[j], 0);
    };
    auto fill_store = [&](unsigned bufoff, const unsigned (&a)[16]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned i = ((unsigned)j + rot) & 3u;                      // the entry this lane stores in step j
            const unsigned sel = ((4u + i) << 8) | i;                        // (a_even.b_i, a_odd.b_i, -, -)
            adc_u32x4s e;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const unsigned p01 = __builtin_amdgcn_perm(a[4 * gq + 1], a[4 * gq], sel);
                const unsigned p23 = __builtin_amdgcn_perm(a[4 * gq + 3], a[4 * gq + 2], sel);
                e[gq] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);      // queries 4 gq .. 4 gq + 3 of entry (c, 4 u + i)
            }
            *reinterpret_cast<adc_u32x4s*>(smem + (bufoff + tid * 64u + i * 16u)) = e;
        }
    };
    // The loader waves' form (256 threads): thread = code c, all four quads in ONE 16-byte load per query — 16 load instructions per
    // thread and phase instead of 64.  The wall-clock trace (tools/ivf16_timeline.py, profiles/r06j_ivf16_timeline.txt) showed the
    // loader waves as the stage's critical path: 1.3 us transposing and storing + 1.5 us ISSUING the 64 dword requests of the next
    // phase, against 2.2-2.5 us of gathers + hand-over.  The price: a thread's sixteen entries are one whole 256-byte row, so the
    // eight lanes of a store group can only be spread over FOUR distinct 16-byte slots (rotation l & 3 of the entry inside its quad):
    // two-way bank conflicts on the 16 stores, 256 instead of 128 LDS cycles per wave and phase.
    // (Requesting the phase in two 8-byte halves — the half just stored frees its registers for the same half of the phase after
    // next, so the first request leaves a quarter into the loader's stage — was built and is SLOWER: 32 load instructions per
    // thread cost the loader 1.2-1.4 us of issue against 0.6 for 16, 6.6 ms against 4.1 per 6 980-query search at nprobe 128
    // (profiles/r06j_ivf16_timeline_half_sets.txt).  The loader waves stay the stage's critical path at ~2.9 us in the traced build:
    // ~0.8 us waiting for the phase requested at the end of the previous stage, 1.1 us transposing and storing, 0.6 us requesting.)
    typedef unsigned adc_u32x4l __attribute__((ext_vector_type(4)));
    auto fill_load4 = [&](int p16, const unsigned (&so)[16], unsigned c, adc_u32x4l (&a)[16]) {
        const int y = p16 >> 1, hh = p16 & 1;
        const unsigned PM = (unsigned)ivfs_pm(M, y);
        const unsigned voff = (unsigned)(RC_K * 32 * y) + c * PM + 16u * (unsigned)hh;
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = __builtin_amdgcn_raw_buffer_load_b128(qrsrc, voff, so[j], 0);
    };
    auto fill_store4 = [&](unsigned bufoff, unsigned c, const adc_u32x4l (&a)[16]) {
        const unsigned rot4 = (unsigned)l & 3u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned i = ((unsigned)j + rot4) & 3u;
                const unsigned sel = ((4u + i) << 8) | i;
                adc_u32x4s e;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const unsigned p01 = __builtin_amdgcn_perm(a[4 * gq + 1][u], a[4 * gq][u], sel);
                    const unsigned p23 = __builtin_amdgcn_perm(a[4 * gq + 3][u], a[4 * gq + 2][u], sel);
                    e[gq] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
                }
                *reinterpret_cast<adc_u32x4s*>(smem + (bufoff + c * 256u + (unsigned)(4 * u) * 16u + i * 16u)) = e;
            }
        }
    };
    // ---- codes of one stage: the wave's chunks of the round (ivfs_chunks_of); one dword per lane and chunk
    auto chunks_of = [&](unsigned nrows, int rd) { return ivfs_chunks_of<GW, R>(nrows, rd, wv); };
    auto load_codes = [&](int p16, unsigned t0, unsigned nrows, int rd, unsigned (&w)[R]) {
        const int reff = chunks_of(nrows, rd);
        if (reff == 0) return;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(image + (size_t)t0 * M), 0, -1, 0x00020000);
        const unsigned first = ((unsigned)rd * (unsigned)(ROUND / 16) + (unsigned)wv) * (unsigned)(16 * M) + (unsigned)(256 * p16);
#pragma unroll
        for (int c = 0; c < R; ++c)
            if (c < reff) w[c] = __builtin_amdgcn_raw_buffer_load_b32(rs, (unsigned)l * 4u, first + (unsigned)(c * GW * 16 * M), 0);
    };
    adc_i32x4v bsel = {0, 0, 0, 0};                          // B[k][n = r] = [k mod 16 == r]
    bsel[r >> 2] = 1 << (8 * (r & 3));
    const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(smem));
    if (lds0 & 0xFFFFu) __builtin_trap();                    // the one-instruction gather address needs 64 KiB-aligned table buffers
    unsigned off[4];                                          // this lane's slot addresses in the CURRENT table buffer (bit 16 toggles)
#pragma unroll
    for (int j = 0; j < 4; ++j) off[j] = lds0 + (unsigned)adc_q16_slot(l, j) * 16u;
    adc_i32x4v acc[R];
    // ---- gathers + folds of one stage: the four gathers of chunk c + 1 are issued before the four MFMAs of chunk c
    auto gathers = [&](bool first, const unsigned (&w)[R], int reff) {
        if (reff <= 0) return;                                // wave-uniform
        adc_u32x4s ea[4], eb[4];
        auto gather = [&](int c, adc_u32x4s (&e)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // buffer base (0 / 64 KiB: bytes 2-3) | code << 8 | slot offset (< 256): one v_perm_b32
                const unsigned addr = __builtin_amdgcn_perm(w[c], off[j], 0x03020000u | ((4u + (unsigned)j) << 8));
                e[j] = *reinterpret_cast<const adc_u32x4s __attribute__((address_space(3)))*>(addr);
            }
        };
        auto fold = [&](int c, const adc_u32x4s (&e)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const adc_i32x4v a = {(int)e[j][0], (int)e[j][1], (int)e[j][2], (int)e[j][3]};
                if (j == 0 && first) acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bsel, adc_i32x4v{0, 0, 0, 0}, 0, 0, 0);
                else acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bsel, acc[c], 0, 0, 0);
            }
        };
        gather(0, ea);
#pragma unroll
        for (int c = 0; c < R; ++c) {
            if (c < reff) {                                   // wave-uniform
                ivfs_prio_at<R>(c);
                __builtin_amdgcn_sched_barrier(0);
                if (c + 1 < R && c + 1 < reff) gather(c + 1, (c & 1) ? ea : eb);
                __builtin_amdgcn_sched_barrier(0);
                fold(c, (c & 1) ? eb : ea);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        ivfs_prio_done();
    };
    // ---- survivors: (query, row) pairs appended to the wave's own stream (ivfs_survivors); 16 query columns here
    const __amdgpu_buffer_rsrc_t strsrc = ivfs_stream_rsrc(stream, stream_cap, wv);
    unsigned woff = 0;                                        // wave-uniform: pairs in the wave's stream

    // ---- prologue: every thread takes one item of the first tables
    const ivfs_task16 first = load_task(0);
    if (!first.valid) return;                                 // block-uniform
    {
        unsigned so[16], a0[16];
        task_offsets(first, so);
        fill_load(0, so, a0);
        fill_store(0u, a0);
    }
    // ---- loader waves: their own walk over the stages, two stages ahead with the requests, one with the stores.  Exactly one
    // barrier per stage, as the gathering waves.
    if (wv >= GW) {                                           // wave-uniform
        static_assert(LW * 64 == RC_K, "one loader thread per code");
        const unsigned lt = tid - (unsigned)(GW * 64);
        struct pos { ivfs_task16 d; unsigned k; int rd, P; };
        auto next = [&](const pos& p) {
            pos n = p;
            if (!p.d.valid) return n;
            if (++n.P == NPH) {
                n.P = 0;
                if (++n.rd == ivfs_rounds_of<ROUND>(p.d.rows)) { n.rd = 0; n.k = p.k + 1; n.d = load_task(n.k); }
            }
            return n;
        };
        unsigned so[16];
        adc_u32x4l a[16];
        unsigned so_k = 0xFFFFFFFFu;                          // the task `so` belongs to
        auto request = [&](const pos& p) {
            if (p.k != so_k) { task_offsets(p.d, so); so_k = p.k; }
            fill_load4(p.P, so, lt, a);
        };
        pos p1 = next(pos{first, 0u, 0, 0});                   // the stage AFTER the one that is about to run
        if (p1.d.valid) request(p1);
        unsigned bufoff = (unsigned)IVFS_BUF;                   // where p1's tables go
        unsigned sidx = 0;                                    // stage counter (trace builds only)
        (void)sidx;
        for (;;) {
            ivfs_block_sync();                                // a stage begins: everybody is done with the other buffer
            IVFS16_TSTAMP(sidx, 0);
            if (!p1.d.valid) break;
            fill_store4(bufoff, lt, a);
            IVFS16_TSTAMP(sidx, 1);
            p1 = next(p1);
            if (p1.d.valid) request(p1);
            IVFS16_TSTAMP(sidx, 2);
            bufoff ^= (unsigned)IVFS_BUF;
            ++sidx;
        }
        return;                                               // (its stream stays empty: stream_cnt was cleared by the host)
    }
    // ---- the gathering waves' walk over (task, round, phase) stages
    ivfs_task16 cur = first;
    int myq = lane_q(cur), tq = ivfs_lane_thr<M>(tint, myq);
    unsigned w[R];
    load_codes(0, cur.rows.t0, cur.rows.nrows, 0, w);
    unsigned k = 0;
    unsigned sidx = 0;                                        // stage counter (trace builds only)
    (void)sidx;
    for (;;) {                                                // tasks of this block
        const ivfs_task16 nxt = load_task(k + 1);
        const int nrounds = ivfs_rounds_of<ROUND>(cur.rows);
        for (int rd = 0; rd < nrounds; ++rd) {
            const bool more = rd + 1 < nrounds;               // block-uniform
            auto stage = [&](auto Pc) {
                constexpr int P = decltype(Pc)::value;
                constexpr bool LASTP = (P == NPH - 1);
                constexpr int PN = LASTP ? 0 : P + 1;         // phase of the next stage
                ivfs_block_sync();
                IVFS16_TSTAMP(sidx, 0);
                const bool to_next = LASTP && !more;          // block-uniform
                const bool has_next = !to_next || nxt.valid;
                const ivfs_task16 nd = to_next ? nxt : cur;
                const int nrd = to_next ? 0 : (LASTP ? rd + 1 : rd);
                {
                    // the codes of the NEXT stage are requested before this stage's gathers, into a second set of ten
                    // registers (the 8-query screen needs twenty per set and requests them after its last gather: every
                    // stage then begins by waiting 0.7-1 us for them, profiles/r03g_ivf_timeline.txt)
                    const int reff = chunks_of(cur.rows.nrows, rd);
                    unsigned wn[R];
                    if (has_next) load_codes(PN, nd.rows.t0, nd.rows.nrows, nrd, wn);
                    gathers(P == 0, w, reff);
                    IVFS16_TSTAMP(sidx, 1);
                    if constexpr (LASTP)
                        ivfs_survivors<R, GW, 16>(acc, cur.rows, rd, tq, myq, reff, wv, l, stream_cap, status, strsrc, woff);
                    if (has_next) {
#pragma unroll
                        for (int c = 0; c < R; ++c) w[c] = wn[c];
                    }
                    IVFS16_TSTAMP(sidx, 2);
                    ++sidx;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) off[j] ^= (unsigned)IVFS_BUF;     // the other table buffer (64 KiB-aligned bases)
            };
            stage(std::integral_constant<int, 0>{});
            if constexpr (NPH > 1) stage(std::integral_constant<int, 1>{});
            if constexpr (NPH > 2) stage(std::integral_constant<int, 2>{});
            if constexpr (NPH > 3) stage(std::integral_constant<int, 3>{});
            if constexpr (NPH > 4) stage(std::integral_constant<int, 4>{});
            if constexpr (NPH > 5) stage(std::integral_constant<int, 5>{});
            static_assert(NPH <= 6, "M <= 96");
        }
        if (!nxt.valid) break;
        cur = nxt;
        myq = lane_q(cur); tq = ivfs_lane_thr<M>(tint, myq);
        ++k;
    }
    if (l == 0) stream_cnt[blockIdx.x * IVFS_WAVES + (unsigned)wv] = woff;
}
