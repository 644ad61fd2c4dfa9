// Exact IVF search over dense rows (faiss.IndexIVFFlat): the rows of a dense store are kept list-major (sorted by coarse cell)
// and a query is scored, with the chain of the flat dense searches bit for bit, against the rows of its probed cells only.
//
// Score of a (query, row) pair: one fp32 accumulator from +0.0f, d ascending, dense_chain_step<L2> over the values widened to
// fp32 (inner product: s = fmaf(q_d, x_d, s); L2: t = q_d - x_d, s = fmaf(t, t, s)).  Every stage works on s, or on -d for L2,
// and dense_l2_launch_negate turns the k output values into distances at the end.
//
// Stages, all on the caller's stream, no host synchronisation:
//   1. ivf_flat_plan_query_kernel   per query: base[q][p] = rows of its probes before probe p, count[q] = all of them; counts
//                                   the queries probing every cell
//   2. ivf_plan_cells / _scatter / _tasks_kernel (ivf_plan.h, shared with the PQ search): tasks of up to IVFF_QG queries of
//                                   one cell
//   3. ivf_flat_scan_kernel         the scan below: dense[q][base[q][p] + r] = s, rowid[..] = the row
//   4. ivf_kth_kernel, ivf_filter_kernel (ivf_select.h, shared with rc_ivf_search), rc_adc_launch_select: the exact k-th
//                                   largest score per query, the keys adc_exact_key(s, ids[row]) at or above it, sort + emit.
//                                   More than ADC_CAND_CAP rows tied at the k-th score: status / qstatus bit 1.
//   5. L2: the negation.
//
// The scan is list-centric.  At 8.84 M x 768 rows in 5000 cells, 1200 queries and nprobe 32 a probed cell is shared by ~8
// queries of the call and nearly every cell is probed: scanning per query would read the store eight times, scanning per cell
// reads it at most once per group of IVFF_QG queries.  The pair work is vector-ALU work (the chain's order leaves one
// accumulator per pair; the matrix cores' 16- and 32-wide tiles would be mostly padding at 8 queries per cell).
//
// ivf_flat_scan_kernel: block (task, y) = (cell, <= 8 queries probing it), row chunks y, y + gridDim.y, .. of IVFF_RT = 512
// rows, so a long cell is spread over gridDim.y blocks.  256 threads: thread (tx = tid % 128, ty = tid / 128) owns rows
// 4 tx .. + 3 of the chunk and queries 4 ty .. + 3 of the task, 16 accumulators that each walk d ascending.  D is walked in
// chunks of IVFF_KC = 16 through LDS, double buffered: the loaders read every row's slice of 16 values with 16-byte loads (a row's
// slice is 64 (fp32) / 32 (fp16) contiguous bytes, consecutive lanes take consecutive pieces) into registers while the previous
// chunk is computed, then store them k-major as fp32 (row pitch 516 words: 4 k apart is 16 banks apart); the task's 8 query
// slices are staged beside them, k-major.  Per k a thread reads one 16-byte vector of row values (128 lanes: 2 KiB contiguous)
// and one of query values (uniform over the wave: a broadcast) for 16 chain steps.  The query values are staged per K chunk,
// not once per task: any D fits.  The last, partial K chunk runs a loop of D mod 16 steps: no padding enters a chain.
// PAD: rows that are not 16-byte aligned (or a D that is no multiple of 16 bytes) are read element by element into the same
// registers; the arithmetic is the same.  Rows past the cell's end in the last chunk repeat its last row and are not written.
//   LDS: 2 x 16 x 516 x 4 + 2 x 16 x 8 x 4 = 67 072 bytes, two blocks per CU.
// T = signed char, TQ = float (rc_ivf_flat_sq8_search; faiss.IndexIVFScalarQuantizer, QT_8bit): the same scan over a list-major
// store of 8-bit scalar-quantiser codes, fp32 queries.  A code is decoded once, fmaf((float)c', step_d, mid_d) (dense_sq8.h), on
// its way from the staged registers into the same fp32 tile: the chains, and so the score bits, are those of the fp32 scan over
// the decoded rows under either metric.  Same LDS, same plan, same selection.
// RES (rc_ivf_flat_sq8r_search; faiss.IndexIVFScalarQuantizer, QT_8bit, by_residual = true): the codes are those of the row minus
// the centroid of its cell, and a stored value is x^ = fp32(fmaf((float)c', step_d, mid_d) + coarse[cell][d]): the decode, then
// ONE separate fp32 addition (two roundings) on the way into the tile.  A task is one cell, so the 16 centroid values of a
// stage are uniform over the block, as step and mid are.
#include "dense_l2.h"
#include "dense_sq8.h"
#include "ivf_plan.h"
#include "ivf_select.h"
#include <type_traits>

#define IVFF_QG 8                                        // queries per task
#define IVFF_RT 512                                      // rows per chunk
#define IVFF_KC 16                                       // values of a row per stage
#define IVFF_XLD (IVFF_RT + 4)                           // words per k of the row tile
#define IVFF_MAX_NLIST 16384
#define IVFF_Y_MAX 8                                     // blocks a cell's row chunks are dealt to

typedef unsigned ivff_u4 __attribute__((ext_vector_type(4)));

// One block per query: base of every probe in the query's score row, the total, the queries probing every cell.  A probe
// outside [0, nlist) or a total above `stride` (a caller's error) scans nothing of that probe / clamps and sets status bit 2.
__global__ __launch_bounds__(256) void ivf_flat_plan_query_kernel(const int64_t* __restrict__ list_off, const int* __restrict__ probes,
                                                                  int nprobe, int nlist, int64_t stride, int* __restrict__ base,
                                                                  int* __restrict__ count, int* __restrict__ per_cell,
                                                                  int* __restrict__ status) {
    __shared__ int s_wave[4];
    const int qi = blockIdx.x, tid = threadIdx.x;
    int64_t carry = 0;
    bool bad = false;
    for (int b0 = 0; b0 < nprobe; b0 += 256) {                // block-uniform
        const int p = b0 + tid;
        int size = 0;
        if (p < nprobe) {
            const int c = probes[(size_t)qi * nprobe + p];
            if (c >= 0 && c < nlist) {
                const int64_t n = list_off[c + 1] - list_off[c];
                size = (n > 0 && n <= stride && n <= 0x7FFFFFFFll) ? (int)n : 0;
                bad |= n < 0 || n > stride;
                atomicAdd(per_cell + c, 1);
            } else {
                bad = true;
            }
        }
        int total;
        const int ex = ivfp_block_scan256(size, s_wave, total);
        // past `stride` nothing is written by the scan (it tests every position): the base only has to be an int
        if (p < nprobe) base[(size_t)qi * nprobe + p] = (int)((carry + ex) > 0x7FFFFFFFll ? 0x7FFFFFFFll : carry + ex);
        carry += (unsigned)total;
    }
    if (tid == 0) {
        if (carry > stride) { carry = stride; bad = true; }
        count[qi] = (int)(carry > 0x7FFFFFFFll ? 0x7FFFFFFFll : carry);
    }
    if (bad) atomicOr(status, 4);
}

// The scan's body.  T: the stored type, TQ: the queries' (T itself for the fp32 and fp16 stores).  T = signed char is the coded
// form: rows of 8-bit scalar-quantiser codes c' = c - 128 (dense_sq8.h), fp32 queries that are not rounded, dec = [step | mid].
// A value is decoded once per (row, d), on its way from the staged registers into the fp32 tile, so the compute loop and the
// LDS tile are those of the other stores and the 16 chains see fmaf((float)c', step_d, mid_d).  A row's slice of a stage is
// ONE 16-byte piece there (P = 1): the 64 lanes of a load touch 64 rows, and the seven later stages of a row's 128-byte line
// are served by the caches.  Holding the slices of 2 or 4 stages in registers (one wider fetch per lane every 2 or 4 stages)
// was measured and is slower at every nprobe (profiles/ivf_flat_sq8_form_ab.txt); this form is the one kept.
// RES (coded form only): coarse [nlist][ldc] fp32, the centroid of the task's cell is added to every decoded value.
// MAP (the subset search): the scan runs over the virtual store x' = x[rows].  rows [ns] int64 holds the store positions of the
// selected rows, strictly ascending (so grouped by cell, corpus id ascending inside a cell), and `list_off` is the caller's
// sel_off [nlist + 1]: the offsets of the cells INSIDE rows.  Logical row i of the task's cell is read at x + rows[sel_off[c]
// + i] * ldx and rowid receives that store position, so everything after the scan (ids[rowid], the tie rule) is untouched.  A
// loader thread's NL row addresses are formed once per row chunk and held in registers over the chunk's K stages (rows[] is
// read once per (row, chunk), never per stage); the logical row of a partial last chunk is clamped BEFORE the map, so rows[] is
// never read at or past sel_off[c + 1].  !MAP never reads `rows` and forms its addresses as before.
template <typename T, typename TQ, bool L2, bool PAD, bool RES = false, bool MAP = false>
__device__ __forceinline__ void ivf_flat_scan_body(const T* __restrict__ x, int64_t ldx, const int64_t* __restrict__ list_off,
                                                   int D, const TQ* __restrict__ q, const float* __restrict__ dec,
                                                   const float* __restrict__ coarse, int64_t ldc,
                                                   const int* __restrict__ probes, const int* __restrict__ base, int nprobe,
                                                   int64_t stride, const int* __restrict__ task_list,
                                                   const int* __restrict__ task_qstart, const int* __restrict__ task_qcnt,
                                                   const int* __restrict__ sorted_q, float* __restrict__ dense,
                                                   int* __restrict__ rowid, const int64_t* __restrict__ rows) {
    constexpr bool SQ = std::is_same<T, signed char>::value;
    static_assert(SQ || !RES, "the residual form is a form of the coded scan");
    constexpr int EPP = 16 / (int)sizeof(T);                 // values per 16-byte piece
    constexpr int P = IVFF_KC / EPP;                         // pieces of a row's slice
    constexpr int NL = IVFF_RT * P / 256;                    // pieces per loader thread and stage
    __shared__ __attribute__((aligned(16))) float sx[2][IVFF_KC * IVFF_XLD];
    __shared__ __attribute__((aligned(16))) float sq[2][IVFF_KC * IVFF_QG];
    __shared__ int64_t s_qbase[IVFF_QG];                     // position of the cell's first row in the query's score row, or -1
    const int t = blockIdx.x, tid = threadIdx.x, tx = tid & 127, ty = tid >> 7;
    const int qc = task_qcnt[t];
    if (qc <= 0) return;                                      // a task past the device-side count (block-uniform)
    const int cell = task_list[t], qs = task_qstart[t];
    const int64_t c0 = list_off[cell], size = list_off[cell + 1] - c0;
    if ((int64_t)blockIdx.y * IVFF_RT >= size) return;       // block-uniform
    if (tid < IVFF_QG) {
        int64_t o = -1;
        if (tid < qc) {
            const int qi = sorted_q[qs + tid];
            const int* pr = probes + (size_t)qi * nprobe;
            int lo = 0, hi = nprobe - 1;                      // ascending distinct cells: the slot of `cell`
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pr[mid] < cell) lo = mid + 1; else hi = mid;
            }
            if (pr[lo] == cell) o = (int64_t)base[(size_t)qi * nprobe + lo];
        }
        s_qbase[tid] = o;
    }
    // the query loader: thread (g = tid / 16, kk = tid % 16) of the first 128 stages value k0 + kk of query g
    const int qg = tid >> 4, qk = tid & 15;
    const bool qload = tid < IVFF_QG * IVFF_KC;
    const TQ* qp = q + (int64_t)((qload && qg < qc) ? sorted_q[qs + qg] : sorted_q[qs]) * D;
    const int nkc = (D + IVFF_KC - 1) / IVFF_KC;
    const float* cp = RES ? coarse + (int64_t)cell * ldc : nullptr;      // the cell's centroid (block-uniform)
    for (int64_t ch = blockIdx.y; ch * IVFF_RT < size; ch += gridDim.y) {
        const int64_t r0 = c0 + ch * IVFF_RT;
        const int nrows = size - ch * IVFF_RT < IVFF_RT ? (int)(size - ch * IVFF_RT) : IVFF_RT;
        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][r] = 0.f;
        ivff_u4 stg[NL];
        float rq = 0.f;
        const T* xr[MAP ? NL : 1];                                  // MAP: the loader's rows of this chunk, mapped once
        if constexpr (MAP) {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int row = (j * 256 + tid) / P;
                xr[j] = x + rows[r0 + (row < nrows ? row : nrows - 1)] * ldx;
            }
        }
        float dstep[SQ ? IVFF_KC : 1], dmid[SQ ? IVFF_KC : 1];      // coded form: step and mid of the staged slice (wave-uniform)
        float dcen[RES ? IVFF_KC : 1];                              // residual form: the cell's centroid over the slice, likewise
        // piece i = j 256 + tid of the stage: row i / P of the chunk, piece i % P of its slice; whole pieces inside the row with
        // one 16-byte load, nothing past D (PAD: value by value)
        auto gload = [&](int kc) {
            const int k0 = kc * IVFF_KC;
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int i = j * 256 + tid, row = i / P, pc = i % P;
                const T* p = (MAP ? xr[j] : x + (r0 + (row < nrows ? row : nrows - 1)) * ldx) + k0 + pc * EPP;
                if constexpr (!PAD) {
                    stg[j] = (k0 + pc * EPP < D) ? *reinterpret_cast<const ivff_u4*>(p) : ivff_u4{0u, 0u, 0u, 0u};
                } else {
                    union { ivff_u4 v; T e[EPP]; } u;
                    u.v = ivff_u4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int e = 0; e < EPP; ++e)
                        if (k0 + pc * EPP + e < D) u.e[e] = p[e];
                    stg[j] = u.v;
                }
            }
            if constexpr (SQ) {
#pragma unroll
                for (int e = 0; e < IVFF_KC; ++e) {               // past D: the last dimension's, no chain reads the value
                    const int d = k0 + e < D ? k0 + e : D - 1;
                    dstep[e] = dec[d];
                    dmid[e] = dec[D + d];
                    if constexpr (RES) dcen[e] = cp[d];
                }
            }
            if (qload) rq = (qg < qc && k0 + qk < D) ? (float)qp[k0 + qk] : 0.f;
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int i = j * 256 + tid, row = i / P, pc = i % P;
                union { ivff_u4 v; T e[EPP]; } u;
                u.v = stg[j];
#pragma unroll
                for (int e = 0; e < EPP; ++e) {
                    if constexpr (RES)          // the decode's rounding, then the addition's: never one fused operation
                        sx[buf][(pc * EPP + e) * IVFF_XLD + row] =
                            dense_sq8_decode(u.e[e], dstep[pc * EPP + e], dmid[pc * EPP + e]) + dcen[pc * EPP + e];
                    else if constexpr (SQ)
                        sx[buf][(pc * EPP + e) * IVFF_XLD + row] = dense_sq8_decode(u.e[e], dstep[pc * EPP + e], dmid[pc * EPP + e]);
                    else
                        sx[buf][(pc * EPP + e) * IVFF_XLD + row] = (float)u.e[e];
                }
            }
            if (qload) sq[buf][qk * IVFF_QG + qg] = rq;
        };
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
            const int kn = D - kc * IVFF_KC;
            auto step = [&](int k) {
                const float4 xv = *reinterpret_cast<const float4*>(&sx[buf][k * IVFF_XLD + 4 * tx]);
                const float4 qa = *reinterpret_cast<const float4*>(&sq[buf][k * IVFF_QG + 4 * ty]);
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
                const float qv[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[a][r] = dense_chain_step<L2>(qv[a], xs[r], acc[a][r]);
            };
            if (kn >= IVFF_KC) {
#pragma unroll
                for (int k = 0; k < IVFF_KC; ++k) step(k);
            } else {
                for (int k = 0; k < kn; ++k) step(k);         // the last chunk of a D that is no multiple of 16: no padding in a chain
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t qb = s_qbase[4 * ty + a];
            if (qb < 0) continue;
            const int qi = sorted_q[qs + 4 * ty + a];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * tx + r;
                const int64_t pos = qb + ch * IVFF_RT + row;
                if (row < nrows && pos < stride) {
                    dense[(int64_t)qi * stride + pos] = L2 ? -acc[a][r] : acc[a][r];
                    rowid[(int64_t)qi * stride + pos] = (int)(unsigned)(MAP ? rows[r0 + row] : r0 + row);
                }
            }
        }
    }
}

// grid (task bound, <= IVFF_Y_MAX).  dense / rowid: [nq][stride].  One kernel for every store: dec is the coded store's
// [2][D], coarse [nlist][ldc] the residual form's centroids; a form that does not take them is handed nullptr / 0.  MAP: rows
// [ns] and list_off = sel_off (above); !MAP is handed rows = nullptr.
template <typename T, typename TQ, bool L2, bool PAD, bool RES, bool MAP>
__global__ __launch_bounds__(256, 2) void ivf_flat_scan_kernel(const T* __restrict__ x, int64_t ldx,
                                                               const int64_t* __restrict__ list_off, int D,
                                                               const TQ* __restrict__ q, const float* __restrict__ dec,
                                                               const float* __restrict__ coarse, int64_t ldc,
                                                               const int* __restrict__ probes, const int* __restrict__ base,
                                                               int nprobe, int64_t stride, const int* __restrict__ task_list,
                                                               const int* __restrict__ task_qstart,
                                                               const int* __restrict__ task_qcnt,
                                                               const int* __restrict__ sorted_q, float* __restrict__ dense,
                                                               int* __restrict__ rowid, const int64_t* __restrict__ rows) {
    ivf_flat_scan_body<T, TQ, L2, PAD, RES, MAP>(x, ldx, list_off, D, q, dec, coarse, ldc, probes, base, nprobe, stride, task_list,
                                                 task_qstart, task_qcnt, sorted_q, dense, rowid, rows);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
namespace {
struct ivff_ws {
    size_t dense, rowid, thr, cnt, cand, base, count, per_cell, cursor, cell_start, first_task, ntasks, sorted_q, task_list,
        task_qstart, task_qcnt, total;
    int64_t ub;
};
ivff_ws ivff_layout(int nq, int nprobe, int nlist, int64_t stride) {
    ivff_ws L;
    const size_t pairs = (size_t)nq * nprobe;
    L.ub = (int64_t)ivf_plan_task_bound(nq, nprobe, nlist, IVFF_QG);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += rc_align_up(bytes, 256); return at; };
    L.dense = take((size_t)nq * (size_t)stride * sizeof(float));
    L.rowid = take((size_t)nq * (size_t)stride * sizeof(int));
    L.thr = take((size_t)nq * sizeof(float));
    L.cnt = take((size_t)nq * sizeof(unsigned));
    L.cand = take((size_t)nq * ADC_CAND_CAP * sizeof(unsigned long long));
    L.base = take(pairs * sizeof(int));
    L.count = take((size_t)nq * sizeof(int));
    L.per_cell = take((size_t)nlist * sizeof(int));          // per_cell and cursor are adjacent: one memset clears both
    L.cursor = take((size_t)nlist * sizeof(int));
    L.cell_start = take((size_t)nlist * sizeof(int));
    L.first_task = take((size_t)nlist * sizeof(int));
    L.ntasks = take(sizeof(int));
    L.sorted_q = take(pairs * sizeof(int));
    L.task_list = take((size_t)L.ub * sizeof(int));
    L.task_qstart = take((size_t)L.ub * sizeof(int));
    L.task_qcnt = take((size_t)L.ub * sizeof(int));
    L.total = o;
    return L;
}

// rows: the subset search's row list (then list_off is its sel_off), or nullptr; the one place MAP is chosen.
template <typename T, typename TQ, bool L2, bool RES>
int ivff_launch_scan(rc_handle_t h, const T* x, int64_t ldx, const int64_t* list_off, const int64_t* rows, int D, const TQ* q,
                     const float* dec, const float* coarse, int64_t ldc, const int* probes, int nprobe, int64_t stride, char* w,
                     const ivff_ws& L, hipStream_t s) {
    auto I = [&](size_t off) { return (const int*)(w + off); };
    int64_t y = (stride + IVFF_RT - 1) / IVFF_RT;
    if (y > IVFF_Y_MAX) y = IVFF_Y_MAX;
    const dim3 grid((unsigned)L.ub, (unsigned)(y < 1 ? 1 : y));
    const bool vec = (D * (int64_t)sizeof(T)) % 16 == 0 && (ldx * (int64_t)sizeof(T)) % 16 == 0 && !((uintptr_t)x & 15u);
    const auto kernel = rows ? (vec ? ivf_flat_scan_kernel<T, TQ, L2, false, RES, true> : ivf_flat_scan_kernel<T, TQ, L2, true, RES, true>)
                             : (vec ? ivf_flat_scan_kernel<T, TQ, L2, false, RES, false> : ivf_flat_scan_kernel<T, TQ, L2, true, RES, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, x, ldx, list_off, D, q, dec, coarse, ldc, probes, I(L.base), nprobe, stride,
                       I(L.task_list), I(L.task_qstart), I(L.task_qcnt), I(L.sorted_q), (float*)(w + L.dense),
                       (int*)(w + L.rowid), rows);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// The body of the four entries.  Order of the checks: pointers and signs, shapes, the nq == 0 success, the workspace.
// dec: the coded store's [step | mid] (T = signed char), not looked at otherwise.  RES: the residual coded form, coarse
// [nlist][ldc >= D] the centroids the codes are residuals of; not looked at otherwise.  mapped (the _rows entries): after the
// argument checks of the twin, rows / sel_off null or ns outside [1, N] is RC_EINVAL; the plan and the scan then read sel_off
// where they read list_off, and the scan reads x through rows.  Neither is read on the host.
template <typename T, typename TQ, bool RES = false>
int ivff_entry(rc_handle_t h, const T* x, int64_t ldx, const int64_t* list_off, const int64_t* ids, int64_t N, int nlist, int D,
               const TQ* q, const float* dec, const float* coarse, int64_t ldc, int nq, const int* probes, int nprobe,
               int64_t stride, int k, int metric,
               float* scores, int64_t* out_ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream,
               bool mapped = false, const int64_t* rows = nullptr, int64_t ns = 0, const int64_t* sel_off = nullptr) {
    constexpr bool SQ = std::is_same<T, signed char>::value;
    rc_device_guard device_guard_(h);
    if (!h || !x || (SQ && !dec) || (RES && (!coarse || ldc < D)) || !list_off || !ids || !q || !probes || !scores || !out_ids ||
        !status || N <= 0 || nlist <= 0 || D <= 0 || ldx < D || nq < 0 || nprobe <= 0 || nprobe > nlist || stride <= 0 || k <= 0)
        return RC_EINVAL;
    if (k > ADC_CAND_CAP / 2 || N > 0xFFFFFFFFll || nlist > IVFF_MAX_NLIST || (metric != 0 && metric != 1)) return RC_ESHAPE;
    if (mapped && (!rows || !sel_off || ns < 1 || ns > N)) return RC_EINVAL;      // the twins leave rows null: !MAP below
    const int64_t* off = mapped ? sel_off : list_off;        // the cells' offsets the plan and the scan work with
    if (nq == 0) return RC_OK;
    const ivff_ws L = ivff_layout(nq, nprobe, nlist, stride);
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < L.total) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    auto I = [&](size_t off) { return (int*)(w + off); };
    const int64_t pairs = (int64_t)nq * nprobe;
    RC_HIP_CHECK(h, hipMemsetAsync(w + L.per_cell, 0, L.cell_start - L.per_cell, s));      // per_cell and cursor
    hipLaunchKernelGGL(ivf_flat_plan_query_kernel, dim3((unsigned)nq), dim3(256), 0, s, off, probes, nprobe, nlist, stride,
                       I(L.base), I(L.count), I(L.per_cell), status);
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(ivf_plan_cells_kernel, dim3(1), dim3(256), 0, s, (const int*)I(L.per_cell), nlist, I(L.cell_start),
                       I(L.first_task), I(L.ntasks), IVFF_QG);
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(ivf_plan_scatter_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, probes, pairs, nprobe, nlist,
                       (const int*)I(L.cell_start), I(L.cursor), I(L.sorted_q));
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(ivf_plan_tasks_kernel, dim3((unsigned)((L.ub + 255) / 256)), dim3(256), 0, s, (const int*)I(L.per_cell),
                       (const int*)I(L.cell_start), (const int*)I(L.first_task), (const int*)I(L.ntasks), nlist, L.ub,
                       I(L.task_list), I(L.task_qstart), I(L.task_qcnt), IVFF_QG);
    RC_LAUNCH_CHECK(h);
    rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
    int rc = metric ? ivff_launch_scan<T, TQ, true, RES>(h, x, ldx, off, rows, D, q, dec, coarse, ldc, probes, nprobe, stride, w,
                                                         L, s)
                    : ivff_launch_scan<T, TQ, false, RES>(h, x, ldx, off, rows, D, q, dec, coarse, ldc, probes, nprobe, stride,
                                                          w, L, s);
    rc_prof_mark(h, RC_PROF_ADC_SCAN, s);
    if (rc != RC_OK) return rc;
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    rc = ivf_launch_kth_filter(h, (const float*)(w + L.dense), (const int*)I(L.rowid), (const int*)I(L.count), nq, stride, k, ids,
                               (float*)(w + L.thr), cnt, cand, s);
    if (rc != RC_OK) return rc;
    // N = 0: fewer than k rows in the probed cells is legitimate, only an overflowing tie group is reported (bit 1)
    rc = rc_adc_launch_select(h, cand, cnt, nq, 0, k, 0, scores, out_ids, status, s, qstatus);
    if (rc != RC_OK) return rc;
    return metric ? dense_l2_launch_negate(h, scores, (int64_t)nq * k, s) : RC_OK;
}
}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int rc_ivf_flat_query_group(void) { return IVFF_QG; }

extern "C" size_t rc_ivf_flat_search_ws_bytes(int nq, int nprobe, int nlist, int64_t stride) {
    if (nq <= 0 || nprobe <= 0 || nlist <= 0 || nprobe > nlist || stride <= 0) return 0;
    return ivff_layout(nq, nprobe, nlist, stride).total;
}

extern "C" int rc_ivf_flat_search(rc_handle_t h, const float* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                  int64_t N, int nlist, int D, const float* q, int nq, const int* probes, int nprobe,
                                  int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status, int* qstatus,
                                  void* ws, size_t ws_bytes, rc_stream_t stream) {
    return ivff_entry<float, float>(h, x, ldx, list_off, ids, N, nlist, D, q, nullptr, nullptr, 0, nq, probes, nprobe, stride, k,
                                    metric, scores, out_ids, status, qstatus, ws, ws_bytes, stream);
}

extern "C" int rc_ivf_flat_f16_search(rc_handle_t h, const uint16_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                      int64_t N, int nlist, int D, const uint16_t* q, int nq, const int* probes, int nprobe,
                                      int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status,
                                      int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return ivff_entry<_Float16, _Float16>(h, reinterpret_cast<const _Float16*>(x), ldx, list_off, ids, N, nlist, D,
                                reinterpret_cast<const _Float16*>(q), nullptr, nullptr, 0, nq, probes, nprobe, stride, k, metric,
                                scores, out_ids, status, qstatus, ws, ws_bytes, stream);
}

extern "C" int rc_ivf_flat_sq8_search(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                      int64_t N, int nlist, int D, const float* q, int nq, const float* dec, const int* probes,
                                      int nprobe, int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status,
                                      int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    // the codec's width limit first, as the rc_dense_sq8 entries order it (shapes, then pointers); then the shared order
    if (D > rc_dense_sq8_max_d()) return RC_ESHAPE;
    return ivff_entry<signed char, float>(h, reinterpret_cast<const signed char*>(x), ldx, list_off, ids, N, nlist, D, q, dec,
                                          nullptr, 0, nq, probes, nprobe, stride, k, metric, scores, out_ids, status, qstatus, ws,
                                          ws_bytes, stream);
}

extern "C" int rc_ivf_flat_sq8r_search(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                       int64_t N, int nlist, int D, const float* q, int nq, const float* dec, const float* coarse,
                                       int64_t ldc, const int* probes, int nprobe, int64_t stride, int k, int metric, float* scores,
                                       int64_t* out_ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    // the order of rc_ivf_flat_sq8_search: the codec's width limit, then the shared order with dec and coarse among the pointers
    if (D > rc_dense_sq8_max_d()) return RC_ESHAPE;
    return ivff_entry<signed char, float, true>(h, reinterpret_cast<const signed char*>(x), ldx, list_off, ids, N, nlist, D, q, dec,
                                                coarse, ldc, nq, probes, nprobe, stride, k, metric, scores, out_ids, status,
                                                qstatus, ws, ws_bytes, stream);
}

// The subset searches: the arguments of the twin, then rows [ns], ns, sel_off [nlist + 1] (include/repconc_hip.h).
extern "C" int rc_ivf_flat_search_rows(rc_handle_t h, const float* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                       int64_t N, int nlist, int D, const float* q, int nq, const int* probes, int nprobe,
                                       int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status,
                                       int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream, const int64_t* rows, int64_t ns,
                                       const int64_t* sel_off) {
    return ivff_entry<float, float>(h, x, ldx, list_off, ids, N, nlist, D, q, nullptr, nullptr, 0, nq, probes, nprobe, stride, k,
                                    metric, scores, out_ids, status, qstatus, ws, ws_bytes, stream, true, rows, ns, sel_off);
}

extern "C" int rc_ivf_flat_f16_search_rows(rc_handle_t h, const uint16_t* x, int64_t ldx, const int64_t* list_off,
                                           const int64_t* ids, int64_t N, int nlist, int D, const uint16_t* q, int nq,
                                           const int* probes, int nprobe, int64_t stride, int k, int metric, float* scores,
                                           int64_t* out_ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                                           rc_stream_t stream, const int64_t* rows, int64_t ns, const int64_t* sel_off) {
    return ivff_entry<_Float16, _Float16>(h, reinterpret_cast<const _Float16*>(x), ldx, list_off, ids, N, nlist, D,
                                          reinterpret_cast<const _Float16*>(q), nullptr, nullptr, 0, nq, probes, nprobe, stride, k,
                                          metric, scores, out_ids, status, qstatus, ws, ws_bytes, stream, true, rows, ns, sel_off);
}

extern "C" int rc_ivf_flat_sq8_search_rows(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off, const int64_t* ids,
                                           int64_t N, int nlist, int D, const float* q, int nq, const float* dec, const int* probes,
                                           int nprobe, int64_t stride, int k, int metric, float* scores, int64_t* out_ids,
                                           int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream,
                                           const int64_t* rows, int64_t ns, const int64_t* sel_off) {
    if (D > rc_dense_sq8_max_d()) return RC_ESHAPE;
    return ivff_entry<signed char, float>(h, reinterpret_cast<const signed char*>(x), ldx, list_off, ids, N, nlist, D, q, dec,
                                          nullptr, 0, nq, probes, nprobe, stride, k, metric, scores, out_ids, status, qstatus, ws,
                                          ws_bytes, stream, true, rows, ns, sel_off);
}

extern "C" int rc_ivf_flat_sq8r_search_rows(rc_handle_t h, const int8_t* x, int64_t ldx, const int64_t* list_off,
                                            const int64_t* ids, int64_t N, int nlist, int D, const float* q, int nq,
                                            const float* dec, const float* coarse, int64_t ldc, const int* probes, int nprobe,
                                            int64_t stride, int k, int metric, float* scores, int64_t* out_ids, int* status,
                                            int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream, const int64_t* rows,
                                            int64_t ns, const int64_t* sel_off) {
    if (D > rc_dense_sq8_max_d()) return RC_ESHAPE;
    return ivff_entry<signed char, float, true>(h, reinterpret_cast<const signed char*>(x), ldx, list_off, ids, N, nlist, D, q, dec,
                                                coarse, ldc, nq, probes, nprobe, stride, k, metric, scores, out_ids, status,
                                                qstatus, ws, ws_bytes, stream, true, rows, ns, sel_off);
}
