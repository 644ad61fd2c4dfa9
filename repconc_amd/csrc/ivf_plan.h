// The device-side plan of the list-centric IVF searches, shared by ivf_lists.hip (PQ codes) and ivf_flat.hip (dense rows): from
// the number of queries probing every cell (per_cell, counted by the unit's own per-query kernel) to the task list — cells,
// then the queries of every cell, then tasks of up to `tw` queries of one cell.  Device code: every unit compiles its own copy
// (static kernels, no -fgpu-rdc).  Nothing here depends on what a cell's rows hold.
#pragma once
#include "rc_common.h"

// exclusive scan of one int per thread over a 256-thread block; returns the block total through `total`
__device__ __forceinline__ int ivfp_block_scan256(int v, int* s_wave, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) before += (j < wv) ? s_wave[j] : 0;
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return before + inc - v;
}

// One block: exclusive prefix sums over the cells of (queries probing the cell) and of (tasks of the cell).
static __global__ __launch_bounds__(256) void ivf_plan_cells_kernel(const int* __restrict__ per_cell, int nlist,
                                                                    int* __restrict__ cell_start, int* __restrict__ first_task,
                                                                    int* __restrict__ ntasks, int tw) {
    __shared__ int s_wave[4];
    int cq = 0, ct = 0;
    for (int b0 = 0; b0 < nlist; b0 += 256) {
        const int c = b0 + (int)threadIdx.x;
        const int n = c < nlist ? per_cell[c] : 0, t = (n + tw - 1) / tw;     // tw = queries per task (8 | 16)
        int tq, tt;
        const int eq = ivfp_block_scan256(n, s_wave, tq);
        const int et = ivfp_block_scan256(t, s_wave, tt);
        if (c < nlist) { cell_start[c] = cq + eq; first_task[c] = ct + et; }
        cq += tq;
        ct += tt;
    }
    if (threadIdx.x == 0) *ntasks = ct;
}

// (query, probe) pairs bucketed by cell; the order inside a cell is whatever the atomics give — it only decides which
// queries share a task, never a result.  A probe outside [0, nlist) belongs to no cell and is skipped, as the unit's per-query
// kernel must have skipped it when it counted per_cell.
static __global__ __launch_bounds__(256) void ivf_plan_scatter_kernel(const int* __restrict__ probes, int64_t pairs, int nprobe,
                                                                      int nlist, const int* __restrict__ cell_start,
                                                                      int* __restrict__ cursor, int* __restrict__ sorted_q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pairs) return;
    const int c = probes[i];
    if (c < 0 || c >= nlist) return;
    sorted_q[cell_start[c] + atomicAdd(cursor + c, 1)] = (int)(i / nprobe);
}

// task t -> (cell, first entry in sorted_q, number of queries); tasks past the device-side count get 0 queries
static __global__ __launch_bounds__(256) void ivf_plan_tasks_kernel(const int* __restrict__ per_cell, const int* __restrict__ cell_start,
                                                                    const int* __restrict__ first_task, const int* __restrict__ ntasks,
                                                                    int nlist, int64_t ub, int* __restrict__ task_list,
                                                                    int* __restrict__ task_qstart, int* __restrict__ task_qcnt, int tw) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ub) return;
    int cell = 0, qs = 0, qc = 0;
    if (t < *ntasks) {
        int lo = 0, hi = nlist;                               // last cell with first_task <= t (the non-empty one of a plateau)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first_task[mid] <= (int)t) lo = mid; else hi = mid;
        }
        cell = lo;
        const int within = (int)t - first_task[cell];
        qs = cell_start[cell] + tw * within;
        qc = per_cell[cell] - tw * within;
        qc = qc > tw ? tw : qc;
    }
    task_list[t] = cell;
    task_qstart[t] = qs;
    task_qcnt[t] = qc;
}

// upper bound of the number of tasks of nq x nprobe pairs over nlist cells at tw queries per task: at most one partly filled
// group per probed cell
static inline size_t ivf_plan_task_bound(int nq, int nprobe, int nlist, int tw) {
    const size_t pairs = (size_t)nq * nprobe;
    size_t ub = (size_t)nlist + pairs / tw + 1;
    return ub > pairs ? pairs : ub;
}
