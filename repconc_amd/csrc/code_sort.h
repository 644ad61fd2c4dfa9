// Stable counting sort of P items by an 8-bit code, once per sub-quantiser m (the pattern of rc_ivf_coarse_update, kmeans.hip):
// per-tile counts -> exclusive offsets -> perm[m][.] = the items of every (m, c) segment, ascending.  Shared by the two
// fixed-order centroid gradients: the JPQ scoring head (jpq_head.hip, items = (query, id) pairs) and the deterministic
// decode backward (decode_det.hip, items = rows).
//
// Where an item's code comes from is the template parameter.  A code source `Src` is a small struct passed to the kernels by
// value with
//     __device__ int operator()(int64_t p, int m) const;      // the code of item p under sub-quantiser m in [0, 256),
//                                                             // or a negative value for a HOLE (sorted nowhere, counted nowhere)
//
//   code_sort_hist_kernel<Src>      hist[m][tile][c] = items of the tile with code c under m
//   code_sort_scan_kernel           hist -> exclusive offsets along the tiles; count[m][c], start[m][c]
//   code_sort_scatter_kernel<Src>   perm[m][start[m][c] .. + count[m][c]) = the items with code c under m, ascending
//
// Tiles of CS_TILE items, one wave per (tile, m), 64 items per step, eight ballots per step for the rank among the lanes of
// the step with the same code.  The only atomics are the integer LDS counts of the hist kernel (order-free).  Every kernel
// walks its work with a grid-stride loop; nothing is sized by the shape except the caller's workspace:
//   hist [M][tiles][256], count [M][256], start [M][256], perm [M][P] — all uint32, each aligned to 256 bytes.  P < 2^31.
#pragma once
#include "rc_common.h"

#define CS_TILE 1024          // items per sort tile: 16 wave-wide steps of one wave
#define CS_MG 4               // sub-quantisers (= waves) per sort block
#define CS_MAX_GRID 65536

// all lanes of the wave that are `valid` and hold the same 8-bit code as this lane (meaningless on a lane that is not valid)
__device__ __forceinline__ unsigned long long cs_same_code(int c, bool valid) {
    unsigned long long mask = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (c >> b) & 1;
        const unsigned long long bal = __ballot(bit);
        mask &= bit ? bal : ~bal;
    }
    return mask;
}

// work item = (tile of CS_TILE items, group of CS_MG sub-quantisers); wave v of the block serves m = group*CS_MG + v.
// hist[m][tile][c] = items of the tile with code c under m (holes are not counted).
template <typename Src>
__global__ __launch_bounds__(64 * CS_MG) void code_sort_hist_kernel(const Src src, int64_t P, int M, int64_t tiles,
                                                                    unsigned* __restrict__ hist) {
    __shared__ unsigned cnt[CS_MG][RC_K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int groups = (M + CS_MG - 1) / CS_MG;
    const int64_t items = tiles * groups;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t tile = w / groups;
        const int m = (int)(w - tile * groups) * CS_MG + wv;
        const bool live = m < M;
        for (int c = lane; c < RC_K; c += 64) cnt[wv][c] = 0u;
        __syncthreads();
        const int64_t p0 = tile * CS_TILE;
        for (int s = 0; s < CS_TILE; s += 64) {
            const int64_t p = p0 + s + lane;
            if (live && p < P) {
                const int c = src(p, m);
                if (c >= 0) atomicAdd(&cnt[wv][c], 1u);                         // integer counts: order-free
            }
        }
        __syncthreads();
        if (live)
            for (int c = lane; c < RC_K; c += 64) hist[((size_t)m * tiles + tile) * RC_K + c] = cnt[wv][c];
        __syncthreads();
    }
}

// block per sub-quantiser, thread per code: hist[m][.][c] -> exclusive offsets along the tiles, count[m][c] = the segment's
// length, start[m][c] = its first slot in perm[m] (exclusive scan of the counts over c).
static __global__ __launch_bounds__(RC_K) void code_sort_scan_kernel(unsigned* __restrict__ hist, int64_t tiles, int M,
                                                                     unsigned* __restrict__ count, unsigned* __restrict__ start) {
    __shared__ unsigned s_w[RC_K / 64];
    const int c = threadIdx.x, lane = c & 63, wv = c >> 6;
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        unsigned run = 0;
        for (int64_t t = 0; t < tiles; ++t) {
            const size_t at = ((size_t)m * tiles + t) * RC_K + c;
            const unsigned v = hist[at];
            hist[at] = run;
            run += v;
        }
        count[(size_t)m * RC_K + c] = run;
        unsigned incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        unsigned before = 0;
        for (int v = 0; v < wv; ++v) before += s_w[v];
        start[(size_t)m * RC_K + c] = before + incl - run;
        __syncthreads();
    }
}

// Same walk as the hist kernel.  The wave steps through its tile 64 items at a time; an item's slot is the running position of
// its segment plus the number of lower lanes of the step with the same code, so perm[m] lists every segment in ascending p.
template <typename Src>
__global__ __launch_bounds__(64 * CS_MG) void code_sort_scatter_kernel(const Src src, int64_t P, int M, int64_t tiles,
                                                                       const unsigned* __restrict__ hist,
                                                                       const unsigned* __restrict__ start,
                                                                       unsigned* __restrict__ perm) {
    __shared__ unsigned pos[CS_MG][RC_K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int groups = (M + CS_MG - 1) / CS_MG;
    const int64_t items = tiles * groups;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t tile = w / groups;
        const int m = (int)(w - tile * groups) * CS_MG + wv;
        const bool live = m < M;
        if (live)
            for (int c = lane; c < RC_K; c += 64)
                pos[wv][c] = start[(size_t)m * RC_K + c] + hist[((size_t)m * tiles + tile) * RC_K + c];
        __syncthreads();
        const int64_t p0 = tile * CS_TILE;
        for (int s = 0; s < CS_TILE; s += 64) {
            const int64_t p = p0 + s + lane;
            bool valid = live && p < P;
            int c = 0;
            if (valid) {
                c = src(p, m);
                valid = c >= 0;
                if (!valid) c = 0;
            }
            const unsigned long long same = cs_same_code(c, valid);
            const unsigned at = valid ? pos[wv][c] : 0u;
            __syncthreads();                                                    // every lane has read before any lane advances
            if (valid) {
                const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
                perm[(size_t)m * P + at + rank] = (unsigned)p;
                if (lane == 63 - (int)__builtin_clzll(same)) pos[wv][c] = at + (unsigned)__popcll(same);   // last lane of the group
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------- host side
static inline int64_t cs_tiles(int64_t P) { return (P + CS_TILE - 1) / CS_TILE; }

static inline unsigned cs_grid(int64_t blocks, int64_t cap = CS_MAX_GRID) {
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks > cap ? cap : blocks);
}

// the workspace of one sort of P items under M sub-quantisers, carved from the caller's block in this order
struct code_sort_ws {
    unsigned *hist, *count, *start, *perm;
    static size_t bytes(int64_t P, int M) {
        return rc_align_up((size_t)M * cs_tiles(P) * RC_K * sizeof(unsigned), 256) + 2 * rc_align_up((size_t)M * RC_K * sizeof(unsigned), 256) +
               rc_align_up((size_t)M * P * sizeof(unsigned), 256);
    }
    code_sort_ws(void* ws, int64_t P, int M) {
        char* w = (char*)ws;
        hist = (unsigned*)w;  w += rc_align_up((size_t)M * cs_tiles(P) * RC_K * sizeof(unsigned), 256);
        count = (unsigned*)w; w += rc_align_up((size_t)M * RC_K * sizeof(unsigned), 256);
        start = (unsigned*)w; w += rc_align_up((size_t)M * RC_K * sizeof(unsigned), 256);
        perm = (unsigned*)w;
    }
};

// the three launches; 0 < P < 2^31, M >= 1, max_grid >= 1 blocks per launch
template <typename Src>
static int code_sort(rc_handle_t h, const Src& src, int64_t P, int M, const code_sort_ws& L, int64_t max_grid, hipStream_t s) {
    const int64_t tiles = cs_tiles(P);
    const unsigned sort_grid = cs_grid(tiles * ((M + CS_MG - 1) / CS_MG), max_grid);
    hipLaunchKernelGGL(code_sort_hist_kernel<Src>, dim3(sort_grid), dim3(64 * CS_MG), 0, s, src, P, M, tiles, L.hist);
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(code_sort_scan_kernel, dim3(cs_grid(M, max_grid)), dim3(RC_K), 0, s, L.hist, tiles, M, L.count, L.start);
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(code_sort_scatter_kernel<Src>, dim3(sort_grid), dim3(64 * CS_MG), 0, s, src, P, M, tiles,
                       (const unsigned*)L.hist, (const unsigned*)L.start, L.perm);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
