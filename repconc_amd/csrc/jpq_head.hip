// Stage-2 (JPQ) scoring head: scores of (query, document id) pairs straight from the resident uint8 codes, and the
// gradients of those scores w.r.t. the queries and the centroids — the reference's search -> index_select -> decode ->
// multiply -> sum (models/jpq/finetune_jpq.py:176-189) without the decoded [nq*k, D] embeddings and without atomics on
// values.  The arithmetic is fixed on the OUTPUT (DESIGN.md "JPQ scoring head"): every product is of two fp32 values taken
// in fp64 (exact), every sum is fp64, sequential from 0.0 in a stated order, rounded to fp32 once — so each result is a
// function of the inputs alone, whatever the launch.
//
//   scores[i,t]    = fp32( sum_m ( sum_j q[i, m*dsub+j] * C[m, codes[pids[i,t], m], j] ) )     j ascending, then m ascending
//   grad_q[i, d]   = fp32( sum_t g[i,t] * C[m, codes[pids[i,t], m], j] )                        t ascending, d = m*dsub+j
//   grad_C[m,c,j]  = fp32( sum_p g[p] * q[p div k, m*dsub+j] )   over the pairs p = i*k+t with codes[pids[p], m] == c, p ascending
//
// A pair whose id is outside [0, N) is a HOLE (the -1 padding of a short index): score +0.0f, no gradient.
//
//   jpq_fwd_kernel      16 lanes per pair: lane l owns the sub-quantisers m = l, l+16, ...; the 16 partial sums of a chunk are
//                       passed round the group and added in m order by every lane (no LDS, no shape-sized resource)
//   jpq_gradq_kernel    thread per (query, d): walks the query's k pairs in order
//   code_sort_*_kernel  stable counting sort of the pairs by code, per sub-quantiser (code_sort.h, shared with the
//                       deterministic decode backward): perm[m][.] = the pairs of every (m, c) segment, ascending
//   jpq_gradc_kernel    thread per (m, c, j): the one owner of its output adds its segment in order
//
// The only atomics of the unit are the integer tile counts of the sort's hist kernel (order-free).  Every kernel walks its work with
// a grid-stride loop, so nq*k < 2^31 needs no large grid.
#include "rc_common.h"
#include "code_sort.h"

#define JH_TILE CS_TILE       // pairs per sort tile (code_sort.h)
#define JH_U 8                // independent loads in flight ahead of an ordered chain of adds
#define JH_MAX_GRID CS_MAX_GRID

// ------------------------------------------------------------------------------------------------------- forward
template <bool VEC4>
__global__ __launch_bounds__(256) void jpq_fwd_kernel(const float* __restrict__ q, const uint8_t* __restrict__ codes, int64_t N,
                                                      const int64_t* __restrict__ pids, const float* __restrict__ C, int64_t P,
                                                      int k, int M, int dsub, float* __restrict__ scores) {
    const int l = threadIdx.x & 15;
    const int64_t D = (int64_t)M * dsub;
    for (int64_t base = (int64_t)blockIdx.x * 16; base < P; base += (int64_t)gridDim.x * 16) {   // uniform over the block
        const int64_t p = base + (threadIdx.x >> 4);
        const bool valid = p < P;
        const int64_t pid = valid ? pids[p] : -1;
        const bool hole = pid < 0 || pid >= N;
        const float* qrow = q + (valid ? p / k : 0) * D;
        double tot = 0.0;
        for (int m0 = 0; m0 < M; m0 += 16) {
            const int m = m0 + l;
            double s = 0.0;
            if (!hole && m < M) {
                const int code = codes[pid * M + m];
                const float* qp = qrow + (int64_t)m * dsub;
                const float* cp = C + ((size_t)m * RC_K + code) * dsub;
                if (VEC4) {
                    for (int j = 0; j < dsub; j += 4) {
                        const float4 a = *reinterpret_cast<const float4*>(qp + j);
                        const float4 b = *reinterpret_cast<const float4*>(cp + j);
                        s = s + (double)a.x * (double)b.x;
                        s = s + (double)a.y * (double)b.y;
                        s = s + (double)a.z * (double)b.z;
                        s = s + (double)a.w * (double)b.w;
                    }
                } else {
                    for (int j = 0; j < dsub; ++j) s = s + (double)qp[j] * (double)cp[j];
                }
            }
            const int nm = (M - m0 < 16) ? M - m0 : 16;
            for (int u = 0; u < nm; ++u) tot = tot + __shfl(s, u, 16);      // m ascending, the same chain on all 16 lanes
        }
        if (valid && l == 0) scores[p] = (float)tot;                         // a hole added nothing: +0.0f
    }
}

// ------------------------------------------------------------------------------------------------------- grad_q
// work item = (query i, slice of 256 columns); a thread owns grad_q[i, d].  JH_U pairs' codes and centroid values are
// fetched ahead, then added in t order.
__global__ __launch_bounds__(256) void jpq_gradq_kernel(const uint8_t* __restrict__ codes, int64_t N, const int64_t* __restrict__ pids,
                                                        const float* __restrict__ C, const float* __restrict__ g, int nq, int k,
                                                        int M, int dsub, float* __restrict__ gq) {
    const int D = M * dsub;
    const int slices = (D + 255) / 256;
    const int64_t items = (int64_t)nq * slices;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t i = w / slices;
        const int d = (int)(w - i * slices) * 256 + threadIdx.x;
        if (d >= D) continue;
        const int m = d / dsub, j = d - m * dsub;
        const float* Cm = C + (size_t)m * RC_K * dsub + j;
        const int64_t* prow = pids + i * k;
        const float* grow = g + i * k;
        double acc = 0.0;
        for (int t0 = 0; t0 < k; t0 += JH_U) {
            bool ok[JH_U];
            float gg[JH_U], cc[JH_U];
#pragma unroll
            for (int u = 0; u < JH_U; ++u) {
                const int t = t0 + u;
                const int64_t pid = (t < k) ? prow[t] : -1;
                ok[u] = pid >= 0 && pid < N;
                const int code = ok[u] ? (int)codes[pid * M + m] : 0;      // a hole reads centroid 0 and does not use it
                cc[u] = Cm[(size_t)code * dsub];
                gg[u] = ok[u] ? grow[t] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < JH_U; ++u)
                if (ok[u]) acc = acc + (double)gg[u] * (double)cc[u];
        }
        gq[i * D + d] = (float)acc;
    }
}

// ------------------------------------------------------------------------------------------------------- the sort
// code_sort.h, over the pairs: the code of pair p under m is codes[pids[p]*M + m]; a pair whose id is outside [0, N) is a hole.
struct jpq_code_src {
    const uint8_t* codes;
    int64_t N;
    const int64_t* pids;
    int M;
    __device__ __forceinline__ int operator()(int64_t p, int m) const {
        const int64_t pid = pids[p];
        return (pid >= 0 && pid < N) ? (int)codes[pid * M + m] : -1;
    }
};

// ------------------------------------------------------------------------------------------------------- grad_C
// thread per (m, c, j) — the only writer of grad_C[m, c, j] — adds its segment's pairs in ascending p; an empty segment
// stores (float)0.0 = +0.0f.
__global__ __launch_bounds__(256) void jpq_gradc_kernel(const float* __restrict__ q, const float* __restrict__ g, int64_t P, int k,
                                                        int M, int dsub, const unsigned* __restrict__ perm,
                                                        const unsigned* __restrict__ start, const unsigned* __restrict__ count,
                                                        float* __restrict__ gC) {
    const int64_t D = (int64_t)M * dsub;
    const int64_t total = D * RC_K;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t seg = e / dsub;                    // m * 256 + c
        const int j = (int)(e - seg * dsub);
        const int m = (int)(seg / RC_K);
        const unsigned n = count[seg];
        const unsigned* pm = perm + (size_t)m * P + start[seg];
        const float* qd = q + (int64_t)m * dsub + j;
        double acc = 0.0;
        unsigned i = 0;
        for (; i + JH_U <= n; i += JH_U) {
            float gg[JH_U], qq[JH_U];
#pragma unroll
            for (int u = 0; u < JH_U; ++u) {
                const unsigned p = pm[i + u];
                gg[u] = g[p];
                qq[u] = qd[(int64_t)(p / (unsigned)k) * D];
            }
#pragma unroll
            for (int u = 0; u < JH_U; ++u) acc = acc + (double)gg[u] * (double)qq[u];
        }
        for (; i < n; ++i) {
            const unsigned p = pm[i];
            acc = acc + (double)g[p] * (double)qd[(int64_t)(p / (unsigned)k) * D];
        }
        gC[e] = (float)acc;
    }
}

// ------------------------------------------------------------------------------------------------------- entry points
static inline unsigned jh_grid(int64_t blocks) { return cs_grid(blocks, JH_MAX_GRID); }

// the sort's workspace over the nq*k pairs (code_sort.h)
extern "C" size_t rc_jpq_head_ws_bytes(int nq, int k, int M) {
    if (nq <= 0 || k <= 0 || M <= 0) return 0;
    const int64_t P = (int64_t)nq * k;
    if (P > 0x7FFFFFFFll) return 0;
    return code_sort_ws::bytes(P, M);
}

static int jh_check(rc_handle_t h, const void* q, const void* codes, int64_t N, const void* pids, const void* C, int nq, int k, int M,
                    int K, int dsub) {
    if (!h || N < 0 || nq < 0 || k < 0 || M <= 0 || dsub <= 0) return RC_EINVAL;
    if (K != RC_K || N > 0xFFFFFFFFll || (int64_t)nq * k > 0x7FFFFFFFll || (int64_t)M * dsub > 0x7FFFFFFFll) return RC_ESHAPE;
    if (nq > 0 && k > 0 && (!q || !pids || !C || (N > 0 && !codes))) return RC_EINVAL;
    return RC_OK;
}

extern "C" int rc_jpq_head_fwd(rc_handle_t h, const float* q, const uint8_t* codes, int64_t N, const int64_t* pids, const float* C,
                               int nq, int k, int M, int K, int dsub, float* scores, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int rc = jh_check(h, q, codes, N, pids, C, nq, k, M, K, dsub);
    if (rc != RC_OK) return rc;
    if (nq == 0 || k == 0) return RC_OK;
    if (!scores) return RC_EINVAL;
    const int64_t P = (int64_t)nq * k;
    const unsigned grid = jh_grid((P + 15) / 16);
    hipStream_t s = (hipStream_t)stream;
    if (dsub % 4 == 0 && (((uintptr_t)q | (uintptr_t)C) & 15) == 0)
        hipLaunchKernelGGL(jpq_fwd_kernel<true>, dim3(grid), dim3(256), 0, s, q, codes, N, pids, C, P, k, M, dsub, scores);
    else
        hipLaunchKernelGGL(jpq_fwd_kernel<false>, dim3(grid), dim3(256), 0, s, q, codes, N, pids, C, P, k, M, dsub, scores);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// grad_q [nq, D] and / or grad_C [M, 256, dsub]: a null output is not computed.  ws is needed for grad_C only.
extern "C" int rc_jpq_head_bwd(rc_handle_t h, const float* q, const uint8_t* codes, int64_t N, const int64_t* pids, const float* C,
                               const float* g, int nq, int k, int M, int K, int dsub, float* grad_q, float* grad_C, void* ws,
                               size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int rc = jh_check(h, q, codes, N, pids, C, nq, k, M, K, dsub);
    if (rc != RC_OK) return rc;
    if (nq == 0 || k == 0) return RC_OK;
    if (!g || (!grad_q && !grad_C)) return RC_EINVAL;
    if (grad_C && (!ws || ws_bytes < rc_jpq_head_ws_bytes(nq, k, M))) return RC_EWORKSPACE;
    const int64_t P = (int64_t)nq * k;
    const int D = M * dsub;
    hipStream_t s = (hipStream_t)stream;
    if (grad_q) {
        hipLaunchKernelGGL(jpq_gradq_kernel, dim3(jh_grid((int64_t)nq * ((D + 255) / 256))), dim3(256), 0, s, codes, N, pids, C, g, nq, k,
                           M, dsub, grad_q);
        RC_LAUNCH_CHECK(h);
    }
    if (grad_C) {
        const code_sort_ws L(ws, P, M);
        const jpq_code_src src{codes, N, pids, M};
        const int sorted = code_sort(h, src, P, M, L, JH_MAX_GRID, s);
        if (sorted != RC_OK) return sorted;
        hipLaunchKernelGGL(jpq_gradc_kernel, dim3(jh_grid(((int64_t)D * RC_K + 255) / 256)), dim3(256), 0, s, q, g, P, k, M, dsub,
                           (const unsigned*)L.perm, (const unsigned*)L.start, (const unsigned*)L.count, grad_C);
        RC_LAUNCH_CHECK(h);
    }
    return RC_OK;
}
