// Stage-1 in-batch contrastive loss, fused after the similarity GEMM: the duplicate and false-negative masks from the ids,
// the dynamic top-k cut, the log-softmax cross-entropy and its gradient — the reference's torch composition
// (models/repconc/finetune_repconc.py:398-451) without the [nd, nd] duplicate compare, without an [nq, nd] mask and
// without atomics on values.  The arithmetic is fixed on the OUTPUT (include/repconc_hip.h, rc_contrastive_*): the logits z
// are fp32 with the reference's roundings (bit-equal to the composition on tie-free rows), everything after them is fp64 in a
// stated order, rounded to fp32 once — so loss and gradient are functions of the inputs alone.
//
//   cl_dup_kernel     dup[j] = some i < j has docids[i] == docids[j]: 64 columns per block, the earlier ids stream through LDS
//                     in tiles of 256, the four waves of a block each compare a quarter of a tile (all-pairs: nd <= 2^18)
//   cl_fwd_kernel     one block per query row; the row (49 152 floats in the recipe) does not fit in LDS and is re-read from
//                     L2 / HBM by every pass, the mask of an entry is recomputed from docids / dup / the row's positives:
//                       select  the topk-th largest key of neg[i, :] (adc_kth_largest of topk.h; only when 0 < topk < nd)
//                       count   keys above / equal to it, per wave segment
//                       mark    wave w walks its contiguous quarter of the row's 64-column words in order: an equal key is kept
//                               while fewer than topk - #above equal keys precede it (ascending j), the keep bits of a word are one
//                               wave ballot stored by lane 0, z goes to z_out if asked for, the row maximum is taken
//                       sum     sum_{j != i} exp(z - max) in fp64
//   cl_finish_kernel  loss = fp32(sum_i loss_i / nq), i ascending, one thread
//   cl_bwd_kernel     one block per row: z again from sim, the ids and the keep bits, then the softmax gradient
#include "rc_common.h"
#include "topk.h"

#define CL_THREADS 256
#define CL_WAVES 4                // CL_THREADS / 64
#define CL_WORD 64                // columns per keep word = one wave step
#define CL_DUP_COLS 64            // columns per block of the duplicate kernel
#define CL_DUP_TILE 256           // earlier ids staged per step of the duplicate kernel
#define CL_REL_LDS 64             // positives of a row kept in LDS (the rest is read from global memory)
#define CL_U 4                    // independent loads in flight ahead of the ordered part of a pass
#define CL_MAX_ND (1 << 18)       // the all-pairs duplicate kernel: nd^2 / 2 compares
#define CL_STAT 4                 // doubles per row: max, sum, sum without the diagonal, loss_i

static_assert(CL_THREADS == CL_WAVES * 64 && CL_DUP_TILE == CL_THREADS && CL_DUP_COLS == 64, "block shapes");

// ------------------------------------------------------------------------------------------------------- workspace
struct cl_ws {
    size_t dup, keep, stat, total;
    int64_t words;                                                    // keep words per row
    cl_ws(int64_t nq, int64_t nd) {
        words = (nd + CL_WORD - 1) / CL_WORD;
        size_t o = 0;
        dup = o;  o += rc_align_up((size_t)nd, 256);
        keep = o; o += rc_align_up((size_t)nq * (size_t)words * sizeof(unsigned long long), 256);
        stat = o; o += rc_align_up((size_t)nq * CL_STAT * sizeof(double), 256);
        total = o;
    }
};

// ------------------------------------------------------------------------------------------------------- duplicates
__global__ __launch_bounds__(CL_THREADS) void cl_dup_kernel(const int64_t* __restrict__ docids, int64_t nd, uint8_t* __restrict__ dup) {
    __shared__ int64_t tile[CL_DUP_TILE];
    __shared__ int s_flag[CL_WAVES][CL_DUP_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * CL_DUP_COLS, j = j0 + lane;
    const bool valid = j < nd;
    const int64_t mine = valid ? docids[j] : 0;
    const int64_t jend = (j0 + CL_DUP_COLS < nd) ? j0 + CL_DUP_COLS : nd;          // earlier ids end before the block's last column
    int flag = 0;
    for (int64_t t0 = 0; t0 + 1 < jend; t0 += CL_DUP_TILE) {                        // block-uniform
        const int64_t src = t0 + tid;
        tile[tid] = src < nd ? docids[src] : 0;
        __syncthreads();
        const int64_t e0 = t0 + wv * 64;
#pragma unroll 8
        for (int e = 0; e < 64; ++e)                                                // e0 + e < j < nd: the entry was loaded
            flag |= (valid && e0 + e < j && tile[wv * 64 + e] == mine) ? 1 : 0;
        __syncthreads();
    }
    s_flag[wv][lane] = flag;
    __syncthreads();
    if (wv == 0 && valid) dup[j] = (uint8_t)(s_flag[0][lane] | s_flag[1][lane] | s_flag[2][lane] | s_flag[3][lane]);
}

// ------------------------------------------------------------------------------------------------------- one row
// What a pass needs to recompute an entry of row i: the row of sim, the ids, the duplicate flags and the row's positives.
struct cl_row {
    const float* sim;                 // sim + i * nd
    const int64_t* docids;
    const uint8_t* dup;
    const int64_t* rel_lds;           // the first min(nrel, CL_REL_LDS) positives
    const int64_t* rel_glb;           // all of them
    int64_t nrel, i, nd;

    // z1 = sim - 10000 * mask: a masked entry takes one fp32 subtraction, an unmasked one is sim itself
    __device__ __forceinline__ float z1(int64_t j, float s, int64_t d, uint8_t du) const {
        bool m = du != 0;
        const int64_t nl = nrel < CL_REL_LDS ? nrel : CL_REL_LDS;
        for (int64_t r = 0; r < nl; ++r) m = m || rel_lds[r] == d;
        for (int64_t r = CL_REL_LDS; r < nrel; ++r) m = m || rel_glb[r] == d;
        return (m && j != i) ? s - 10000.0f : s;
    }
    // the key the cut orders by: neg = z1 with the diagonal at -10000; "+ 0.0f" makes -0.0 and +0.0 one key
    __device__ __forceinline__ unsigned key(int64_t j, float z1v) const {
        return adc_order_key((j == i ? -10000.0f : z1v) + 0.0f);
    }
    __device__ __forceinline__ unsigned key_at(int64_t j) const { return key(j, z1(j, sim[j], docids[j], dup[j])); }
};

// the positives of row blockIdx.x: rel_ids[lo, hi) with both ends clamped into [0, R]; the first CL_REL_LDS go to LDS
__device__ __forceinline__ cl_row cl_open_row(const float* sim, const int64_t* docids, const int64_t* rel_off, const int64_t* rel_ids,
                                              int64_t R, int64_t nd, const uint8_t* dup, int64_t* s_rel) {
    const int64_t i = blockIdx.x;
    int64_t lo = rel_off[i], hi = rel_off[i + 1];
    lo = lo < 0 ? 0 : (lo > R ? R : lo);
    hi = hi < lo ? lo : (hi > R ? R : hi);
    if ((int64_t)threadIdx.x < hi - lo && threadIdx.x < CL_REL_LDS) s_rel[threadIdx.x] = rel_ids[lo + threadIdx.x];
    __syncthreads();
    return cl_row{sim + i * nd, docids, dup, s_rel, rel_ids + lo, hi - lo, i, nd};
}

__device__ __forceinline__ bool cl_keep_bit(const unsigned long long* keep_row, int64_t j) {
    return (keep_row[j >> 6] >> (j & 63)) & 1ull;
}

// ------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(CL_THREADS) void cl_fwd_kernel(const float* __restrict__ sim, const int64_t* __restrict__ docids,
                                                            const int64_t* __restrict__ rel_off, const int64_t* __restrict__ rel_ids,
                                                            int64_t R, int64_t nd, int64_t topk, const uint8_t* __restrict__ dup,
                                                            unsigned long long* __restrict__ keep, int64_t words,
                                                            double* __restrict__ stat, float* __restrict__ z_out) {
    __shared__ unsigned hist[256], s_scan[4], s_sel[2], s_mm[2], s_gt[CL_WAVES], s_eq[CL_WAVES];
    __shared__ int64_t s_rel[CL_REL_LDS];
    __shared__ float s_max[CL_WAVES];
    __shared__ double s_sum[CL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const cl_row row = cl_open_row(sim, docids, rel_off, rel_ids, R, nd, dup, s_rel);
    const int64_t i = row.i;
    const bool cut = topk > 0 && topk < nd;                                         // topk >= nd keeps every column
    unsigned long long* keep_row = keep + i * words;
    // wave wv owns the words [wa, wb): a contiguous quarter of the row, so "ascending j" is wave order, then word order
    const int64_t wq = (words + CL_WAVES - 1) / CL_WAVES;
    const int64_t wa = wv * wq < words ? wv * wq : words, wb = wa + wq < words ? wa + wq : words;

    unsigned T = 0u, need = 0u, before = 0u;
    if (cut) {
        T = adc_kth_largest([&](int64_t j) { return row.key_at(j); }, nd, (unsigned)topk, hist, s_scan, s_sel, s_mm);
        unsigned gt = 0u, eq = 0u;                                                  // wave-uniform counts
        for (int64_t w0 = wa; w0 < wb; w0 += CL_U) {
            unsigned k[CL_U];
            bool ok[CL_U];
#pragma unroll
            for (int u = 0; u < CL_U; ++u) {
                const int64_t j = (w0 + u) * CL_WORD + lane;
                ok[u] = w0 + u < wb && j < nd;
                k[u] = ok[u] ? row.key_at(j) : 0u;
            }
#pragma unroll
            for (int u = 0; u < CL_U; ++u) {
                gt += (unsigned)__popcll(__ballot(ok[u] && k[u] > T));
                eq += (unsigned)__popcll(__ballot(ok[u] && k[u] == T));
            }
        }
        if (lane == 0) { s_gt[wv] = gt; s_eq[wv] = eq; }
        __syncthreads();
        unsigned above = 0u;
        for (int w = 0; w < CL_WAVES; ++w) {
            above += s_gt[w];
            before += w < wv ? s_eq[w] : 0u;
        }
        need = (unsigned)topk - above;                                              // the T-th key exists: above < topk
    }

    // mark: keep bits, z_out, row maximum
    float mx = -INFINITY;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t w0 = wa; w0 < wb; w0 += CL_U) {
        float s[CL_U];
        int64_t d[CL_U];
        uint8_t du[CL_U];
#pragma unroll
        for (int u = 0; u < CL_U; ++u) {
            const int64_t j = (w0 + u) * CL_WORD + lane;
            const bool ok = w0 + u < wb && j < nd;
            s[u] = ok ? row.sim[j] : 0.f;
            d[u] = ok ? docids[j] : 0;
            du[u] = ok ? dup[j] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < CL_U; ++u) {
            if (w0 + u >= wb) break;                                                // wave-uniform
            const int64_t j = (w0 + u) * CL_WORD + lane;
            const bool ok = j < nd;
            const float z1 = row.z1(j, s[u], d[u], du[u]);
            bool kp = ok;
            if (cut) {
                const unsigned k = row.key(j, z1);
                const bool eq = ok && k == T;
                const unsigned long long m = __ballot(eq);
                const unsigned rank = before + (unsigned)__popcll(m & below);       // equal keys at a lower j
                kp = ok && (k > T || (eq && rank < need) || j == i);
                before += (unsigned)__popcll(m);
                const unsigned long long kb = __ballot(kp);
                if (lane == 0) keep_row[w0 + u] = kb;
            }
            const float z = kp ? z1 : z1 - 10000.0f;
            if (ok) {
                mx = fmaxf(mx, z);
                if (z_out) z_out[i * nd + j] = z;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) s_max[wv] = mx;
    __syncthreads();                                                                // also: the keep words are visible to the block
    mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    const double M = (double)mx;

    // sum over j != i: a thread adds its columns j = tid, tid + 256, ... in ascending j, the 64 lanes of a wave are added as a
    // butterfly, the four waves in order
    double acc = 0.0;
    for (int64_t j0 = tid; j0 < nd; j0 += (int64_t)CL_THREADS * CL_U) {
        float s[CL_U];
        int64_t d[CL_U];
        uint8_t du[CL_U];
        bool kp[CL_U];
#pragma unroll
        for (int u = 0; u < CL_U; ++u) {
            const int64_t j = j0 + (int64_t)u * CL_THREADS;
            const bool ok = j < nd;
            s[u] = ok ? row.sim[j] : 0.f;
            d[u] = ok ? docids[j] : 0;
            du[u] = ok ? dup[j] : (uint8_t)0;
            kp[u] = (ok && cut) ? cl_keep_bit(keep_row, j) : true;
        }
#pragma unroll
        for (int u = 0; u < CL_U; ++u) {
            const int64_t j = j0 + (int64_t)u * CL_THREADS;
            if (j < nd && j != i) {
                const float z1 = row.z1(j, s[u], d[u], du[u]);
                const float z = kp[u] ? z1 : z1 - 10000.0f;
                acc = acc + exp((double)z - M);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
    if (lane == 0) s_sum[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        const double off = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        const double zii = (double)row.sim[i];                                      // the label column: never masked, always kept
        const double sum = off + exp(zii - M);
        double* st = stat + i * CL_STAT;
        st[0] = M;
        st[1] = sum;
        st[2] = off;
        st[3] = (M + log(sum)) - zii;
    }
}

__global__ void cl_finish_kernel(const double* __restrict__ stat, int64_t nq, float* __restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    for (int64_t i0 = 0; i0 < nq; i0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + u < nq ? stat[(i0 + u) * CL_STAT + 3] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u < nq) acc = acc + v[u];
    }
    *loss = (float)(acc / (double)nq);
}

// ------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(CL_THREADS) void cl_bwd_kernel(const float* __restrict__ sim, const int64_t* __restrict__ docids,
                                                            const int64_t* __restrict__ rel_off, const int64_t* __restrict__ rel_ids,
                                                            int64_t R, int64_t nq, int64_t nd, int64_t topk,
                                                            const uint8_t* __restrict__ dup, const unsigned long long* __restrict__ keep,
                                                            int64_t words, const double* __restrict__ stat, const float* __restrict__ gout,
                                                            float* __restrict__ grad) {
    __shared__ int64_t s_rel[CL_REL_LDS];
    const int tid = threadIdx.x;
    const cl_row row = cl_open_row(sim, docids, rel_off, rel_ids, R, nd, dup, s_rel);
    const int64_t i = row.i;
    const bool cut = topk > 0 && topk < nd;
    const unsigned long long* keep_row = keep + i * words;
    const double M = stat[i * CL_STAT], sum = stat[i * CL_STAT + 1], off = stat[i * CL_STAT + 2];
    const double g = (double)gout[0], n = (double)nq;
    float* grow = grad + i * nd;
    for (int64_t j0 = tid; j0 < nd; j0 += (int64_t)CL_THREADS * CL_U) {
        float s[CL_U];
        int64_t d[CL_U];
        uint8_t du[CL_U];
        bool kp[CL_U];
#pragma unroll
        for (int u = 0; u < CL_U; ++u) {
            const int64_t j = j0 + (int64_t)u * CL_THREADS;
            const bool ok = j < nd;
            s[u] = ok ? row.sim[j] : 0.f;
            d[u] = ok ? docids[j] : 0;
            du[u] = ok ? dup[j] : (uint8_t)0;
            kp[u] = (ok && cut) ? cl_keep_bit(keep_row, j) : true;
        }
#pragma unroll
        for (int u = 0; u < CL_U; ++u) {
            const int64_t j = j0 + (int64_t)u * CL_THREADS;
            if (j >= nd) continue;
            const float z1 = row.z1(j, s[u], d[u], du[u]);
            const float z = kp[u] ? z1 : z1 - 10000.0f;
            const double v = (j == i) ? -(off / sum) : exp((double)z - M) / sum;    // the diagonal without cancellation
            grow[j] = (float)((g * v) / n);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- entry points
extern "C" size_t rc_contrastive_ws_bytes(int64_t nq, int64_t nd) {
    if (nq <= 0 || nd <= 0 || nq > nd || nd > CL_MAX_ND) return 0;
    return cl_ws(nq, nd).total;
}

static int cl_check(rc_handle_t h, const void* sim, const void* docids, const void* rel_off, const void* rel_ids, int64_t R, int64_t nq,
                    int64_t nd, int64_t topk, const void* ws, size_t ws_bytes) {
    if (!h || !sim || !docids || !rel_off || R < 0 || (R > 0 && !rel_ids)) return RC_EINVAL;
    if (nq <= 0 || nd <= 0 || nq > nd || nd > CL_MAX_ND || topk < 0 || topk > nd) return RC_EINVAL;
    if (!ws || ws_bytes < cl_ws(nq, nd).total) return RC_EWORKSPACE;
    return RC_OK;
}

extern "C" int rc_contrastive_fwd(rc_handle_t h, const float* sim, const int64_t* docids, const int64_t* rel_off, const int64_t* rel_ids,
                                  int64_t R, int64_t nq, int64_t nd, int64_t topk, float* loss, float* z_out, void* ws, size_t ws_bytes,
                                  rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int rc = cl_check(h, sim, docids, rel_off, rel_ids, R, nq, nd, topk, ws, ws_bytes);
    if (rc != RC_OK) return rc;
    if (!loss) return RC_EINVAL;
    const cl_ws L(nq, nd);
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cl_dup_kernel, dim3((unsigned)((nd + CL_DUP_COLS - 1) / CL_DUP_COLS)), dim3(CL_THREADS), 0, s, docids, nd,
                       (uint8_t*)(w + L.dup));
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(cl_fwd_kernel, dim3((unsigned)nq), dim3(CL_THREADS), 0, s, sim, docids, rel_off, rel_ids, R, nd, topk,
                       (const uint8_t*)(w + L.dup), (unsigned long long*)(w + L.keep), L.words, (double*)(w + L.stat), z_out);
    RC_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(cl_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)(w + L.stat), nq, loss);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

extern "C" int rc_contrastive_bwd(rc_handle_t h, const float* sim, const int64_t* docids, const int64_t* rel_off, const int64_t* rel_ids,
                                  int64_t R, int64_t nq, int64_t nd, int64_t topk, const float* gout, float* grad_sim, const void* ws,
                                  size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int rc = cl_check(h, sim, docids, rel_off, rel_ids, R, nq, nd, topk, ws, ws_bytes);
    if (rc != RC_OK) return rc;
    if (!gout || !grad_sim) return RC_EINVAL;
    const cl_ws L(nq, nd);
    const char* w = (const char*)ws;
    hipLaunchKernelGGL(cl_bwd_kernel, dim3((unsigned)nq), dim3(CL_THREADS), 0, (hipStream_t)stream, sim, docids, rel_off, rel_ids, R, nq,
                       nd, topk, (const uint8_t*)(w + L.dup), (const unsigned long long*)(w + L.keep), L.words,
                       (const double*)(w + L.stat), gout, grad_sim);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
