// Exact re-ranking of candidate lists against a dense store (Faiss IndexRefineFlat's second stage): the candidates come from
// outside — a PQ or IVF search — instead of from one of the dense screens, and only their rows are scored.
//
// Score: what the dense searches define for the (query, row) pair, bit for bit: one fp32 accumulator from +0.0f, d ascending,
// dense_chain_step<L2> over the values widened to fp32 (inner product: s = fmaf(q_d, x_d, s); L2: t = q_d - x_d,
// s = fmaf(t, t, s)).  Every stage works on s, or on -d for L2, and the L2 finish of the dense searches (dense_l2_launch_negate)
// turns the k output values into distances: +0.0f for a zero, +inf for the padding.
//
// Stages, all on the caller's stream:
//   1. dense_rerank_kernel / dense_rerank_rows_kernel: candidate c of query i is valid iff 0 <= c - id_offset < N; a valid
//      one is scored and its key adc_exact_key(score, c - id_offset) appended to cand[i][ADC_CAND_CAP], the number of keys
//      goes to cnt[i] (one atomic per wave on the counter, none on a value: the list's order varies, its content does not, and
//      the sort makes the output the same from run to run).  A list is a multiset: an id given twice yields two equal keys.
//   2. rc_adc_launch_select: sort + emit the min(k, cnt[i]) best, (-inf, -1) after them.  Its "fewer than min(k, N)
//      candidates" bit lands in a status word of the workspace that nobody reads: here it is no error.
//   3. L2: the negation.
//
// dense_rerank_kernel (16-byte aligned rows whose pitch is a multiple of 16 bytes).  The chain's fixed order leaves one
// accumulator per candidate, so a wave owns 64 candidates of one query, one per lane — and a lane that read its own row would
// touch 64 rows with every load instruction.  Instead the wave walks D in slices of DENSE_RERANK_SLICE bytes and loads the 64
// slices cooperatively: lane l of load j takes piece l % P of the row of lane j (64 / P) + l / P (P = 16-byte pieces per
// slice), so one instruction covers 64 / P whole slices of 128 (256) contiguous bytes.  The pieces wait in registers while the
// previous slice is computed and are then stored to the wave's own LDS tile with a row stride of SLICE + 16 bytes: 16
// consecutive rows lie on 16 distinct 4-bank groups (36 r mod 64 = 4 (9 r mod 16)), the quarter-wave rule of ds_read_b128
// (dense_screen_lds_off), so lane r reads row r back without conflicts.  The tile is private to the wave: the loop has no
// block barrier, only the wave's own ordering of its LDS stores and loads.  The query's values are staged per block,
// DENSE_RESCORE_QCHUNK at a time, and read as broadcasts.  Invalid lanes of a wave that has valid ones point at the wave's
// first valid row (no access outside the store, no extra traffic); a wave without valid lanes only joins the barriers.
//   LDS: 4 waves x 64 x (SLICE + 16) + 4 KiB = 40 KiB at 128-byte slices, four blocks per CU; 72 KiB at 256, two.
// dense_rerank_rows_kernel: one lane per row, dense_rescore_kernel's loop.  The path of a store whose rows are not 16-byte
// aligned (VEC = false), and with -DDENSE_RERANK_LANE_PER_ROW the A/B form of the aligned ones (VEC = true).
#include "dense_l2.h"

#ifndef DENSE_RERANK_SLICE
#define DENSE_RERANK_SLICE 128                           // bytes of a row per stage: 128 or 256
#endif
#define DENSE_RERANK_PIECES (DENSE_RERANK_SLICE / 16)    // 16-byte pieces of a slice = load instructions per stage
#define DENSE_RERANK_STRIDE (DENSE_RERANK_SLICE + 16)    // bytes between two rows of the LDS tile
#define DENSE_RERANK_TILE (64 * DENSE_RERANK_STRIDE)     // one wave's tile
static_assert(DENSE_RERANK_SLICE == 128 || DENSE_RERANK_SLICE == 256, "a slice is 128 or 256 bytes");

typedef unsigned dense_rerank_u4 __attribute__((ext_vector_type(4)));

// candidate i of query qi: valid iff 0 <= c - id_offset < N (unsigned: one comparison); row = c - id_offset
__device__ __forceinline__ bool dense_rerank_row(const int64_t* __restrict__ ids, int64_t ldc, int kc, int qi, int i,
                                                 int64_t id_offset, int64_t N, unsigned* row) {
    *row = 0u;
    if (i >= kc) return false;
    const uint64_t r = (uint64_t)ids[(int64_t)qi * ldc + i] - (uint64_t)id_offset;
    if (r >= (uint64_t)N) return false;
    *row = (unsigned)r;
    return true;
}

// the key of every valid lane joins the query's list; called by whole waves
template <bool L2>
__device__ __forceinline__ void dense_rerank_append(bool valid, float s, unsigned row, int qi, unsigned* __restrict__ cnt,
                                                    unsigned long long* __restrict__ cand) {
    const unsigned long long m = __ballot(valid);
    if (!m) return;                                                    // wave-uniform
    const unsigned slot = adc_wave_append(m, cnt + qi);                // < the query's valid candidates <= kc <= ADC_CAND_CAP
    if (valid) cand[(size_t)qi * ADC_CAND_CAP + slot] = adc_exact_key(L2 ? -s : s, (int64_t)row);
}

// the wave's LDS stores become visible to its own later loads (the tile is private to the wave: no block barrier)
__device__ __forceinline__ void dense_rerank_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grid: (nq, ceil(kc / 256)) blocks of 256 threads.  x: [N, ldx], rows 16-byte aligned, ldx sizeof(T) % 16 == 0; q: [nq, D];
// ids: [nq, ldc]; cnt [nq] zeroed; cand [nq][ADC_CAND_CAP].
template <typename T, bool L2>
__global__ __launch_bounds__(256) void dense_rerank_kernel(const T* __restrict__ x, int64_t ldx, int64_t N, int D,
                                                           const T* __restrict__ q, const int64_t* __restrict__ ids,
                                                           int64_t ldc, int kc, int64_t id_offset,
                                                           unsigned* __restrict__ cnt, unsigned long long* __restrict__ cand) {
    constexpr int P = DENSE_RERANK_PIECES, RPL = 64 / P;               // rows per load instruction
    constexpr int EPP = 16 / (int)sizeof(T), EPS = DENSE_RERANK_SLICE / (int)sizeof(T);   // elements per piece, per slice
    __shared__ float sq[DENSE_RESCORE_QCHUNK];
    __shared__ __attribute__((aligned(16))) unsigned char sx[4 * DENSE_RERANK_TILE];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned row;
    const bool valid = dense_rerank_row(ids, ldc, kc, qi, (int)blockIdx.y * 256 + tid, id_offset, N, &row);
    const unsigned long long vm = __ballot(valid);
    const bool active = vm != 0ull;                                    // wave-uniform
    const unsigned lrow = (unsigned)__shfl((int)row, active ? (int)__builtin_ctzll(vm) : 0);
    if (!valid) row = lrow;                                            // a row of the store whenever the wave is active
    // this lane's part in the P loads of a stage: piece `pc` of the rows of lanes j RPL + lane / P
    const int pc = lane % P;
    const unsigned char* src[P];
#pragma unroll
    for (int j = 0; j < P; ++j)
        src[j] = reinterpret_cast<const unsigned char*>(x + (int64_t)(unsigned)__shfl((int)row, j * RPL + lane / P) * ldx) + pc * 16;
    unsigned char* tile = sx + wv * DENSE_RERANK_TILE;
    unsigned char* dst = tile + (lane / P) * DENSE_RERANK_STRIDE + pc * 16;       // + j RPL STRIDE
    const unsigned char* mine = tile + lane * DENSE_RERANK_STRIDE;
    const T* qp = q + (int64_t)qi * D;
    const int nst = (D + EPS - 1) / EPS;                               // stages
    dense_rerank_u4 stg[P];
    // the pieces of stage c: whole pieces inside the row with one 16-byte load, the piece that D cuts element by element
    // (what follows D in the last row of a store need not exist), nothing past it
    auto gload = [&](int c) {
        const int e0 = c * EPS + pc * EPP;                             // first element of this lane's piece
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const unsigned char* p = src[j] + (int64_t)c * DENSE_RERANK_SLICE;
            if (e0 + EPP <= D) {
                stg[j] = *reinterpret_cast<const dense_rerank_u4*>(p);
            } else {
                union { dense_rerank_u4 v; T e[EPP]; } u;
                u.v = dense_rerank_u4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < EPP; ++e)
                    if (e0 + e < D) u.e[e] = reinterpret_cast<const T*>(p)[e];
                stg[j] = u.v;
            }
        }
    };
    float s = 0.f;
    if (active) gload(0);
    for (int d0 = 0; d0 < D; d0 += DENSE_RESCORE_QCHUNK) {
        const int dn = D - d0 < DENSE_RESCORE_QCHUNK ? D - d0 : DENSE_RESCORE_QCHUNK;
        __syncthreads();
        for (int d = tid; d < dn; d += 256) sq[d] = (float)qp[d0 + d];
        __syncthreads();
        if (!active) continue;                                         // wave-uniform; the barriers above are the block's only ones
        const int c0 = d0 / EPS, c1 = (d0 + dn + EPS - 1) / EPS;
        for (int c = c0; c < c1; ++c) {
#pragma unroll
            for (int j = 0; j < P; ++j) *reinterpret_cast<dense_rerank_u4*>(dst + j * RPL * DENSE_RERANK_STRIDE) = stg[j];
            if (c + 1 < nst) gload(c + 1);                             // in flight while this stage is computed
            dense_rerank_wave_sync();
            const float* qs = sq + (c * EPS - d0);
            const int ne = D - c * EPS;
            if (ne >= EPS) {
#pragma unroll
                for (int g = 0; g < EPS / 8; ++g) {
                    float v[8];
                    dense_load8(reinterpret_cast<const T*>(mine) + 8 * g, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = dense_chain_step<L2>(qs[8 * g + e], v[e], s);
                }
            } else {
                for (int e = 0; e < ne; ++e) s = dense_chain_step<L2>(qs[e], (float)reinterpret_cast<const T*>(mine)[e], s);
            }
            dense_rerank_wave_sync();                                  // the next stage's stores overwrite the tile
        }
    }
    dense_rerank_append<L2>(valid, s, row, qi, cnt, cand);
}

// The same result with one lane per candidate row, the loop of dense_rescore_kernel.  VEC: 16-byte aligned rows.
template <bool VEC, typename T, bool L2>
__global__ __launch_bounds__(256) void dense_rerank_rows_kernel(const T* __restrict__ x, int64_t ldx, int64_t N, int D,
                                                                const T* __restrict__ q, const int64_t* __restrict__ ids,
                                                                int64_t ldc, int kc, int64_t id_offset,
                                                                unsigned* __restrict__ cnt,
                                                                unsigned long long* __restrict__ cand) {
    __shared__ float sq[DENSE_RESCORE_QCHUNK];
    const int qi = blockIdx.x, tid = threadIdx.x;
    unsigned row;
    const bool valid = dense_rerank_row(ids, ldc, kc, qi, (int)blockIdx.y * 256 + tid, id_offset, N, &row);
    const T* xp = x + (int64_t)row * ldx;
    const T* qp = q + (int64_t)qi * D;
    float s = 0.f;
    for (int d0 = 0; d0 < D; d0 += DENSE_RESCORE_QCHUNK) {
        const int dn = D - d0 < DENSE_RESCORE_QCHUNK ? D - d0 : DENSE_RESCORE_QCHUNK;
        __syncthreads();
        for (int d = tid; d < dn; d += 256) sq[d] = (float)qp[d0 + d];
        __syncthreads();
        if (valid) {
            int d = 0;
            if constexpr (VEC) {
                for (; d + 8 <= dn; d += 8) {
                    float v[8];
                    dense_load8(xp + d0 + d, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = dense_chain_step<L2>(sq[d + e], v[e], s);
                }
            }
            for (; d < dn; ++d) s = dense_chain_step<L2>(sq[d], (float)xp[d0 + d], s);
        }
    }
    dense_rerank_append<L2>(valid, s, row, qi, cnt, cand);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct dense_rerank_layout { size_t cnt, cand, status, total; };
static inline dense_rerank_layout dense_rerank_ws(int nq) {
    dense_rerank_layout L;
    size_t o = 0;
    L.cnt = o;    o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
    L.cand = o;   o += rc_align_up((size_t)nq * ADC_CAND_CAP * sizeof(unsigned long long), 256);
    L.status = o; o += 256;
    L.total = o;
    return L;
}

template <typename T, bool L2>
static int dense_rerank_launch(rc_handle_t h, const T* x, int64_t ldx, int64_t N, int D, const T* q, int nq, const int64_t* ids,
                               int64_t ldc, int kc, int64_t id_offset, unsigned* cnt, unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)nq, (unsigned)((kc + 255) / 256));
    const bool aligned = (ldx * (int64_t)sizeof(T)) % 16 == 0 && !((uintptr_t)x & 15u);
#ifdef DENSE_RERANK_LANE_PER_ROW
    if (aligned)
        hipLaunchKernelGGL((dense_rerank_rows_kernel<true, T, L2>), grid, dim3(256), 0, s, x, ldx, N, D, q, ids, ldc, kc, id_offset,
                           cnt, cand);
#else
    if (aligned)
        hipLaunchKernelGGL((dense_rerank_kernel<T, L2>), grid, dim3(256), 0, s, x, ldx, N, D, q, ids, ldc, kc, id_offset, cnt,
                           cand);
#endif
    else
        hipLaunchKernelGGL((dense_rerank_rows_kernel<false, T, L2>), grid, dim3(256), 0, s, x, ldx, N, D, q, ids, ldc, kc, id_offset,
                           cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// The body of both entries.  Order of the checks: shapes (pure arithmetic), pointers, the nq == 0 success, the workspace.
template <typename T>
static int dense_rerank_entry(rc_handle_t h, const T* x, int64_t ldx, int64_t N, int D, const T* q, int nq, const int64_t* ids_in,
                              int64_t ldc, int kc, int k, int64_t id_offset, int metric, float* scores, int64_t* ids, void* ws,
                              size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll || k > ADC_CAND_CAP / 2 || kc > ADC_CAND_CAP || (metric != 0 && metric != 1)) return RC_ESHAPE;
    if (!h || !q || !ids_in || !scores || !ids || N < 0 || (N > 0 && !x) || D <= 0 || nq < 0 || k <= 0 || kc <= 0 || ldx < D ||
        ldc < kc)
        return RC_EINVAL;
    if (nq == 0) return RC_OK;
    const dense_rerank_layout L = dense_rerank_ws(nq);
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < L.total) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned* cnt = (unsigned*)((char*)ws + L.cnt);
    unsigned long long* cand = (unsigned long long*)((char*)ws + L.cand);
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    // N == 0: no candidate is valid, nothing is read from x, every output slot is padding
    int rc = metric ? dense_rerank_launch<T, true>(h, x, ldx, N, D, q, nq, ids_in, ldc, kc, id_offset, cnt, cand, s)
                    : dense_rerank_launch<T, false>(h, x, ldx, N, D, q, nq, ids_in, ldc, kc, id_offset, cnt, cand, s);
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_select(h, cand, cnt, nq, N, k, id_offset, scores, ids, (int*)((char*)ws + L.status), s);
    if (rc != RC_OK) return rc;
    return metric ? dense_l2_launch_negate(h, scores, (int64_t)nq * k, s) : RC_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" size_t rc_dense_rerank_ws_bytes(int nq, int kc) {
    return nq > 0 && kc > 0 && kc <= ADC_CAND_CAP ? dense_rerank_ws(nq).total : 0;
}

extern "C" int rc_dense_rerank(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                               const int64_t* cand, int64_t ldc, int kc, int k, int64_t id_offset, int metric, float* scores,
                               int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_rerank_entry<float>(h, x, ldx, N, D, q, nq, cand, ldc, kc, k, id_offset, metric, scores, ids, ws, ws_bytes, stream);
}

extern "C" int rc_dense_f16_rerank(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                   const int64_t* cand, int64_t ldc, int kc, int k, int64_t id_offset, int metric, float* scores,
                                   int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_rerank_entry<_Float16>(h, reinterpret_cast<const _Float16*>(x), ldx, N, D, reinterpret_cast<const _Float16*>(q), nq,
                                        cand, ldc, kc, k, id_offset, metric, scores, ids, ws, ws_bytes, stream);
}
