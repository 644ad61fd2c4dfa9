// Exact dense inner-product top-k search (Faiss IndexFlatIP, useFloat16 = False) — what step 3 of every recipe of the
// reference runs: models/dense/evaluate_dense.py:84-129 (create_index / dense_search / batch_dense_search).
//
// Score: s(q, n) = fmaf chain over d = 0 .. D-1 ascending from +0.0f, s = fmaf(q[d], x[n][d], s) — what
// v_mfma_f32_32x32x2_f32 computes when K is walked in ascending order through one accumulator (ivf_search.hip, coarse
// quantiser).  Results are therefore bit-defined (ids AND score bits), unlike Faiss's cuBLAS order.  D is zero-padded up
// to the K chunk of 16: bit-neutral, a chain that starts at +0 never holds -0 and fmaf(0, 0, s) = s.
//
// One GEMM kernel, dense_gemm_kernel<MODE, PAD>, with the structure of ivf_coarse_assign_kernel: a block owns 128 corpus rows
// and walks every tile of 128 queries (the queries stay cache-resident, the corpus is read from HBM once per launch); wave
// (wr, wc) owns 64 queries x 64 rows as 2 x 2 tiles of v_mfma_f32_32x32x2_f32, queries = rows of the MFMA result (a lane holds
// ONE corpus row and 16 queries per tile), K in chunks of 16 staged in LDS.  Epilogues:
//   DENSE_STORE   the scores themselves -> out[q][j] (the sample, and the exact route's full score rows)
//   DENSE_FILTER  the 64-bit key (ordered score << 32 | ~row) of every s >= thr[q] is appended to q's candidate list:
//                 one ballot per (tile, register), one global atomic per query and 32-row half-wave that has survivors
//
// Fast route (N > 4 S):
//   1. dense_gemm_kernel<STORE> over the strided sample j -> row j N / S, S = min(N, 32768) rows: the same chain
//   2. adc_threshold_kernel (topk.hip): thr[q] = the r-th best sample score, r by the ADC formula (rc_adc_sample_rank)
//   3. dense_gemm_kernel<FILTER> over all N rows
//   4. adc_select_kernel (rc_adc_launch_select): sort + emit; qstatus bit0 = fewer than min(k, N) candidates, bit1 = overflow
// Exact route (small N, and the queries the fast route gives up on): dense_gemm_kernel<STORE> writes the full score rows of a
// chunk of queries, then the 8-pass radix select over the 64-bit keys of rc_adc_search_exact (rc_adc_launch_exact_select).
// It terminates with the same answer for any content (all rows identical, k >= N, ...).
#include "topk.h"

#include <stdint.h>

typedef float dense_f32x16 __attribute__((ext_vector_type(16)));
#define DENSE_TILE 128
#define DENSE_KC 16
#define DENSE_LD (DENSE_KC + 1)
#define DENSE_STORE 0
#define DENSE_FILTER 1
#define DENSE_EXACT_MAX_N (4 * ADC_SAMPLE_MAX)      // up to here every call takes the exact route
#define DENSE_EXACT_SC_BYTES (256ull << 20)          // score rows of one exact round
#define DENSE_EXACT_QX_MAX 512

// grid: ceil(nrows / 128) blocks of 256 threads.  Logical row j in [0, nrows) is corpus row (smap ? j N / smap : j).
// x: [N, ldx] (16-byte aligned rows unless PAD), q: [nq, D] contiguous.  STORE: out [nq][nrows].  FILTER: thr [nq],
// cnt [nq] (zeroed), cand [nq][ADC_CAND_CAP].
template <int MODE, bool PAD>
__global__ __launch_bounds__(256) void dense_gemm_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int64_t nrows,
                                                         int64_t smap, const float* __restrict__ q, int nq, int D,
                                                         const float* __restrict__ thr, float* __restrict__ out,
                                                         unsigned* __restrict__ cnt, unsigned long long* __restrict__ cand) {
    __shared__ float sa[2][DENSE_TILE * DENSE_LD];     // query chunk   [128][16 (+1)]
    __shared__ float sb[2][DENSE_TILE * DENSE_LD];     // corpus chunk  [128][16 (+1)]
    __shared__ float s_thr[DENSE_TILE];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l & 31, half = l >> 5;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> (row = tid / 2, 8 consecutive k = (tid & 1) * 8)
    const int lrow = tid >> 1, lk = (tid & 1) * 8;
    const int64_t jl = (j0 + lrow < nrows) ? j0 + lrow : nrows - 1;
    const int64_t xrow = smap ? (int64_t)((uint64_t)jl * (uint64_t)N / (uint64_t)smap) : jl;
    const float* xp = x + xrow * ldx;
    const int nkc = (D + DENSE_KC - 1) / DENSE_KC;
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        const int qrow = (qt + lrow < nq) ? qt + lrow : nq - 1;
        const float* qp = q + (int64_t)qrow * D;
        if (MODE == DENSE_FILTER && tid < DENSE_TILE) s_thr[tid] = (qt + tid < nq) ? thr[qt + tid] : INFINITY;
        dense_f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        float ra[8], rb[8];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_KC + lk;
            if constexpr (PAD) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    ra[i] = (k0 + i < D) ? qp[k0 + i] : 0.f;
                    rb[i] = (k0 + i < D) ? xp[k0 + i] : 0.f;
                }
            } else {
                const float4* pa = reinterpret_cast<const float4*>(qp + k0);
                const float4* pb = reinterpret_cast<const float4*>(xp + k0);
                const float4 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
                ra[0] = a0.x; ra[1] = a0.y; ra[2] = a0.z; ra[3] = a0.w; ra[4] = a1.x; ra[5] = a1.y; ra[6] = a1.z; ra[7] = a1.w;
                rb[0] = b0.x; rb[1] = b0.y; rb[2] = b0.z; rb[3] = b0.w; rb[4] = b1.x; rb[5] = b1.y; rb[6] = b1.z; rb[7] = b1.w;
            }
        };
        auto sstore = [&](int buf) {
            float* da = &sa[buf][lrow * DENSE_LD + lk];
            float* db = &sb[buf][lrow * DENSE_LD + lk];
#pragma unroll
            for (int i = 0; i < 8; ++i) { da[i] = ra[i]; db[i] = rb[i]; }
        };
        // row tiles of A that hold only padding (small query sets): their MFMAs are skipped, wave-uniformly — a call with
        // <= 32 queries issues a quarter of the matrix work of a full tile and is bounded by the corpus read instead
        const bool act[2] = {qt + wr * 64 < nq, qt + wr * 64 + 32 < nq};
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
#pragma unroll
            for (int ks = 0; ks < DENSE_KC / 2; ++ks) {
                float fa[2], fb[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    fa[t] = sa[buf][(wr * 64 + t * 32 + col) * DENSE_LD + 2 * ks + half];   // A[i = col][k = half]
                    fb[t] = sb[buf][(wc * 64 + t * 32 + col) * DENSE_LD + 2 * ks + half];   // B[k = half][j = col]
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (act[a])
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        // epilogue: this lane's row of column tile b is j0 + wc*64 + b*32 + col; its 16 queries of row tile a are
        // qt + wr*64 + a*32 + (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + wc * 64 + b * 32 + col;
            const bool jv = j < nrows;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qo = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const int qi = qt + qo;
                    const float s = acc[a][b][r];
                    if constexpr (MODE == DENSE_STORE) {
                        if (jv && qi < nq) out[(int64_t)qi * nrows + j] = s;
                    } else {
                        const bool pass = jv && qi < nq && s >= s_thr[qo];
                        const unsigned long long m = __ballot(pass);
                        if (m) {                                       // wave-uniform; each half-wave is one query
                            const unsigned hm = half ? (unsigned)(m >> 32) : (unsigned)m;
                            const int lead = hm ? __builtin_ctz(hm) : 0;
                            unsigned base = 0;
                            if (hm && col == lead) base = atomicAdd(cnt + qi, (unsigned)__popc(hm));
                            base = __shfl(base, 32 * half + lead);
                            if (pass) {
                                const unsigned slot = base + (unsigned)__popc(hm & ((1u << col) - 1u));
                                if (slot < ADC_CAND_CAP)
                                    cand[(int64_t)qi * ADC_CAND_CAP + slot] = adc_exact_key(s, j);
                            }
                        }
                    }
                }
        }
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

template <int MODE>
static int dense_launch_gemm(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int64_t nrows, int64_t smap,
                             const float* q, int nq, int D, const float* thr, float* out, unsigned* cnt,
                             unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (D % DENSE_KC == 0)
        hipLaunchKernelGGL((dense_gemm_kernel<MODE, false>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr, out,
                           cnt, cand);
    else
        hipLaunchKernelGGL((dense_gemm_kernel<MODE, true>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr, out,
                           cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

static bool dense_exact_route(int64_t N) { return N <= DENSE_EXACT_MAX_N; }

struct dense_exact_layout { size_t sc; topk_exact_layout sel; int qx; };      // sel.total = bytes of the whole workspace
static dense_exact_layout dense_exact_ws(int64_t N, int nq) {
    dense_exact_layout L;
    int64_t qx = (int64_t)(DENSE_EXACT_SC_BYTES / ((uint64_t)N * sizeof(float)));
    if (qx < 1) qx = 1;
    if (qx > DENSE_EXACT_QX_MAX) qx = DENSE_EXACT_QX_MAX;
    if (qx > nq) qx = nq;
    L.qx = (int)qx;
    L.sc = 0;
    L.sel = topk_exact_ws(rc_align_up((size_t)qx * (size_t)N * sizeof(float), 256), L.qx);
    return L;
}

struct dense_fast_layout { size_t sample, thr, cnt, cand, total; int64_t S; };
static dense_fast_layout dense_fast_ws(int64_t N, int nq) {
    dense_fast_layout L;
    L.S = N < ADC_SAMPLE_MAX ? N : ADC_SAMPLE_MAX;
    size_t o = 0;
    L.sample = o; o += rc_align_up((size_t)nq * (size_t)L.S * sizeof(float), 256);
    L.thr = o;    o += rc_align_up((size_t)nq * sizeof(float), 256);
    L.cnt = o;    o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
    L.cand = o;   o += rc_align_up((size_t)nq * ADC_CAND_CAP * sizeof(unsigned long long), 256);
    L.total = o;
    return L;
}

// argument checks shared by both entries: shapes first (pure arithmetic), then pointers
static int dense_check(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                       const float* scores, const int64_t* ids) {
    if (N > 0xFFFFFFFFll || k > ADC_CAND_CAP / 2) return RC_ESHAPE;
    if (!h || !x || !q || !scores || !ids || N <= 0 || D <= 0 || nq < 0 || k <= 0 || ldx < D) return RC_EINVAL;
    if (D % DENSE_KC == 0 && (ldx % 4 != 0 || ((uintptr_t)x & 15u) || ((uintptr_t)q & 15u))) return RC_EINVAL;
    return RC_OK;
}

extern "C" size_t rc_dense_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    if (N <= 0 || N > 0xFFFFFFFFll || D <= 0 || nq <= 0 || k <= 0 || k > ADC_CAND_CAP / 2) return 0;
    return dense_exact_ws(N, nq).sel.total;
}

extern "C" size_t rc_dense_search_ws_bytes(int64_t N, int D, int nq, int k) {
    if (N <= 0 || N > 0xFFFFFFFFll || D <= 0 || nq <= 0 || k <= 0 || k > ADC_CAND_CAP / 2) return 0;
    return dense_exact_route(N) ? dense_exact_ws(N, nq).sel.total : dense_fast_ws(N, nq).total;
}

static int dense_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                       int64_t id_offset, float* scores, int64_t* ids, char* w, const dense_exact_layout& L, hipStream_t s) {
    float* sc = (float*)(w + L.sc);             // (the select's status word is never set: exactly min(k, N) keys are collected)
    for (int q0 = 0; q0 < nq; q0 += L.qx) {
        const int nx = nq - q0 < L.qx ? nq - q0 : L.qx;
        int rc = dense_launch_gemm<DENSE_STORE>(h, x, ldx, N, N, 0, q + (int64_t)q0 * D, nx, D, nullptr, sc, nullptr, nullptr, s);
        if (rc != RC_OK) return rc;
        rc = topk_exact_select(h, sc, N, nx, k, id_offset, w, L.sel, scores + (size_t)q0 * k, ids + (size_t)q0 * k, s);
        if (rc != RC_OK) return rc;
    }
    return RC_OK;
}

extern "C" int rc_dense_search_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                     int k, int64_t id_offset, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                                     rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int crc = dense_check(h, x, ldx, N, D, q, nq, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (nq == 0) return RC_OK;
    const dense_exact_layout L = dense_exact_ws(N, nq);
    if (!ws || ws_bytes < L.sel.total) return RC_EWORKSPACE;
    return dense_exact(h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, (char*)ws, L, (hipStream_t)stream);
}

extern "C" int rc_dense_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                                 int64_t id_offset, double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus,
                                 void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int crc = dense_check(h, x, ldx, N, D, q, nq, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (!status) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    if (!ws || ws_bytes < rc_dense_search_ws_bytes(N, D, nq, k)) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dense_exact_route(N)) return dense_exact(h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, (char*)ws, dense_exact_ws(N, nq), s);
    const dense_fast_layout L = dense_fast_ws(N, nq);
    char* w = (char*)ws;
    float* sample = (float*)(w + L.sample);
    float* thr = (float*)(w + L.thr);
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    int rc = dense_launch_gemm<DENSE_STORE>(h, x, ldx, N, L.S, L.S, q, nq, D, nullptr, sample, nullptr, nullptr, s);
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_threshold(h, sample, L.S, nq, rc_adc_sample_rank(N, L.S, k, sel_slack), thr, s);
    if (rc != RC_OK) return rc;
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    rc = dense_launch_gemm<DENSE_FILTER>(h, x, ldx, N, N, 0, q, nq, D, thr, nullptr, cnt, cand, s);
    if (rc != RC_OK) return rc;
    return rc_adc_launch_select(h, cand, cnt, nq, N, k, id_offset, scores, ids, status, s, qstatus);
}
