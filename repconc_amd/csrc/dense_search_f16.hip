// Exact dense inner-product top-k search over an fp16 corpus (Faiss IndexFlatIP with useFloat16 = True): the corpus is half
// the bytes of dense_search.hip's and the screen runs on the f16 matrix cores, 16x the fp32 matrix rate.
//
// Score: x and q are IEEE fp16; s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f over the widened values —
// the definition of dense_search.hip applied to x.float(), q.float().  A product of two fp16 values is exact in fp32, but
// the f16 matrix instruction sums the products of a K step in an order of its own: what it computes is a SCREEN, s~, never a result.
//
// Fast route (N > 131072):
//   1. dense_f16_gemm_kernel<STORE> over the strided sample (S = 32768 rows): s~ of the sample
//   2. adc_threshold_kernel (topk.hip): thr~[q] = the r-th best s~ of the sample (rc_adc_sample_rank)
//   3. dense_f16_gemm_kernel<FILTER> over all N rows: the key (s~, row) of every s~ >= thr~[q] -> q's candidate list
//   4. dense_f16_rescore_kernel: the score half of every candidate key is replaced by the chain, literal fmaf calls
//   5. adc_select_kernel (rc_adc_launch_select, unchanged): sort + emit; qstatus bit0 / bit1 as in dense_search.hip
//   6. dense_f16_certify_kernel: with t = the query's k-th exact score and
//          E_q = DENSE_F16_ERR_C * D_pad * 2^-24 * ||q||_2 * X,   X >= the largest row norm of the corpus, D_pad = D up to 16,
//      every |s~ - s| <= E_q (both are fp32 sums of the same D exact products: each errs by < D ulps of sum |q_d x_d|), so a
//      row outside the list has s~ < thr~, hence s < thr~ + E_q: if t >= thr~ + E_q (everything rounded upwards) no such row
//      can enter the top-k or tie with its last member and the answer is proven equal to the exact route's.  Otherwise
//      qstatus bit2, "not certified": the caller repeats the query with another slack or takes the exact route.
// Exact route (N <= 131072, and the queries the fast route gives up on): dense_gemm_kernel<STORE, PAD, _Float16>
// (dense_gemm.h) — the fp32 matrix cores over rows widened on load, i.e. the chain itself — then the radix select.
#include "dense_gemm.h"

#include <type_traits>

typedef _Float16 dense_f16x8 __attribute__((ext_vector_type(8)));
typedef float dense_f32x4 __attribute__((ext_vector_type(4)));
#define DENSE_F16_KC 64                                  // halves of K per LDS stage: 128-byte rows, 8 chunks of 16 bytes
#define DENSE_F16_OPERAND_BYTES (DENSE_TILE * DENSE_F16_KC * 2)
#define DENSE_F16_LDS_BYTES (4 * DENSE_F16_OPERAND_BYTES)                       // 2 operands x 2 buffers: 64 KB
#define DENSE_F16_ERR_C 4.0                              // the certificate's constant (rc_dense_f16_error_constant)
#define DENSE_F16_RESCORE_QCHUNK 1024                    // query values staged in LDS by the rescoring kernel
// The matrix instruction of the screen: 0 = v_mfma_f32_32x32x16_f16, 1 = v_mfma_f32_16x16x32_f16, both at 64 x 64 outputs per
// wave.  16x16x32 is the default: at 8 841 823 x 768 its FILTER launch takes 27.1 ms per ~1 163 queries against 28.0 ms, and a
// batch 35.9 ms against 36.9 ms (profiles/dense_f16_form_ab.txt).  -DDENSE_F16_SCREEN_16X16X32=0 builds the other.
#ifndef DENSE_F16_SCREEN_16X16X32
#define DENSE_F16_SCREEN_16X16X32 1
#endif

// byte offset of the 16-byte chunk c (k = 8c .. 8c+7 of the stage) of tile row `row`: XOR swizzle with (row / 2) % 8.  Two
// rows share 256 bytes = all 64 banks.  32x32x16: a ds_read_b128 is served in groups of 16 lanes that hold rows {0-3, 12-15,
// 20-27} or {4-11, 16-19, 28-31} of one chunk index, and within either group the 8 even and the 8 odd rows have 8 different
// row / 2 % 8.  16x16x32: any 16 lanes that hold 16 consecutive rows of one chunk index cover all 64 banks once.
__device__ __forceinline__ int dense_f16_lds_off(int row, int c) { return row * (DENSE_F16_KC * 2) + ((c ^ ((row >> 1) & 7)) << 4); }

// grid: ceil(nrows / 128) blocks of 256 threads, two per CU (64 KB of LDS each).  Arguments as dense_gemm_kernel; x and q are
// fp16.  !PAD: D % 8 == 0, 16-byte aligned rows; PAD assembles its chunks element by element (189 - 212 vector registers over
// the M16 instantiations, 176 - 228 over the others, no scratch; the FILTER ones keep a few scalars in vector lanes).  The block owns 128 corpus
// rows and walks every tile of 128 queries; wave (wr, wc) owns 64 queries x 64 rows as NT x NT tiles of TM x TM:
//   !M16: 2 x 2 of v_mfma_f32_32x32x16_f16, lane l holds k = 8 (l / 32) .. + 7 of row l % 32 of both operands,
//    M16: 4 x 4 of v_mfma_f32_16x16x32_f16, lane l holds k = 8 (l / 16) .. + 7 of row l % 16 of both operands
// (one 16-byte LDS read per operand tile and K step).  Result element r of lane l is corpus row l % TM and query
// (r & 3) + 8 (r >> 2) + 4 (l / 32) of the tile (!M16) or 4 (l / 16) + r (M16); dense_emit is the epilogue of both.
template <int MODE, bool PAD, bool M16>
__global__ __launch_bounds__(256, 2) void dense_f16_gemm_kernel(const _Float16* __restrict__ x, int64_t ldx, int64_t N,
                                                             int64_t nrows, int64_t smap, const _Float16* __restrict__ q,
                                                             int nq, int D, const float* __restrict__ thr,
                                                             float* __restrict__ out, unsigned* __restrict__ cnt,
                                                             unsigned long long* __restrict__ cand) {
    constexpr int TM = M16 ? 16 : 32, NT = 64 / TM, KS = M16 ? 32 : 16, NR = M16 ? 4 : 16;
    using acc_t = std::conditional_t<M16, dense_f32x4, dense_f32x16>;
    __shared__ __attribute__((aligned(16))) unsigned char dense_f16_smem[DENSE_F16_LDS_BYTES];
    unsigned char* sa = dense_f16_smem;                                     // [2][128 rows][128 bytes] queries
    unsigned char* sb = dense_f16_smem + 2 * DENSE_F16_OPERAND_BYTES;       // [2][128 rows][128 bytes] corpus
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l % TM, grp = l / TM;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> chunk lc = tid % 8 of rows tid / 8 + 32 i, i < 4 (8 threads read 128 contiguous bytes of a row)
    const int lrow = tid >> 3, lc = tid & 7;
    const _Float16* xp[4];
    int so[4];                                                             // swizzled LDS offsets of the four chunks
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t jl = (j0 + lrow + 32 * i < nrows) ? j0 + lrow + 32 * i : nrows - 1;
        const int64_t xrow = smap ? (int64_t)((uint64_t)jl * (uint64_t)N / (uint64_t)smap) : jl;
        xp[i] = x + xrow * ldx;
        so[i] = dense_f16_lds_off(lrow + 32 * i, lc);
    }
    const int nkc = (D + DENSE_F16_KC - 1) / DENSE_F16_KC;
    // the thresholds of a query tile go where the operand buffer that the last K stage did not read lies
    float* s_thr = reinterpret_cast<float*>(sa + (nkc & 1) * DENSE_F16_OPERAND_BYTES);
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        const _Float16* qp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qp[i] = q + (int64_t)((qt + lrow + 32 * i < nq) ? qt + lrow + 32 * i : nq - 1) * D;
        acc_t acc[NT][NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[a][b][r] = 0.f;
        dense_f16x8 ra[4], rb[4];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_F16_KC + lc * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (PAD) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        ra[i][e] = (k0 + e < D) ? qp[i][k0 + e] : (_Float16)0;
                        rb[i][e] = (k0 + e < D) ? xp[i][k0 + e] : (_Float16)0;
                    }
                } else if (k0 < D) {                                        // D % 8 == 0: a chunk is inside or outside
                    ra[i] = *reinterpret_cast<const dense_f16x8*>(qp[i] + k0);
                    rb[i] = *reinterpret_cast<const dense_f16x8*>(xp[i] + k0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { ra[i][e] = (_Float16)0; rb[i][e] = (_Float16)0; }
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<dense_f16x8*>(sa + buf * DENSE_F16_OPERAND_BYTES + so[i]) = ra[i];
                *reinterpret_cast<dense_f16x8*>(sb + buf * DENSE_F16_OPERAND_BYTES + so[i]) = rb[i];
            }
        };
        // query tiles that hold only padding skip their MFMAs, wave-uniformly (a call with <= 32 queries issues a quarter of
        // the matrix work and is bounded by the corpus read)
        bool act[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) act[a] = qt + wr * 64 + a * TM < nq;
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
            const unsigned char* pa = sa + buf * DENSE_F16_OPERAND_BYTES;
            const unsigned char* pb = sb + buf * DENSE_F16_OPERAND_BYTES;
#pragma unroll
            for (int ks = 0; ks < DENSE_F16_KC / KS; ++ks) {
                dense_f16x8 fa[NT], fb[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    fa[t] = *reinterpret_cast<const dense_f16x8*>(pa + dense_f16_lds_off(wr * 64 + t * TM + col, (KS / 8) * ks + grp));
                    fb[t] = *reinterpret_cast<const dense_f16x8*>(pb + dense_f16_lds_off(wc * 64 + t * TM + col, (KS / 8) * ks + grp));
                }
#pragma unroll
                for (int a = 0; a < NT; ++a)
                    if (act[a])
#pragma unroll
                        for (int b = 0; b < NT; ++b) {
                            if constexpr (M16) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
                            else acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
                        }
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        if constexpr (MODE == DENSE_FILTER) {
            if (tid < DENSE_TILE) s_thr[tid] = (qt + tid < nq) ? thr[qt + tid] : INFINITY;
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int64_t j = j0 + wc * 64 + b * TM + col;
            const bool jv = j < nrows;
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const int qo = wr * 64 + a * TM + (M16 ? 4 * grp + r : (r & 3) + 8 * (r >> 2) + 4 * grp);
                    dense_emit<MODE, TM>(acc[a][b][r], j, jv, qt + qo, nq, MODE == DENSE_FILTER ? s_thr[qo] : 0.f, nrows, out, cnt,
                                         cand, l);
                }
        }
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

// grid: (nq, ADC_CAND_CAP / 256) blocks of 256 threads; one lane per candidate key of query blockIdx.x.  The key's score half
// (the screen's s~) is replaced by the chain: literal fmaf calls, d ascending, one accumulator.  VEC: 16-byte aligned rows.
template <bool VEC>
__global__ __launch_bounds__(256) void dense_f16_rescore_kernel(const _Float16* __restrict__ x, int64_t ldx, int D,
                                                                const _Float16* __restrict__ q,
                                                                const unsigned* __restrict__ cnt,
                                                                unsigned long long* __restrict__ cand) {
    __shared__ float sq[DENSE_F16_RESCORE_QCHUNK];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const unsigned raw = cnt[qi];
    const unsigned n = raw > ADC_CAND_CAP ? ADC_CAND_CAP : raw;
    if (blockIdx.y * 256u >= n) return;                                // block-uniform
    const unsigned i = blockIdx.y * 256u + tid;
    const bool mine = i < n;
    unsigned long long* kp = cand + (size_t)qi * ADC_CAND_CAP + i;
    const unsigned row = mine ? 0xFFFFFFFFu - (unsigned)(*kp & 0xFFFFFFFFull) : 0u;
    const _Float16* xp = x + (int64_t)row * ldx;
    const _Float16* qp = q + (int64_t)qi * D;
    float s = 0.f;
    for (int d0 = 0; d0 < D; d0 += DENSE_F16_RESCORE_QCHUNK) {
        const int dn = D - d0 < DENSE_F16_RESCORE_QCHUNK ? D - d0 : DENSE_F16_RESCORE_QCHUNK;
        __syncthreads();
        for (int d = tid; d < dn; d += 256) sq[d] = (float)qp[d0 + d];
        __syncthreads();
        if (mine) {
            int d = 0;
            if constexpr (VEC) {
                for (; d + 8 <= dn; d += 8) {
                    const dense_f16x8 v = *reinterpret_cast<const dense_f16x8*>(xp + d0 + d);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = __builtin_fmaf(sq[d + e], (float)v[e], s);
                }
            }
            for (; d < dn; ++d) s = __builtin_fmaf(sq[d], (float)xp[d0 + d], s);
        }
    }
    if (mine) *kp = adc_exact_key(s, (int64_t)row);
}

// grid: nq blocks of 64 threads.  Sets bit2 of status / qstatus[q] unless t >= thr~ + E_q is proven (header comment): the norm,
// E_q and the sum are evaluated in fp64 and pushed upwards by more than their rounding errors; a NaN anywhere is "not certified".
__global__ __launch_bounds__(64) void dense_f16_certify_kernel(const _Float16* __restrict__ q, int D, int k,
                                                               const float* __restrict__ thr,
                                                               const float* __restrict__ xnorm_max,
                                                               const float* __restrict__ scores, int* __restrict__ status,
                                                               int* __restrict__ qstatus) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    const _Float16* qp = q + (int64_t)qi * D;
    double ss = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)(float)qp[d];
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane != 0) return;
    const double up = 1.0 + 0x1p-30;
    const int dpad = (D + 15) / 16 * 16;
    const double eq = DENSE_F16_ERR_C * (double)dpad * 0x1p-24 * (sqrt(ss) * up) * (double)xnorm_max[0] * up;
    const double sum = (double)thr[qi] + eq;
    const double bound = sum + fabs(sum) * 0x1p-30;
    const double t = (double)scores[(size_t)qi * k + (k - 1)];
    if (!(t >= bound)) {
        atomicOr(status, 4);
        if (qstatus) atomicOr(qstatus + qi, 4);
    }
}

static bool dense_f16_aligned(const void* x, int64_t ldx, const void* q, int D) {
    return D % 8 == 0 && ldx % 8 == 0 && !((uintptr_t)x & 15u) && !((uintptr_t)q & 15u);
}

template <int MODE>
static int dense_f16_launch_gemm(rc_handle_t h, const _Float16* x, int64_t ldx, int64_t N, int64_t nrows, int64_t smap,
                                 const _Float16* q, int nq, int D, const float* thr, float* out, unsigned* cnt,
                                 unsigned long long* cand, hipStream_t s) {
    constexpr bool M16 = DENSE_F16_SCREEN_16X16X32 != 0;
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (dense_f16_aligned(x, ldx, q, D))
        hipLaunchKernelGGL((dense_f16_gemm_kernel<MODE, false, M16>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand);
    else
        hipLaunchKernelGGL((dense_f16_gemm_kernel<MODE, true, M16>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

extern "C" double rc_dense_f16_error_constant(void) { return DENSE_F16_ERR_C; }
extern "C" int rc_dense_f16_screen_form(void) { return DENSE_F16_SCREEN_16X16X32 ? 16 : 32; }

extern "C" size_t rc_dense_f16_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_shape_ok(N, D, nq, k) ? dense_exact_ws(N, nq).sel.total : 0;
}

extern "C" size_t rc_dense_f16_search_ws_bytes(int64_t N, int D, int nq, int k) {
    if (!dense_shape_ok(N, D, nq, k)) return 0;
    return dense_exact_route(N) ? dense_exact_ws(N, nq).sel.total : dense_fast_ws(N, nq).total;
}

extern "C" int rc_dense_f16_search_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                         int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                         size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const _Float16* xh = reinterpret_cast<const _Float16*>(x);
    const _Float16* qh = reinterpret_cast<const _Float16*>(q);
    const int crc = dense_check(h, xh, ldx, N, D, qh, nq, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (nq == 0) return RC_OK;
    const dense_exact_layout L = dense_exact_ws(N, nq);
    if (!ws || ws_bytes < L.sel.total) return RC_EWORKSPACE;
    return dense_exact(h, xh, ldx, N, D, qh, nq, k, id_offset, scores, ids, (char*)ws, L, (hipStream_t)stream);
}

extern "C" int rc_dense_f16_scores(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                   float* out, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll) return RC_ESHAPE;
    if (!h || !x || !q || !out || N <= 0 || D <= 0 || nq < 0 || ldx < D) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    return dense_f16_launch_gemm<DENSE_STORE>(h, reinterpret_cast<const _Float16*>(x), ldx, N, N, 0,
                                              reinterpret_cast<const _Float16*>(q), nq, D, nullptr, out, nullptr, nullptr,
                                              (hipStream_t)stream);
}

extern "C" int rc_dense_f16_search_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                     const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores,
                                     int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const _Float16* xh = reinterpret_cast<const _Float16*>(x);
    const _Float16* qh = reinterpret_cast<const _Float16*>(q);
    const int crc = dense_check(h, xh, ldx, N, D, qh, nq, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (!status || !xnorm_max) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    if (!ws || ws_bytes < rc_dense_f16_search_ws_bytes(N, D, nq, k)) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dense_exact_route(N)) return dense_exact(h, xh, ldx, N, D, qh, nq, k, id_offset, scores, ids, (char*)ws, dense_exact_ws(N, nq), s);
    const dense_fast_layout L = dense_fast_ws(N, nq);
    char* w = (char*)ws;
    float* sample = (float*)(w + L.sample);
    float* thr = (float*)(w + L.thr);
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    int rc = dense_f16_launch_gemm<DENSE_STORE>(h, xh, ldx, N, L.S, L.S, qh, nq, D, nullptr, sample, nullptr, nullptr, s);
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_threshold(h, sample, L.S, nq, rc_adc_sample_rank(N, L.S, k, sel_slack), thr, s);
    if (rc != RC_OK) return rc;
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    rc = dense_f16_launch_gemm<DENSE_FILTER>(h, xh, ldx, N, N, 0, qh, nq, D, thr, nullptr, cnt, cand, s);
    if (rc != RC_OK) return rc;
    const dim3 rgrid((unsigned)nq, ADC_CAND_CAP / 256);
    if (ldx % 8 == 0 && !((uintptr_t)x & 15u))
        hipLaunchKernelGGL(dense_f16_rescore_kernel<true>, rgrid, dim3(256), 0, s, xh, ldx, D, qh, cnt, cand);
    else
        hipLaunchKernelGGL(dense_f16_rescore_kernel<false>, rgrid, dim3(256), 0, s, xh, ldx, D, qh, cnt, cand);
    RC_LAUNCH_CHECK(h);
    rc = rc_adc_launch_select(h, cand, cnt, nq, N, k, id_offset, scores, ids, status, s, qstatus);
    if (rc != RC_OK) return rc;
    hipLaunchKernelGGL(dense_f16_certify_kernel, dim3((unsigned)nq), dim3(64), 0, s, qh, D, k, thr, xnorm_max, scores, status,
                       qstatus);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
