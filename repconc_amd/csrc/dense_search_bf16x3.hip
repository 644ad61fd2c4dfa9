// Exact dense inner-product top-k search over an fp32 corpus with a bf16x3 matrix-core screen: the results of
// dense_search.hip (ids AND score bits of rc_dense_search_q), the corpus stays fp32, only the screen leaves the fp32 matrix
// cores.  The route is dense_search_route (dense_screen.h) with this unit's variant: dense_bf16x3_split_kernel is its query
// pre-pass, dense_bf16x3_gemm_kernel screens, the candidates are rescored by the chain and every answer carries a certificate
// with the E_q derived below.  Exact route: the rows of dense_exact_rows_f32 (dense_search.hip), i.e. rc_dense_search_exact.
//
// Score (unchanged): s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f on the fp32 values.
//
// Screen.  Every fp32 operand a is split a = a_h + a_l + r with round-to-nearest-even conversions (v_cvt_pk_bf16_f32):
//   a_h = bf16(a),  a_l = bf16(a - a_h)   (the subtraction is exact in fp32: a - a_h is the low 16 bits of a's significand),
// and s~ = sum_d (q_h x_h + q_h x_l + q_l x_h): three bf16 MFMAs per K step into one fp32 accumulator.  A product of two bf16
// values has 16 significant bits: exact in fp32 unless it underflows.  The corpus is split while it is staged global -> LDS
// (no second copy in HBM); the queries are split once per call into two bf16 planes in the workspace, zero-padded to a
// multiple of 32 columns (dense_bf16x3_split_kernel: the bytes of q again).
//
// The bound |s~ - s| <= E_q.  Write P = sum_d |q_d x_d| <= ||q||_2 ||x||_2 <= ||q||_2 X.
//   split:     |a - a_h| <= 2^-9 |a|, |a_l| <= 2^-9 (1 + 2^-8) |a|, |r| <= 2^-9 |a - a_h| <= 2^-18 |a| while a_l is a normal
//              bf16 (the issue's looser 2^-8 / 2^-16 are kept for the constant).  The part of q_d x_d the screen drops is
//              q_l x_l + r_q x + (q_h + q_l) r_x, at most 3.02 * 2^-16 |q_d x_d|: in total <= 3.02 * 2^-16 P.
//   screen:    an fp32 sum, in an order of the hardware's own, of 3 D exact products whose absolute values sum to <= 1.008 P:
//              at most 3 D additions, each off by <= 2^-23 (truncation) of a partial sum <= 1.008 P: <= 6.05 D 2^-24 P.
//   chain:     D roundings to nearest of partial sums <= P (1 + D 2^-24): <= 1.01 D 2^-24 P.
//   together   (7.1 D 2^-24 + 3.02 * 2^-16) P, second-order terms (1 + 2^-23)^(3 D) included while D <= 65536:
//              E_rel = (8 D_pad 2^-24 + 4 * 2^-16) ||q||_2 X,   D_pad = D rounded up to 16.
//              Above D = 65536 the certificate is never given (every query takes the exact route).
//   underflow: the relative argument fails below the normal ranges, so E_q carries an absolute part:
//              - a_l that is a bf16 subnormal (|a - a_h| < 2^-126, i.e. |a| below about 2^-118) is rounded to a multiple of
//                2^-133: |r| <= 2^-134 instead of 2^-18 |a|.  The products then drop at most
//                2^-134 (1 + 2^-7) (|q_d| + |x_d|) per d, in total <= 2^-133 sqrt(D) (||q||_2 + X);
//              - a product below 2^-126 is rounded to a multiple of 2^-149, as is a subnormal fmaf result of the chain: 3 D + D
//                errors of at most 2^-149 (fp32 additions are exact in the subnormal range);
//              E_abs = 2^-133 sqrt(D_pad) (||q||_2 + X) + 4 D_pad 2^-149.
//              This assumes that neither the conversion, the subtraction nor the matrix instruction flushes subnormal
//              operands or results to zero; see DENSE_B3_C_SUB below.
//   E_q = E_rel + E_abs.  The four constants are exported (rc_dense_bf16x3_error_constants) and are what
//   ops.dense_bf16x3_error_bound evaluates.
#include "dense_screen.h"

typedef __bf16 dense_bf16x8 __attribute__((ext_vector_type(8)));
#define DENSE_B3_KC 32                                   // K per LDS stage: one v_mfma_f32_16x16x32_bf16 step
// one operand's tile row (dense_screen.h): 128 bytes = [32 bf16 high plane | 32 bf16 low plane]; chunks 0 - 3 hold
// k = 8c .. 8c + 7 of the high plane, 4 - 7 the same k of the low plane
#define DENSE_B3_C_SUM 8.0                               // E_rel = (C_SUM D_pad 2^-24 + C_SPLIT 2^-16) ||q|| X
#define DENSE_B3_C_SPLIT 4.0
// E_abs = C_SUB sqrt(D_pad) (||q|| + X) + C_UNDER D_pad, for hardware that does not flush.  Measured on the MI355X (the subnormal
// families of the screen-error test, tests/test_dense_bf16x3.py): neither v_cvt_pk_bf16_f32 nor
// v_mfma_f32_16x16x32_bf16 flushes — fp32-subnormal rows score ~7e-38 with an error of 3.5e-40, at most 0.21 E_q, where a flushed
// operand would lose the whole score; values whose low parts are bf16 subnormals stay below 0.06 E_q.
#define DENSE_B3_C_SUB 0x1p-133
#define DENSE_B3_C_UNDER 0x1p-147
#define DENSE_B3_MAX_D 65536                             // the certificate's second-order terms are bounded up to here

__device__ __forceinline__ void dense_b3_split8(const float* a, dense_bf16x8& h, dense_bf16x8& l) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 hi = (__bf16)a[e];                  // round to nearest even
        h[e] = hi;
        l[e] = (__bf16)(a[e] - (float)hi);               // exact difference, rounded once
    }
}

// grid: ceil(nq * (D32 / 8) / 256) blocks of 256 threads; thread -> 8 consecutive columns of one query.  qs: [2][nq][D32] bf16,
// plane 0 = q_h, plane 1 = q_l, columns D .. D32 - 1 zero.
__global__ __launch_bounds__(256) void dense_bf16x3_split_kernel(const float* __restrict__ q, int nq, int D, int D32,
                                                                 __bf16* __restrict__ qs) {
    const int cpr = D32 / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)nq * cpr) return;
    const int row = (int)(i / cpr), k0 = (int)(i % cpr) * 8;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (k0 + e < D) ? q[(int64_t)row * D + k0 + e] : 0.f;
    dense_bf16x8 h, l;
    dense_b3_split8(a, h, l);
    *reinterpret_cast<dense_bf16x8*>(qs + (int64_t)row * D32 + k0) = h;
    *reinterpret_cast<dense_bf16x8*>(qs + ((int64_t)nq + row) * D32 + k0) = l;
}

// grid: ceil(nrows / 128) blocks of 256 threads, two per CU (64 KB of LDS each).  Arguments as dense_gemm_kernel, except that
// the queries arrive split: qs [2][nq][D32] (dense_bf16x3_split_kernel).  !PAD: D % 8 == 0 and 16-byte aligned corpus rows; PAD
// reads the corpus element by element.  The block owns 128 corpus rows and walks every tile of 128 queries; wave (wr, wc) owns
// 64 queries x 64 rows as 4 x 4 tiles of v_mfma_f32_16x16x32_bf16 (tiling, operand map and epilogue as laid out in
// dense_screen.h), three per tile and K step, one 16-byte LDS read per operand tile, plane and K step.
template <int MODE, bool PAD>
__global__ __launch_bounds__(256, 2) void dense_bf16x3_gemm_kernel(const float* __restrict__ x, int64_t ldx, int64_t N,
                                                                int64_t nrows, int64_t smap, const __bf16* __restrict__ qs,
                                                                int nq, int D, int D32, const float* __restrict__ thr,
                                                                float* __restrict__ out, unsigned* __restrict__ cnt,
                                                                unsigned long long* __restrict__ cand) {
    constexpr int TM = 16, NT = 4;
    __shared__ __attribute__((aligned(16))) unsigned char dense_b3_smem[DENSE_SCREEN_LDS_BYTES];
    unsigned char* sa = dense_b3_smem;                                      // [2][128 rows][128 bytes] queries
    unsigned char* sb = dense_b3_smem + 2 * DENSE_SCREEN_OPERAND_BYTES;         // [2][128 rows][128 bytes] corpus
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l % TM, grp = l / TM;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> k = 8 lc .. 8 lc + 7 of rows tid / 4 + 64 i, i < 2 (4 threads read 128 contiguous bytes of fp32)
    const int lrow = tid >> 2, lc = tid & 3;
    const float* xp[2];
    int so[2];                                                             // swizzled LDS offsets of the high-plane chunks
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t jl = (j0 + lrow + 64 * i < nrows) ? j0 + lrow + 64 * i : nrows - 1;
        const int64_t xrow = smap ? (int64_t)((uint64_t)jl * (uint64_t)N / (uint64_t)smap) : jl;
        xp[i] = x + xrow * ldx;
        so[i] = dense_screen_lds_off(lrow + 64 * i, lc);
    }
    // the low-plane chunk 4 + lc of the same row: (4 + lc) ^ m = (lc ^ m) ^ 4 for any 3-bit m
    const int nkc = (D + DENSE_B3_KC - 1) / DENSE_B3_KC;                    // == D32 / 32
    const __bf16* ql = qs + (int64_t)nq * D32;
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        int64_t qo_[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) qo_[i] = (int64_t)((qt + lrow + 64 * i < nq) ? qt + lrow + 64 * i : nq - 1) * D32 + lc * 8;
        dense_f32x4 acc[NT][NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
        dense_bf16x8 rah[2], ral[2];
        float rb[2][8];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_B3_KC + lc * 8;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                rah[i] = *reinterpret_cast<const dense_bf16x8*>(qs + qo_[i] + kc * DENSE_B3_KC);      // padded planes: in bounds
                ral[i] = *reinterpret_cast<const dense_bf16x8*>(ql + qo_[i] + kc * DENSE_B3_KC);
                if constexpr (PAD) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) rb[i][e] = (k0 + e < D) ? xp[i][k0 + e] : 0.f;
                } else if (k0 < D) {                                        // D % 8 == 0: a chunk is inside or outside
                    dense_load8(xp[i] + k0, rb[i]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) rb[i][e] = 0.f;
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                dense_bf16x8 h, lo;
                dense_b3_split8(rb[i], h, lo);
                *reinterpret_cast<dense_bf16x8*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = rah[i];
                *reinterpret_cast<dense_bf16x8*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + (so[i] ^ 64)) = ral[i];
                *reinterpret_cast<dense_bf16x8*>(sb + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = h;
                *reinterpret_cast<dense_bf16x8*>(sb + buf * DENSE_SCREEN_OPERAND_BYTES + (so[i] ^ 64)) = lo;
            }
        };
        // query tiles that hold only padding skip their MFMAs, wave-uniformly
        bool act[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) act[a] = qt + wr * 64 + a * TM < nq;
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
            const unsigned char* pa = sa + buf * DENSE_SCREEN_OPERAND_BYTES;
            const unsigned char* pb = sb + buf * DENSE_SCREEN_OPERAND_BYTES;
            dense_bf16x8 fah[NT], fal[NT], fbh[NT], fbl[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int oa = dense_screen_lds_off(wr * 64 + t * TM + col, grp), ob = dense_screen_lds_off(wc * 64 + t * TM + col, grp);
                fah[t] = *reinterpret_cast<const dense_bf16x8*>(pa + oa);
                fal[t] = *reinterpret_cast<const dense_bf16x8*>(pa + (oa ^ 64));
                fbh[t] = *reinterpret_cast<const dense_bf16x8*>(pb + ob);
                fbl[t] = *reinterpret_cast<const dense_bf16x8*>(pb + (ob ^ 64));
            }
            // the two small terms first, then q_h x_h: 16 independent accumulators between two MFMAs on the same one
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a])
#pragma unroll
                    for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fal[a], fbh[b], acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a])
#pragma unroll
                    for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fah[a], fbl[b], acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (act[a])
#pragma unroll
                    for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fah[a], fbh[b], acc[a][b], 0, 0, 0);
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        const float* s_thr = dense_screen_stage_thr<MODE>(sa, nkc, thr, qt, nq, tid);
        dense_screen_epilogue<MODE>(acc, j0, wr, wc, col, grp, qt, nq, s_thr, nrows, out, cnt, cand, l);
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

static inline int dense_b3_d32(int D) { return (D + 31) / 32 * 32; }
static inline size_t dense_b3_split_bytes(int nq, int D) { return rc_align_up((size_t)2 * (size_t)nq * (size_t)dense_b3_d32(D) * 2, 256); }

static int dense_b3_launch_split(rc_handle_t h, const float* q, int nq, int D, __bf16* qs, hipStream_t s) {
    const int D32 = dense_b3_d32(D);
    const int64_t n = (int64_t)nq * (D32 / 8);
    hipLaunchKernelGGL(dense_bf16x3_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, nq, D, D32, qs);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

template <int MODE>
static int dense_b3_launch_gemm(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int64_t nrows, int64_t smap,
                                const __bf16* qs, int nq, int D, const float* thr, float* out, unsigned* cnt,
                                unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    const int D32 = dense_b3_d32(D);
    if (D % 8 == 0 && ldx % 4 == 0 && !((uintptr_t)x & 15u))
        hipLaunchKernelGGL((dense_bf16x3_gemm_kernel<MODE, false>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, qs, nq, D, D32,
                           thr, out, cnt, cand);
    else
        hipLaunchKernelGGL((dense_bf16x3_gemm_kernel<MODE, true>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, qs, nq, D, D32,
                           thr, out, cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// The certificate refuses a query value whose bf16 rounding is infinite (|v| >= 2^128 - 2^119; inf and NaN with it) and D > 65536.
struct dense_b3_variant : dense_variant_defaults {
    typedef float T;
    typedef __bf16 Q;
    static constexpr bool approximate = true;
    static constexpr unsigned ws_align = 16;             // the planes are read with 16-byte loads
    static size_t extra_ws_bytes(int nq, int D) { return dense_b3_split_bytes(nq, D); }
    static int prepass(rc_handle_t h, const float* q, int nq, int D, char* tail, const Q** qs, hipStream_t s) {
        *qs = (const __bf16*)tail;                       // 16-byte aligned: the workspace is, and the fast layout is a multiple of 256
        return dense_b3_launch_split(h, q, nq, D, (__bf16*)tail, s);
    }
    template <int MODE, typename... A>
    static int launch_gemm(const float*, A... a) { return dense_b3_launch_gemm<MODE>(a...); }
    static constexpr auto* exact_rows = &dense_exact_rows_f32;
    __device__ static bool refuse(float v, int D) {
        return (__float_as_uint(v) & 0x7FFFFFFFu) >= 0x7F7F8000u || D > DENSE_B3_MAX_D;
    }
    __device__ static double eq(int D, double ss, double xnorm) {
        const double up = 1.0 + 0x1p-30;
        const double dpad = (double)((D + 15) / 16 * 16);
        const double qn = sqrt(ss) * up, X = xnorm * up;
        return ((DENSE_B3_C_SUM * dpad * 0x1p-24 + DENSE_B3_C_SPLIT * 0x1p-16) * qn * X * up +
                DENSE_B3_C_SUB * sqrt(dpad) * up * (qn + X) + DENSE_B3_C_UNDER * dpad) * up;
    }
};

extern "C" void rc_dense_bf16x3_error_constants(double* c) {
    c[0] = DENSE_B3_C_SUM;
    c[1] = DENSE_B3_C_SPLIT;
    c[2] = DENSE_B3_C_SUB;
    c[3] = DENSE_B3_C_UNDER;
}

extern "C" size_t rc_dense_bf16x3_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_b3_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_bf16x3_scores_ws_bytes(int D, int nq) {
    return D > 0 && nq > 0 ? dense_b3_split_bytes(nq, D) : 0;
}

extern "C" int rc_dense_bf16x3_scores(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                      float* out, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll) return RC_ESHAPE;
    if (!h || !x || !q || !out || N <= 0 || D <= 0 || nq < 0 || ldx < D) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    if (!ws || ((uintptr_t)ws & 15u) || ws_bytes < dense_b3_split_bytes(nq, D)) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int rc = dense_b3_launch_split(h, q, nq, D, (__bf16*)ws, s);
    if (rc != RC_OK) return rc;
    return dense_b3_launch_gemm<DENSE_STORE>(h, x, ldx, N, N, 0, (const __bf16*)ws, nq, D, nullptr, out, nullptr, nullptr, s);
}

extern "C" int rc_dense_bf16x3_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                        const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores,
                                        int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_b3_variant>(h, x, ldx, N, D, q, nq, nullptr, xnorm_max, k, id_offset, sel_slack, scores, ids,
                                                status, qstatus, ws, ws_bytes, stream);
}
