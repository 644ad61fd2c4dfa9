// Exact dense inner-product top-k search over a corpus of 8-bit scalar-quantiser codes (Faiss IndexScalarQuantizer, QT_8bit):
// one byte per dimension, a quarter of dense_search.hip's bytes, and the screen runs on the int8 matrix cores.
//
// Store and score.  x holds c'_d = c_d - 128 as int8, c_d in 0 .. 255 the code of dimension d; dec = [step | mid], two fp32
// vectors of D values.  A row decodes to x^_d = fmaf((float)c'_d, step_d, mid_d) and
//   s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f of q_d * x^_d
// — the definition of dense_search.hip applied to the decoded corpus (rc_dense_sq8_decode writes it out).
//
// The route is dense_search_route (dense_screen.h) with this unit's coded variant: dense_i8_prepass_kernel quantises the
// queries, dense_i8_gemm_kernel (dense_i8_gemm.h) screens, the candidates are rescored by the chain over rows decoded on the
// fly (dense_sq8_rescore_kernel) and every answer carries a certificate (dense_sq8_certify_kernel).  Exact route: the chain of
// every pair (dense_sq8_rows_kernel).
//
// The bound |s~ - s| <= E_q.  u = 2^-24; every value below is finite and, until the last paragraph, normal.  Per query:
//   w_d = fl(q_d step_d), W1 = sum_d |w_d|, B1 = sum_d |q_d mid_d|, alpha = alpha_q, v_d = 256 h_d + l_d (dense_i8_gemm.h);
// per corpus: C1 >= the largest sum_d |c'_d| of a row, X >= the largest Euclidean norm of a decoded row.
//   chain     s is D roundings away from R = sum_d q_d x^_d: |s - R| <= D u / (1 - D u) * sum_d |q_d x^_d| <= 1.004 D u P,
//             P = ||q||_2 X (Cauchy-Schwarz), while D <= 65536.
//   decode    x^_d = (c'_d step_d + mid_d)(1 + e), |e| <= u: |R - sum_d q_d c'_d step_d - sum_d q_d mid_d| <= 1.001 u P.
//   w         |q_d step_d - w_d| <= u |w_d| (1 + 2u) and |c'_d| <= 128: |sum_d (q_d step_d - w_d) c'_d| <= 1.001 * 128 u W1.
//   quantise  |w_d - alpha v_d| <= alpha (1/2 + 2^-37): the fp64 quotient is within 2^-53 of the ratio, itself below 2^15.
//             |sum_d (w_d - alpha v_d) c'_d| <= alpha (1/2 + 2^-37) C1.                    <- the only term that is not a rounding
//   combine   T = 256 A_h + A_l = sum_d v_d c'_d exactly.  The epilogue rounds A_h, A_l to fp32 and their fmaf:
//             |t - T| <= u (256 |A_h| + |A_l| + |T| (1 + 3u)) <= 2.001 u sum_d (|256 h_d| + |l_d|) |c'_d|, and
//             |256 h_d| + |l_d| <= |v_d| + 256, alpha |v_d| <= |w_d| + 0.501 alpha:
//             alpha |t - T| <= 2.001 u (128 W1 + 64.2 alpha D + 256 alpha C1).
//   bias      fp64 sum of D products, rounded once: |bias - sum_d q_d mid_d| <= 1.001 u B1.
//   epilogue  s~ = fl(alpha t + bias): <= u |s~| <= 1.001 u (alpha |T| + alpha |t - T| + 1.001 B1)
//             <= 1.002 u (128 W1 + 64.2 alpha D + B1).
//   together  E_rel = C_Q alpha C1 + u (C_W W1 + C_AD alpha D + C_AC alpha C1 + C_B B1 + C_CH (D_pad + 1) ||q||_2 X),
//             C_Q = 0.5, C_W = 520 >= (1.001 + 2.001 + 1.002) 128, C_AD = 194 >= 3.003 * 64.2, C_AC = 515 >= 2.001 * 256,
//             C_B = 2.1, C_CH = 1.02; D_pad = D rounded up to 16.
//   underflow the relative steps fail for subnormal results, whose absolute error is <= 2^-150 instead: a decoded value
//             (times |q_d|: in total <= 2^-150 sqrt(D) ||q||_2), a chain step (D of them), a w_d (times |c'_d|: <= 2^-150 C1)
//             and the epilogue's result:  E_abs = C_ABS 2^-149 (D_pad + sqrt(D_pad) ||q||_2 + C1 + 1), C_ABS = 1.
//   E_q = (E_rel + E_abs)(1 + 2^-20), evaluated in fp64; the factor covers the 2^-37 above and the evaluation's own roundings.
// The certificate refuses (qstatus bit2: the caller repeats, then takes the exact route) a query with a value, a w_d or a
// |q_d mid_d| that is not below 2^100, and one whose alpha is below 2^-100 although some w_d is not zero: up to there no
// intermediate overflows and alpha is normal.  An all-zero w has alpha = 0 and zero limbs: s~ = bias, inside the bound.
// The constants are exported (rc_dense_sq8_error_constants) and are what ops.dense_sq8_error_bound evaluates.
#include "dense_i8_gemm.h"
#include "dense_sq8_chain.h"

#define DENSE_SQ8_C_Q 0.5
#define DENSE_SQ8_C_W 520.0
#define DENSE_SQ8_C_AD 194.0
#define DENSE_SQ8_C_AC 515.0
#define DENSE_SQ8_C_B 2.1
#define DENSE_SQ8_C_CH 1.02
#define DENSE_SQ8_C_ABS 1.0

// The chain over coded rows — dense_sq8_rescore_kernel<VEC> for the fast route's candidates, dense_sq8_rows_kernel<> for the
// exact route — is dense_sq8_chain.h's, shared with the L2 search over the same store.

// grid: ceil(N D / 256) blocks of 256 threads: out [N][D] = the decoded corpus
__global__ __launch_bounds__(256) void dense_sq8_decode_kernel(const signed char* __restrict__ x, int64_t ldx, int64_t N, int D,
                                                               const float* __restrict__ dec, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * D) return;
    const int64_t r = i / D;
    const int d = (int)(i - r * D);
    out[i] = dense_sq8_decode(x[r * ldx + d], dec[d], dec[D + d]);
}

// ---- certificate ------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline double dense_sq8_eq(int D, double alpha, double w1, double b1, double qn, double c1, double X) {
    const double dpad = (double)((D + 15) / 16 * 16);
    const double rel = DENSE_SQ8_C_Q * alpha * c1 +
                       0x1p-24 * (DENSE_SQ8_C_W * w1 + DENSE_SQ8_C_AD * alpha * (double)D + DENSE_SQ8_C_AC * alpha * c1 +
                                  DENSE_SQ8_C_B * b1 + DENSE_SQ8_C_CH * (dpad + 1.0) * qn * X);
    const double abs_ = DENSE_SQ8_C_ABS * 0x1p-149 * (dpad + sqrt(dpad) * qn + c1 + 1.0);
    return (rel + abs_) * (1.0 + 0x1p-20);
}

// what dense_sq8_certify_kernel (dense_sq8_chain.h) adds to thr~: E_q from the sums it collected, each pushed upwards
struct dense_sq8_bound {
    __device__ static double add(int D, double alpha, double w1, double b1, double ss, double c1, double X) {
        const double up = 1.0 + 0x1p-30;
        return dense_sq8_eq(D, alpha, w1 * up, b1 * up, sqrt(ss) * up, c1, X);
    }
};

// ---- the variant ------------------------------------------------------------------------------------------------------------
struct dense_sq8_variant : dense_sq8_variant_base<dense_sq8_variant, false, dense_sq8_bound> {};

extern "C" void rc_dense_sq8_error_constants(double* c) {
    c[0] = DENSE_SQ8_C_Q;
    c[1] = DENSE_SQ8_C_W;
    c[2] = DENSE_SQ8_C_AD;
    c[3] = DENSE_SQ8_C_AC;
    c[4] = DENSE_SQ8_C_B;
    c[5] = DENSE_SQ8_C_CH;
    c[6] = DENSE_SQ8_C_ABS;
}
extern "C" int rc_dense_sq8_qmax(void) { return DENSE_I8_QMAX; }
extern "C" int rc_dense_sq8_max_d(void) { return DENSE_I8_MAX_D; }

extern "C" size_t rc_dense_sq8_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_exact_ws_bytes<dense_sq8_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_sq8_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_sq8_variant>(N, D, nq, k);
}

extern "C" int rc_dense_sq8_search_ws_counts(int64_t N, int D, int nq, int k, size_t* cnt_off) {
    return dense_search_ws_counts<dense_sq8_variant>(N, D, nq, k, cnt_off);
}

extern "C" size_t rc_dense_sq8_scores_ws_bytes(int D, int nq) {
    return D > 0 && D <= DENSE_I8_MAX_D && nq > 0 ? dense_i8_query_ws(nq, D).total : 0;
}

extern "C" int rc_dense_sq8_search_exact(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                         const float* dec, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                         size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_sq8_variant>(h, x, ldx, N, D, q, nq, {nullptr, dec}, false, 0, k, id_offset, scores, ids, ws,
                                                ws_bytes, stream);
}

extern "C" int rc_dense_sq8_scores(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                   const float* dec, float* out, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_scores_entry<dense_sq8_variant>(h, x, ldx, N, D, q, nq, {nullptr, dec}, out, ws, ws_bytes, stream);
}

extern "C" int rc_dense_sq8_decode(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* dec, float* out,
                                   rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll || D > DENSE_I8_MAX_D) return RC_ESHAPE;
    if (!h || !x || !dec || !out || N < 0 || D <= 0 || ldx < D) return RC_EINVAL;
    if (N == 0) return RC_OK;
    hipLaunchKernelGGL(dense_sq8_decode_kernel, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx,
                       N, D, dec, out);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

extern "C" int rc_dense_sq8_search_q(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                     const float* dec, const float* cstat, int k, int64_t id_offset, double sel_slack,
                                     float* scores, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                                     rc_stream_t stream) {
    return dense_search_entry<dense_sq8_variant>(h, x, ldx, N, D, q, nq, {nullptr, dec}, cstat, false, 0, k, id_offset, sel_slack,
                                                 scores, ids, status, qstatus, ws, ws_bytes, stream);
}
