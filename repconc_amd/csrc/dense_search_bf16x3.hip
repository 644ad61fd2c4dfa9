// Exact dense inner-product top-k search over an fp32 corpus with a bf16x3 matrix-core screen: the results of
// dense_search.hip (ids AND score bits of rc_dense_search_q), the corpus stays fp32, only the screen leaves the fp32 matrix
// cores.  The route is dense_search_route (dense_screen.h) with this unit's variant: dense_bf16x3_split_kernel is its query
// pre-pass, dense_bf16x3_gemm_kernel screens, the candidates are rescored by the chain and every answer carries a certificate
// with the E_q derived below.  Exact route: the rows of dense_exact_rows_f32 (dense_search.hip), i.e. rc_dense_search_exact.
//
// Score (unchanged): s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f on the fp32 values.
//
// Screen.  s~ = sum_d (q_h x_h + q_h x_l + q_l x_h) over the round-to-nearest-even bf16 splits a = a_h + a_l + r of both operands:
// the GEMM, the query split pre-pass and the constants below are in dense_bf16x3_gemm.h, shared with the L2 search.
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
//              operands or results to zero; see DENSE_B3_C_SUB (dense_bf16x3_gemm.h).
//   E_q = E_rel + E_abs.  The four constants are exported (rc_dense_bf16x3_error_constants) and are what
//   ops.dense_bf16x3_error_bound evaluates.
#include "dense_bf16x3_gemm.h"

// The certificate refuses a query value whose bf16 rounding is infinite (|v| >= 2^128 - 2^119; inf and NaN with it) and D > 65536
// (dense_b3_variant_base::refuse).
struct dense_b3_variant : dense_b3_variant_base<dense_b3_variant, false> {
    static constexpr auto* exact_rows = &dense_exact_rows_f32;
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
    return dense_scores_entry<dense_b3_variant>(h, x, ldx, N, D, q, nq, {}, out, ws, ws_bytes, stream);
}

extern "C" int rc_dense_bf16x3_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                        const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores,
                                        int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_b3_variant>(h, x, ldx, N, D, q, nq, {}, xnorm_max, false, 0, k, id_offset, sel_slack, scores,
                                                ids, status, qstatus, ws, ws_bytes, stream);
}
