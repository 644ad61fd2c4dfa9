// Exact dense L2 top-k search over an fp32 corpus with the bf16x3 matrix-core screen: the results of dense_search_l2.hip (ids
// AND distance bits of rc_dense_l2_search_q), the corpus stays fp32, only the screen leaves the fp32 matrix cores.
//
// Distance (unchanged): d(q, n) = the fp32 chain  acc = +0.0f;  for j = 0 .. D-1 ascending:  t = q[j] - x[n][j],
// acc = fmaf(t, t, acc).  Every stage works on s = -d; the entry negates the k output values at the end
// (dense_l2_launch_negate): d ascending, +0.0f for a zero, +inf / -1 past N.
//
// Route: dense_search_route (dense_screen.h) with this unit's variant, the bf16x3 variant and the L2 variant combined.
//   N <= DENSE_EXACT_MAX_N, and the queries the fast route gives up on: the rows of rc_dense_l2_search_exact
//   (dense_l2_exact_rows_f32, dense_search_l2.hip), then the radix select, then the sign.  There is no exact entry of its own.
//   Above: dense_bf16x3_split_kernel splits the queries into two bf16 planes in the tail of the workspace;
//   dense_bf16x3_gemm_kernel<.., L2 = true> (dense_bf16x3_gemm.h) screens the strided sample and then all rows with
//   sigma~(q, n) = fmaf(2, s~(q, n), -xsq[n]); s~ is the three-MFMA bf16x3 sum of that header, xsq[n] the caller's fp32 squared
//   norm of row n (an fp64 sum rounded to nearest, ops.dense_row_sqnorms).  The candidates are rescored by
//   dense_rescore_kernel<VEC, float, L2 = true>, selected, certified and negated.
//
// The bound |sigma~ - ||q||^2 + d| <= E_q.  u = 2^-24, X >= the largest row norm, P = sum_j |q_j x_j| <= ||q|| X,
// R = (||q|| + X)^2, so P <= R / 4 (arithmetic and geometric mean), X^2 <= R and 2 P + X^2 <= R; D <= 65536 (above it no
// certificate is given).  In exact arithmetic ||q||^2 - D2 = 2 q.x - ||x||^2 with D2 = sum_j (q_j - x_j)^2 <= R.
//   chain:   as in dense_search_l2.hip: t_j = (q_j - x_j)(1 + e_j), |e_j| <= u, and t_j^2 passes at most D fmaf roundings; the
//            chain differs from D2 by at most gamma_{D+2} D2:                                                 <= 1.01 (D + 2) u R
//   split:   as in dense_search_bf16x3.hip: the part of q_j x_j the three products drop is q_l x_l + r_q x + (q_h + q_l) r_x,
//            at most 3.02 * 2^-16 |q_j x_j| while the low parts are normal bf16:          |sum of the 3 D products - q.x| <= 3.02 * 2^-16 P
//   sum:     s~ is SOME fp32 accumulation of the 3 D exact products, whose absolute values sum to <= 1.008 P: any tree, every
//            addition rounded to nearest or truncated, relative error <= 2 u.  A product passes at most 3 D additions:
//            ((1 + 2 u)^(3 D) - 1) 1.008 P <= 1.012 * 6 D u * 1.008 P (6 D u <= 2^-5.4 while D <= 65536):           <= 6.12 D u P
//   twice:   s~ enters sigma~ with the factor 2: (12.24 D u + 6.04 * 2^-16) P, and P <= R / 4:   <= (3.06 D u + 1.51 * 2^-16) R
//   xsq:     one rounding of an fp64 sum, |xsq - ||x||^2| <= (u + D 2^-53) ||x||^2 <= 1.01 u X^2:                     <= 1.01 u R
//   fmaf:    the one rounding of sigma~ (a vector-ALU fma, to nearest) is at most u |2 s~ - xsq|; |s~| <= (1 + 6.12 D u +
//            3.02 * 2^-16) P <= 1.024 P, so at most u (2.048 P + 1.01 X^2) <= 1.024 u (2 P + X^2):                   <= 1.03 u R
//   total:   (4.07 D + 4.06) u R + 1.51 * 2^-16 R <= (5 D_pad u + 2 * 2^-16) R for every D >= 1, D_pad = D rounded up to 16
//            (D <= 16: 4.07 * 16 + 4.06 < 80; D > 16: 0.93 D > 14.8 > 4.06).          E_rel = (5 D_pad u + 2 * 2^-16) R
//   small:   the relative argument fails below the normal ranges, so E_q carries an absolute part.
//            - operands: a value a with |a| < 2^-126, or a high or low part below 2^-126 (a bf16 subnormal), may be rounded to a
//              multiple of 2^-133 (no flush: it then drops at most 2^-134 * 1.01 of the other operand per product) or read as
//              zero by the conversion or the matrix core (flush: it drops products of at most 2^-126 * 1.01 of the other
//              operand).  Whether the hardware flushes is not assumed either way, as in dense_search_l2.hip: the larger charge is
//              paid.  Per j at most 1.01 * 2^-126 (|q_j| + |x_j|), over the row 1.01 * 2^-126 sqrt(D) (||q|| + X), twice in
//              sigma~:                                                              E_flush = 4 * 2^-126 sqrt(D_pad) (||q|| + X)
//            - results: a product or a sum below 2^-126 is rounded to a multiple of 2^-149 instead of relatively: 3 D products
//              of the screen, each off by <= 2^-149 and entering twice, D fmaf results of the chain (its subtraction is exact
//              there) and the fma of sigma~, each off by <= 2^-150 (fp32 additions are exact in the subnormal range):
//              (6 D + D / 2 + 1 / 2) 2^-149:                                                        E_under = 8 D_pad 2^-149
//   range:   R < 2^126 keeps every intermediate finite (|s~| <= 1.024 P < 2^125, xsq <= 1.01 X^2, d <= 1.01 R); a query value
//            whose bf16 rounding is infinite (|v| >= 2^128 - 2^119) is refused on its own, and a corpus value of that size
//            makes X^2 >= 2^255.  Otherwise a sigma~ may be inf or NaN and fail the FILTER's comparison: no certificate, the
//            exact route answers.
//   E_q = E_rel + E_flush + E_under; the four constants are exported (rc_dense_l2_bf16x3_error_constants) and are what
//   ops.dense_l2_bf16x3_error_bound evaluates.
//
// Certificate: as in dense_search_l2.hip, t >= thr~ - ss_down + E_q with t = the k-th best -d of the list; V::eq is E_q
// (pushed upwards) minus the query's squared norm (pushed downwards), in fp64.  Refused: a non-finite query value, one whose
// bf16 rounding is not finite, D > 65536, R >= 2^126.
#include "dense_bf16x3_gemm.h"
#include "dense_l2.h"

#define DENSE_L2_B3_C_SUM 5.0                            // E_rel   = (C_SUM D_pad 2^-24 + C_SPLIT 2^-16) (||q|| + X)^2
#define DENSE_L2_B3_C_SPLIT 2.0
#define DENSE_L2_B3_C_FLUSH 0x1p-124                     // E_flush = C_FLUSH sqrt(D_pad) (||q|| + X)        (4 * 2^-126)
#define DENSE_L2_B3_C_UNDER 0x1p-146                     // E_under = C_UNDER D_pad                          (8 * 2^-149)
#define DENSE_L2_B3_MAX_R 0x1p126                        // (||q|| + X)^2 below this: nothing overflows

struct dense_l2_b3_variant : dense_b3_variant_base<dense_l2_b3_variant, true> {
    static constexpr auto* exact_rows = &dense_l2_exact_rows_f32;
    static constexpr auto* finish = &dense_l2_launch_negate;
    // E_q - ss_down: what is added to thr~ (header).  +inf (never certified) unless (||q|| + X)^2 < 2^126.
    __device__ static double eq(int D, double ss, double xnorm) {
        const double up = 1.0 + 0x1p-30;
        const double dpad = (double)((D + 15) / 16 * 16);
        const double r = (sqrt(ss) + xnorm) * up, R = r * r * up;
        if (!(R < DENSE_L2_B3_MAX_R)) return INFINITY;
        const double e = ((DENSE_L2_B3_C_SUM * dpad * 0x1p-24 + DENSE_L2_B3_C_SPLIT * 0x1p-16) * R * up +
                          DENSE_L2_B3_C_FLUSH * sqrt(dpad) * up * r + DENSE_L2_B3_C_UNDER * dpad) * up;
        return e - ss * (1.0 - 0x1p-30);
    }
};

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" void rc_dense_l2_bf16x3_error_constants(double* c) {
    c[0] = DENSE_L2_B3_C_SUM;
    c[1] = DENSE_L2_B3_C_SPLIT;
    c[2] = DENSE_L2_B3_C_FLUSH;
    c[3] = DENSE_L2_B3_C_UNDER;
}

extern "C" size_t rc_dense_l2_bf16x3_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_l2_b3_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_l2_bf16x3_scores_ws_bytes(int D, int nq) {
    return D > 0 && nq > 0 ? dense_b3_split_bytes(nq, D) : 0;
}

extern "C" int rc_dense_l2_bf16x3_scores(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                         const float* xsq, float* out, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_scores_entry<dense_l2_b3_variant>(h, x, ldx, N, D, q, nq, {xsq}, out, ws, ws_bytes, stream);
}

extern "C" int rc_dense_l2_bf16x3_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                           const float* xsq, const float* xnorm_max, int k, int64_t id_offset, double sel_slack,
                                           float* dist, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                                           rc_stream_t stream) {
    return dense_search_entry<dense_l2_b3_variant>(h, x, ldx, N, D, q, nq, {xsq}, xnorm_max, false, 0, k, id_offset, sel_slack, dist,
                                                   ids, status, qstatus, ws, ws_bytes, stream);
}
