// Exact dense L2 top-k search over a corpus of 8-bit scalar-quantiser codes (Faiss IndexScalarQuantizer, QT_8bit, METRIC_L2):
// the store of dense_search_sq8.hip under the distance of dense_search_l2.hip, screened on the int8 matrix cores.
//
// Store and distance.  x holds c'_d = c_d - 128 as int8, dec = [step | mid]; a row decodes to x^_d = fmaf((float)c'_d, step_d,
// mid_d) and d(q, n) = the fp32 chain  acc = +0.0f;  for j = 0 .. D-1 ascending:  t = q_j - x^_j,  acc = fmaf(t, t, acc)
// — dense_search_l2.hip's definition applied to the decoded corpus (rc_dense_sq8_decode writes it out): ids and distance bits
// equal rc_dense_l2_search_q on it.  Every stage works on s = -d; the entries negate the k output values at the end
// (dense_l2_launch_negate): d ascending, +0.0f for a zero, +inf / -1 past N.
//
// Route: dense_search_route (dense_screen.h) with this unit's variant, which is coded AND l2: its side operand is the pair
// (dec, xsq).  dense_i8_prepass_kernel quantises q * step as for the inner product, dense_i8_gemm_kernel<.., L2 = true>
// (dense_i8_gemm.h) screens with sigma(q, n) = fmaf(2, s~(q, n), -xsq[n]), s~ the int8 screen's value and xsq[n] the fp32
// squared norm of the decoded row n (an fp64 sum rounded to nearest: dense_sq8_sqnorm_kernel here, the rule of
// ops.dense_row_sqnorms), the candidates are rescored by dense_sq8_rescore_kernel<VEC, L2 = true> (dense_sq8_chain.h),
// selected, certified and negated.  Exact route: dense_sq8_rows_kernel<L2 = true>, the radix select, the sign.
//
// The bound |sigma - ||q||^2 + d| <= E_q.  u = 2^-24; W1, B1, alpha, C1, X as in dense_search_sq8.hip (W1 = sum_d |fl(q_d
// step_d)|, B1 = sum_d |q_d mid_d|, alpha = alpha_q; C1 >= the largest sum_d |c'_d| of a row, X >= the largest norm of a decoded
// row); P = ||q|| X, R = (||q|| + X)^2, S = sum_d q_d x^_d over the decoded fp32 values, D2 = sum_d (q_d - x^_d)^2 =
// ||q||^2 - 2 S + ||x^||^2.  Then
//   sigma - ||q||^2 + d = (sigma - (2 s~ - xsq)) + 2 (s~ - S) - (xsq - ||x^||^2) + (d - D2).
//   screen    |s~ - S| is the int8 proof without its chain term (that proof's s is D roundings away from the same S): decode
//             1.001 u P, w 1.001 * 128 u W1, quantise alpha (1/2 + 2^-37) C1, combine 2.001 u (128 W1 + 64.2 alpha D + 256
//             alpha C1), bias 1.001 u B1, epilogue 1.002 u (128 W1 + 64.2 alpha D + B1).  It enters sigma twice:
//               2 |s~ - S| <= alpha (1 + 2^-36) C1 + u (1025.1 W1 + 385.7 alpha D + 1024.6 alpha C1 + 4.01 B1 + 2.002 P).
//             The quantisation term, the only one that is not a rounding, is alpha C1.
//   xsq       one rounding of an fp64 sum of exact squares: |xsq - ||x^||^2| <= (u + D 2^-53) ||x^||^2 <= 1.01 u X^2 <= 1.01 u R
//   fmaf      the one rounding of sigma: <= u |2 s~ - xsq| (1 + u) <= 1.001 u (2 P + 1.01 X^2 + 2 |s~ - S|)
//             <= 1.02 u R + 1.001 u * 2 |s~ - S|, since 2 P + X^2 <= R
//   chain     as in dense_search_l2.hip over the decoded values: |d - D2| <= gamma_{D+2} D2 <= 1.01 (D + 2) u R
//   together  with P <= R / 4: (1.01 D + 2.02 + 1.01 + 1.02 + 0.5005) u R = (1.01 D + 4.5505) u R <= C_R (D_pad + 5) u R,
//             D_pad = D rounded up to 16, and the factor (1 + 1.001 u) on 2 |s~ - S| goes into the last line:
//             E_rel = C_Q alpha C1 + u (C_W W1 + C_AD alpha D + C_AC alpha C1 + C_B B1 + C_R (D_pad + 5) R),
//             C_Q = 1 (twice 0.5), C_W = 1040 and C_AD = 388 and C_AC = 1030 and C_B = 4.2 (twice the int8 unit's 520, 194, 515,
//             2.1, each above the sums listed under `screen`), C_R = 1.01.
//   underflow a result below 2^-126 is rounded absolutely, by <= 2^-150.  The int8 proof's terms without its chain's, twice:
//             2^-149 (sqrt(D) ||q|| + C1 + 2) (a decoded value times |q_d|, a w_d times |c'_d|, the bias and the epilogue); the
//             chain's D fmaf results (a subtraction that underflows is exact), xsq and sigma: (D + 2) 2^-150.
//             E_abs = C_ABS 2^-149 (D_pad + sqrt(D_pad) ||q|| + C1 + 3), C_ABS = 1.
//   E_q = (E_rel + E_abs)(1 + 2^-20), evaluated in fp64; the factor covers the 2^-36, the 1.001 u and the evaluation's roundings.
//   range     the int8 certificate's refusals stand (a value, a w_d or a |q_d mid_d| not below 2^100; alpha below 2^-100 with a
//             non-zero w): up to there s~ is finite.  The squares need more: R < 2^126 keeps xsq <= 1.01 X^2, d <= 1.01 R and
//             |S| <= P <= R / 4 finite, and E_q < 2^124 keeps |2 s~| <= 2 P + 2 |s~ - S| < 2^126, so sigma is finite and
//             compares as a number in the FILTER.  Otherwise E_q = +inf: no certificate, the exact route answers.  (A cstat
//             that is not such a pair — inf, NaN — makes E_q inf or NaN: not certified.)
// Certificate: as in dense_search_l2.hip, t >= thr~ - ss_down + E_q with t = the k-th best -d of the list: what is added to thr~
// is E_q (pushed upwards) minus the query's squared norm (pushed downwards), in fp64.  The constants are exported
// (rc_dense_l2_sq8_error_constants) and are what ops.dense_l2_sq8_error_bound evaluates.
#include "dense_l2.h"
#include "dense_sq8_chain.h"

#define DENSE_L2_SQ8_C_Q 1.0
#define DENSE_L2_SQ8_C_W 1040.0
#define DENSE_L2_SQ8_C_AD 388.0
#define DENSE_L2_SQ8_C_AC 1030.0
#define DENSE_L2_SQ8_C_B 4.2
#define DENSE_L2_SQ8_C_R 1.01
#define DENSE_L2_SQ8_C_ABS 1.0
#define DENSE_L2_SQ8_MAX_R 0x1p126                       // (||q|| + X)^2 below this, and
#define DENSE_L2_SQ8_MAX_E 0x1p124                       // E_q below this: nothing overflows

// ---- the rows' squared norms --------------------------------------------------------------------------------------------------
// grid: ceil(N / 4) blocks of 256 threads, one wave per row: out[n] = (float) sum_d (double)x^_d^2, x^_d = fmaf(c'_d, step_d,
// mid_d) decoded on the fly (the decoded corpus is never written).  A square of an fp32 value is exact in fp64; lane l sums
// d = l, l + 64, .. ascending, then the xor butterfly: a fixed order.
__global__ __launch_bounds__(256) void dense_sq8_sqnorm_kernel(const signed char* __restrict__ x, int64_t ldx, int64_t N, int D,
                                                               const float* __restrict__ dec, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                                                 // wave-uniform
    const signed char* xp = x + n * ldx;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)dense_sq8_decode(xp[d], dec[d], dec[D + d]);
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[n] = (float)acc;
}

// ---- certificate ------------------------------------------------------------------------------------------------------------
// E_q of the header from quantities already pushed upwards; +inf outside the range
__host__ __device__ static inline double dense_l2_sq8_eq(int D, double alpha, double w1, double b1, double qn, double c1, double X) {
    const double dpad = (double)((D + 15) / 16 * 16);
    const double r = qn + X, R = r * r;
    const double rel = DENSE_L2_SQ8_C_Q * alpha * c1 +
                       0x1p-24 * (DENSE_L2_SQ8_C_W * w1 + DENSE_L2_SQ8_C_AD * alpha * (double)D + DENSE_L2_SQ8_C_AC * alpha * c1 +
                                  DENSE_L2_SQ8_C_B * b1 + DENSE_L2_SQ8_C_R * (dpad + 5.0) * R);
    const double abs_ = DENSE_L2_SQ8_C_ABS * 0x1p-149 * (dpad + sqrt(dpad) * qn + c1 + 3.0);
    const double e = (rel + abs_) * (1.0 + 0x1p-20);
    return (R < DENSE_L2_SQ8_MAX_R && e < DENSE_L2_SQ8_MAX_E) ? e : (e != e ? e : INFINITY);
}

// what dense_sq8_certify_kernel adds to thr~: E_q (pushed upwards) minus the query's squared norm (pushed downwards)
struct dense_l2_sq8_bound {
    __device__ static double add(int D, double alpha, double w1, double b1, double ss, double c1, double X) {
        const double up = 1.0 + 0x1p-30;
        return dense_l2_sq8_eq(D, alpha, w1 * up, b1 * up, sqrt(ss) * up, c1, X) * up - ss * (1.0 - 0x1p-30);
    }
};

// ---- the variant ------------------------------------------------------------------------------------------------------------
struct dense_l2_sq8_variant : dense_sq8_variant_base<dense_l2_sq8_variant, true, dense_l2_sq8_bound> {
    static constexpr auto* finish = &dense_l2_launch_negate;
};

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" void rc_dense_l2_sq8_error_constants(double* c) {
    c[0] = DENSE_L2_SQ8_C_Q;
    c[1] = DENSE_L2_SQ8_C_W;
    c[2] = DENSE_L2_SQ8_C_AD;
    c[3] = DENSE_L2_SQ8_C_AC;
    c[4] = DENSE_L2_SQ8_C_B;
    c[5] = DENSE_L2_SQ8_C_R;
    c[6] = DENSE_L2_SQ8_C_ABS;
    c[7] = DENSE_L2_SQ8_MAX_R;
    c[8] = DENSE_L2_SQ8_MAX_E;
}

extern "C" size_t rc_dense_l2_sq8_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_exact_ws_bytes<dense_l2_sq8_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_l2_sq8_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_l2_sq8_variant>(N, D, nq, k);
}

extern "C" int rc_dense_l2_sq8_search_ws_counts(int64_t N, int D, int nq, int k, size_t* cnt_off) {
    return dense_search_ws_counts<dense_l2_sq8_variant>(N, D, nq, k, cnt_off);
}

extern "C" size_t rc_dense_l2_sq8_scores_ws_bytes(int D, int nq) {
    return D > 0 && D <= DENSE_I8_MAX_D && nq > 0 ? dense_i8_query_ws(nq, D).total : 0;
}

// the exact route reads no norm: o.xsq stays null
extern "C" int rc_dense_l2_sq8_search_exact(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q,
                                            int nq, const float* dec, int k, int64_t id_offset, float* dist, int64_t* ids,
                                            void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_l2_sq8_variant>(h, x, ldx, N, D, q, nq, {nullptr, dec}, false, 0, k, id_offset, dist, ids, ws,
                                                   ws_bytes, stream);
}

extern "C" int rc_dense_l2_sq8_scores(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                      const float* dec, const float* xsq, float* out, void* ws, size_t ws_bytes,
                                      rc_stream_t stream) {
    return dense_scores_entry<dense_l2_sq8_variant>(h, x, ldx, N, D, q, nq, {xsq, dec}, out, ws, ws_bytes, stream);
}

extern "C" int rc_dense_sq8_row_sqnorms(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* dec,
                                        float* out, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll || D > DENSE_I8_MAX_D) return RC_ESHAPE;
    if (!h || !x || !dec || !out || N < 0 || D <= 0 || ldx < D) return RC_EINVAL;
    if (N == 0) return RC_OK;
    hipLaunchKernelGGL(dense_sq8_sqnorm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, N, D,
                       dec, out);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

extern "C" int rc_dense_l2_sq8_search_q(rc_handle_t h, const int8_t* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                        const float* dec, const float* xsq, const float* cstat, int k, int64_t id_offset,
                                        double sel_slack, float* dist, int64_t* ids, int* status, int* qstatus, void* ws,
                                        size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_l2_sq8_variant>(h, x, ldx, N, D, q, nq, {xsq, dec}, cstat, false, 0, k, id_offset, sel_slack,
                                                    dist, ids, status, qstatus, ws, ws_bytes, stream);
}
