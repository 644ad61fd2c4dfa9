// Exact dense L2 top-k search over an fp16 corpus (Faiss IndexFlatL2 with useFloat16 = True): half the bytes of
// dense_search_l2.hip's corpus, and the screen runs on the f16 matrix cores.
//
// Distance: x and q are IEEE fp16, finite; d(q, n) = the fp32 chain of dense_search_l2.hip over the widened values,
// acc = +0.0f;  for j = 0 .. D-1 ascending:  t = (float)q[j] - (float)x[n][j],  acc = fmaf(t, t, acc) — that unit's definition
// applied to x.float(), q.float(): ids and distance bits equal rc_dense_l2_search_q on the widened arrays.  Every stage works
// on s = -d; the entries negate the k output values at the end (dense_l2_launch_negate): d ascending, +0.0f for a zero,
// +inf / -1 past N.
//
// Route: dense_search_route (dense_screen.h) with this unit's variant.
//   N <= DENSE_EXACT_MAX_N, and the queries the fast route gives up on: dense_l2_exact_kernel<PAD, _Float16> (dense_l2.h,
//   instantiated here alone) writes the full rows of -d, then the radix select, then the sign.
//   Above: dense_f16_gemm_kernel<.., L2 = true> (dense_f16_gemm.h) screens the strided sample and then all rows with
//   sigma(q, n) = fmaf(2, dot(q, x_n), -xsq[n]); dot is the f16 matrix cores' fp32 accumulator, xsq[n] the caller's fp32
//   squared norm of the stored (rounded) row n, an fp64 sum rounded to nearest (ops.dense_row_sqnorms).  The candidates are
//   rescored by dense_rescore_kernel<VEC, _Float16, L2 = true>, selected, certified and negated.
//
// The bound |sigma - ||q||^2 + d| <= E_q.  u = 2^-24, X >= the largest row norm, P = ||q|| X, R = (||q|| + X)^2, D <= 65536
// (above it no certificate is given).
//   chain:   as in dense_search_l2.hip: t_j = (q_j - x_j)(1 + e_j), |e_j| <= u, and t_j^2 passes at most D fmaf roundings; the
//            chain differs from D2 = sum_j (q_j - x_j)^2 <= R by at most gamma_{D+2} D2:                    <= 1.01 (D + 2) u R
//   dot:     a product of two fp16 values is exact in fp32, and dot is SOME fp32 accumulation of the D exact products: the
//            matrix instruction's order and rounding mode are its own.  Model: any summation tree, every addition rounded to
//            nearest or truncated, relative error <= 2 u = 2^-23 (the model of the fp16 inner-product certificate).  A product
//            passes at most D additions: |dot - q.x| <= ((1 + 2 u)^D - 1) sum |q_j x_j| <= 1.01 * 2 D u P (2 D u <= 2^-7).  It
//            enters sigma twice: 4.04 D u P, and P <= R / 4 (arithmetic and geometric mean):                    <= 1.01 D u R
//   xsq:     one rounding of an fp64 sum, |xsq - ||x||^2| <= (u + D 2^-53) ||x||^2 <= 1.01 u X^2:                <= 1.01 u R
//   fmaf:    the one rounding of sigma (a vector-ALU fma, to nearest) is at most u |2 dot - xsq| <= u (2.02 P + 1.01 X^2), and
//            2 P + X^2 <= R:                                                                                     <= 1.02 u R
//   sum:     (2.02 D + 4.06) u R <= 2.5 D_pad u R for every D >= 1, D_pad = D rounded up to 16 (D <= 16: 2.02 * 16 + 4.06
//            < 40; D > 16: 0.48 D > 7.68 > 4.06).                                                         E_q = 2.5 D_pad u R
//   range:   a finite fp16 value is below 2^16, so ||q||, X <= 2^16 sqrt(D) <= 2^24 and R <= 2^50 for D <= 65536: dot, xsq,
//            sigma and d stay below 2^52, nothing overflows.  The range term of the fp32 bound vanishes.  (An X that is not
//            such a norm — inf, NaN — makes E_q inf or NaN: not certified.)
//   under:   a non-zero fp16 value is a multiple of 2^-24 of magnitude >= 2^-24.  So every product is a multiple of 2^-48,
//            every t_j = fl(q_j - x_j) a multiple of 2^-24 and every square a multiple of 2^-48, and so is every partial sum:
//            a multiple of 2^-48 below 2^-24 has at most 24 significant bits and is exact in fp32, a larger one rounds to a
//            multiple of its ulp >= 2^-48.  Every intermediate of the screen and of the chain is therefore 0 or >= 2^-48, far
//            above 2^-126: no fp32 result is subnormal, no fp32 operand is one, the roundings are all relative.  The flush and
//            underflow terms of the fp32 bound vanish.
//   fp16 subnormals as matrix operands: the one term the argument above does not reach is a matrix core that would read an
//            fp16 subnormal (|a| < 2^-14) as zero.  The f16 instructions do not: the fp16 inner-product certificate carries no
//            such term on the strength of its hardware test over subnormal operand families
//            (profiles/dense_f16_pytest_gpu.txt: errors of 1e-11 where a flushed operand would cost the whole score), and this
//            search runs the same instruction on the same operands; tests/test_dense_l2_f16.py repeats those families against
//            this screen (profiles/dense_l2_f16_pytest_gpu.txt).
//   The constant is exported (rc_dense_l2_f16_error_constants) and is what ops.dense_l2_f16_error_bound evaluates.
//
// Certificate: as in dense_search_l2.hip, t >= thr~ - ss_down + E_q with t = the k-th best -d of the list; V::eq is E_q
// (pushed upwards) minus the query's squared norm (pushed downwards), in fp64.  A non-finite query value (an fp32 query of
// magnitude >= 65520 rounds to an fp16 inf) or D > 65536 is refused: the exact route answers.
#include "dense_f16_gemm.h"
#include "dense_l2.h"

#define DENSE_L2_F16_C_REL 2.5                           // E_q = C_REL D_pad 2^-24 (||q|| + X)^2
#define DENSE_L2_F16_MAX_D 65536                         // the bound is proven up to here

struct dense_l2_f16_variant : dense_variant_defaults<dense_l2_f16_variant> {
    typedef _Float16 T;
    typedef _Float16 Q;
    static constexpr bool approximate = true;
    static constexpr bool l2 = true;
    static constexpr bool subset = true;
    template <int MODE, typename... A>
    static int launch_gemm(rc_handle_t h, const dense_operands& o, A... a) {
        return o.rows ? dense_f16_launch_gemm<MODE, true, true>(h, o, a...) : dense_f16_launch_gemm<MODE, true>(h, o, a...);
    }
    static int exact_rows(rc_handle_t h, const dense_operands& o, const T* x, int64_t ldx, int64_t N, int D, const T* q, int nq,
                          float* out, hipStream_t s) {
        return o.rows ? dense_l2_launch_exact_rows<T, true>(h, o, x, ldx, N, D, q, nq, out, s)
                      : dense_l2_launch_exact_rows<T>(h, o, x, ldx, N, D, q, nq, out, s);
    }
    static constexpr auto* finish = &dense_l2_launch_negate;
    __device__ static bool refuse(float v, int D) { return !(v - v == 0.f) || D > DENSE_L2_F16_MAX_D; }
    // E_q - ss_down: what is added to thr~ (header)
    __device__ static double eq(int D, double ss, double xnorm) {
        const double up = 1.0 + 0x1p-30;
        const double dpad = (double)((D + 15) / 16 * 16);
        const double r = (sqrt(ss) + xnorm) * up, R = r * r * up;
        return DENSE_L2_F16_C_REL * dpad * 0x1p-24 * R * up - ss * (1.0 - 0x1p-30);
    }
};

static const _Float16* dense_l2_f16_ptr(const uint16_t* p) { return reinterpret_cast<const _Float16*>(p); }

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" void rc_dense_l2_f16_error_constants(double* c) {
    c[0] = DENSE_L2_F16_C_REL;
    c[1] = DENSE_L2_F16_MAX_D;
}

extern "C" size_t rc_dense_l2_f16_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_exact_ws_bytes<dense_l2_f16_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_l2_f16_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_l2_f16_variant>(N, D, nq, k);
}

extern "C" int rc_dense_l2_f16_search_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                            int nq, int k, int64_t id_offset, float* dist, int64_t* ids, void* ws,
                                            size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_l2_f16_variant>(h, dense_l2_f16_ptr(x), ldx, N, D, dense_l2_f16_ptr(q), nq, {}, false, 0, k,
                                                   id_offset, dist, ids, ws, ws_bytes, stream);
}

extern "C" int rc_dense_l2_f16_search_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                        int nq, const float* xsq, const float* xnorm_max, int k, int64_t id_offset,
                                        double sel_slack, float* dist, int64_t* ids, int* status, int* qstatus, void* ws,
                                        size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_l2_f16_variant>(h, dense_l2_f16_ptr(x), ldx, N, D, dense_l2_f16_ptr(q), nq, {xsq}, xnorm_max,
                                                    false, 0, k, id_offset, sel_slack, dist, ids, status, qstatus, ws, ws_bytes,
                                                    stream);
}

extern "C" int rc_dense_l2_f16_scores(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                      const float* xsq, float* out, rc_stream_t stream) {
    return dense_scores_entry<dense_l2_f16_variant>(h, dense_l2_f16_ptr(x), ldx, N, D, dense_l2_f16_ptr(q), nq, {xsq}, out, nullptr,
                                                    0, stream);
}

extern "C" int rc_dense_l2_f16_search_rows_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D,
                                                 const uint16_t* q, int nq, const int64_t* rows, int64_t ns, int k,
                                                 int64_t id_offset, float* dist, int64_t* ids, void* ws, size_t ws_bytes,
                                                 rc_stream_t stream) {
    return dense_exact_entry<dense_l2_f16_variant>(h, dense_l2_f16_ptr(x), ldx, N, D, dense_l2_f16_ptr(q), nq,
                                                   {nullptr, nullptr, rows}, true, ns, k, id_offset, dist, ids, ws, ws_bytes,
                                                   stream);
}

extern "C" int rc_dense_l2_f16_search_rows_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                             int nq, const float* xsq, const float* xnorm_max, const int64_t* rows, int64_t ns,
                                             int k, int64_t id_offset, double sel_slack, float* dist, int64_t* ids, int* status,
                                             int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_l2_f16_variant>(h, dense_l2_f16_ptr(x), ldx, N, D, dense_l2_f16_ptr(q), nq, {xsq, nullptr, rows},
                                                    xnorm_max, true, ns, k, id_offset, sel_slack, dist, ids, status, qstatus, ws,
                                                    ws_bytes, stream);
}
