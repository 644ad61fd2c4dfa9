// Exact dense L2 top-k search (Faiss IndexFlatL2, the flat index the reference names at evaluate_repconc.py:102 and
// run_warmup.py:102,107) over an fp32 corpus: smallest squared Euclidean distance first, lowest row first among equals.
//
// Distance: d(q, n) = the fp32 chain  acc = +0.0f;  for j = 0 .. D-1 ascending:  t = q[j] - x[n][j] (one fp32 subtraction),
// acc = fmaf(t, t, acc).  The direct form, so ids AND distance bits are defined as the inner-product search defines its
// scores; d >= +0 always (t t >= +0 and the chain starts at +0: no -0, zero-padding a chunk of K is bit-neutral).  Every stage
// works on s = -d with the keys of topk.h (negation is exact, every zero is -0.0f, "largest s, lowest row" is "smallest d,
// lowest row"); the entries negate the k output values once at the end: d ascending, +0.0f for a zero, +inf / -1 past N.
//
// Route: dense_search_route (dense_screen.h) with this unit's variant.
//   N <= DENSE_EXACT_MAX_N, and the queries the fast route gives up on: dense_l2_exact_kernel (dense_l2.h) writes the full
//   rows of -d of a chunk of queries (dense_exact), then the radix select (topk_exact_select), then the sign.
//   Above:  1. screen<STORE> over the strided sample  2. threshold  3. screen<FILTER> over all rows, xsq passed to both
//   4. dense_rescore_kernel<.., L2 = true> replaces the score half of every candidate key by -d  5. select
//   6. dense_certify_kernel  7. dense_l2_negate_kernel (the variant's finish).
//
// Screen.  sigma(q, n) = fmaf(2, dot(q, x_n), -xsq[n]): dot is the fp32 MFMA accumulator of the GEMM of dense_gemm.h
// (dense_gemm_body<.., L2 = true>), xsq[n] the caller's fp32 squared norm of row n (an fp64 sum rounded to nearest,
// ops.dense_row_sqnorms).  sigma = ||q||^2 - d up to rounding: it differs from -d by a constant per query, so the sample, the
// threshold and the FILTER run on sigma unchanged.  The expanded form cancels and has no defined bits: it only screens.
//
// The bound |sigma - ||q||^2 + d| <= E_q.  u = 2^-24, X >= the largest row norm, P = ||q|| X, R = (||q|| + X)^2, gamma_n =
// n u / (1 - n u) <= 1.01 n u while n <= 65538 (above D = 65536 no certificate is given).
//   chain:   t_j = (q_j - x_j)(1 + e_j), |e_j| <= u; the term t_j^2 passes at most D fmaf roundings: the chain differs from
//            D2 = sum_j (q_j - x_j)^2 by at most gamma_{D+2} D2, and D2 = ||q - x||^2 <= R:                 <= 1.01 (D + 2) u R
//   screen:  the MFMA accumulator is the fmaf chain of the products: |dot - q.x| <= gamma_D sum |q_j x_j| <= 1.01 D u P, and it
//            enters twice; |xsq - ||x||^2| <= (u + D 2^-53) ||x||^2 <= 1.01 u X^2; the one fmaf rounding of sigma is at most
//            u |sigma| <= 1.01 u (2 P + X^2):                                             <= (2.02 D + 2.02) u P + 2.02 u X^2
//   with P <= R / 4 (arithmetic and geometric mean) and X^2 <= R:  (1.01 D + 2.02 + 0.505 D + 0.505 + 2.02) u R
//            = (1.515 D + 4.545) u R <= 2 D_pad u R for every D >= 1, D_pad = D rounded up to 16 (D < 16: 1.515 D + 4.545 < 28 <= 32;
//            D >= 16: 0.485 D >= 7.7).                                                                 E_rel = 2 D_pad u R
//   flush:   a matrix core that reads an fp32 subnormal operand (|a| < 2^-126) as zero drops the product a b, |a b| < 2^-126 |b|:
//            over the row at most 2^-126 (sum |q_j| + sum |x_j|) <= 2^-126 sqrt(D) (||q|| + X), twice in sigma; no measurement
//            decides whether this term is needed, it is always paid:                 E_flush = 4 * 2^-126 sqrt(D_pad) (||q|| + X)
//   under:   a result below 2^-126 is rounded to a multiple of 2^-149 instead of relatively: D roundings of the chain (the
//            subtraction is exact there), 2 D + 1 of the screen, each <= 2^-150:                     E_under = 4 D_pad 2^-149
//   range:   R < 2^126 keeps every intermediate finite (|dot| <= 1.01 P < 2^125, xsq <= 1.01 X^2, d <= 1.01 R).  Otherwise a
//            sigma may be inf or NaN and fail the FILTER's comparison: no certificate, the exact route answers.
//   E_q = E_rel + E_flush + E_under; the constants are exported (rc_dense_l2_error_constants) and are what
//   ops.dense_l2_error_bound evaluates.
//
// Certificate.  A row outside the list has sigma < thr~, hence -d < thr~ - ||q||^2 + E_q: with t = the k-th best -d of the list,
// t >= thr~ - ss_down + E_q proves that no such row enters the top-k or ties with its last member.  dense_certify_kernel adds
// V::eq to thr~: here E_q (pushed upwards) minus the query's squared norm (pushed downwards), all in fp64.
#include "dense_l2.h"

#define DENSE_L2_C_REL 2.0                               // E_rel   = C_REL D_pad 2^-24 (||q|| + X)^2
#define DENSE_L2_C_FLUSH 0x1p-124                        // E_flush = C_FLUSH sqrt(D_pad) (||q|| + X)        (4 * 2^-126)
#define DENSE_L2_C_UNDER 0x1p-147                        // E_under = C_UNDER D_pad                          (4 * 2^-149)
#define DENSE_L2_MAX_D 65536                             // gamma_n <= 1.01 n u up to here
#define DENSE_L2_MAX_R 0x1p126                           // (||q|| + X)^2 below this: nothing overflows

// ---- screen: the fp32 GEMM with the L2 epilogue ------------------------------------------------------------------------------
// grid and arguments as dense_gemm_kernel, plus xsq [N] (MAP: read at the corpus row, as x is).
template <int MODE, bool PAD, bool MAP = false>
__global__ __launch_bounds__(256) void dense_l2_gemm_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int64_t nrows,
                                                            int64_t smap, const float* __restrict__ q, int nq, int D,
                                                            const float* __restrict__ thr, float* __restrict__ out,
                                                            unsigned* __restrict__ cnt, unsigned long long* __restrict__ cand,
                                                            const float* __restrict__ xsq,
                                                            const int64_t* __restrict__ rows) {
    dense_gemm_body<MODE, PAD, float, true, MAP>(x, ldx, N, nrows, smap, q, nq, D, thr, out, cnt, cand, xsq, rows);
}

// o.rows is read only if MAP: a template argument, as in dense_launch_gemm
template <int MODE, bool MAP = false>
static int dense_l2_launch_gemm(rc_handle_t h, const dense_operands& o, const float* x, int64_t ldx, int64_t N, int64_t nrows,
                                int64_t smap, const float* q, int nq, int D, const float* thr, float* out, unsigned* cnt,
                                unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (D % DENSE_KC == 0)
        hipLaunchKernelGGL((dense_l2_gemm_kernel<MODE, false, MAP>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand, o.xsq, o.rows);
    else
        hipLaunchKernelGGL((dense_l2_gemm_kernel<MODE, true, MAP>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand, o.xsq, o.rows);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ---- the sign at the end (declared in dense_l2.h, the finish of both L2 units) ------------------------------------------------
// -d -> d in place over the n output values: -0.0f -> +0.0f, the -inf of the padding -> +inf
__global__ __launch_bounds__(256) void dense_l2_negate_kernel(float* __restrict__ v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = -v[i];
}

int dense_l2_launch_negate(rc_handle_t h, float* v, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(dense_l2_negate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, n);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// the exact route's rows, also for dense_search_l2_bf16x3.hip (declared in dense_l2.h)
int dense_l2_exact_rows_f32(rc_handle_t h, const dense_operands& o, const float* x, int64_t ldx, int64_t N, int D, const float* q,
                            int nq, float* out, hipStream_t s) {
    return o.rows ? dense_l2_launch_exact_rows<float, true>(h, o, x, ldx, N, D, q, nq, out, s)
                  : dense_l2_launch_exact_rows<float>(h, o, x, ldx, N, D, q, nq, out, s);
}

// ---- the variant -------------------------------------------------------------------------------------------------------------
struct dense_l2_variant : dense_variant_defaults<dense_l2_variant> {
    typedef float T;
    typedef float Q;
    static constexpr bool approximate = true;
    static constexpr bool l2 = true;
    static constexpr bool subset = true;
    static constexpr bool screen_aligned = true;
    template <int MODE, typename... A>
    static int launch_gemm(rc_handle_t h, const dense_operands& o, A... a) {
        return o.rows ? dense_l2_launch_gemm<MODE, true>(h, o, a...) : dense_l2_launch_gemm<MODE>(h, o, a...);
    }
    static constexpr auto* exact_rows = &dense_l2_exact_rows_f32;
    static constexpr auto* finish = &dense_l2_launch_negate;
    __device__ static bool refuse(float v, int D) { return !(v - v == 0.f) || D > DENSE_L2_MAX_D; }
    // E_q - ss_down: what is added to thr~ (header).  +inf (never certified) unless (||q|| + X)^2 < 2^126.
    __device__ static double eq(int D, double ss, double xnorm) {
        const double up = 1.0 + 0x1p-30;
        const double dpad = (double)((D + 15) / 16 * 16);
        const double r = (sqrt(ss) + xnorm) * up, R = r * r * up;
        if (!(R < DENSE_L2_MAX_R)) return INFINITY;
        const double e = (DENSE_L2_C_REL * dpad * 0x1p-24 * R + DENSE_L2_C_FLUSH * sqrt(dpad) * up * r + DENSE_L2_C_UNDER * dpad) * up;
        return e - ss * (1.0 - 0x1p-30);
    }
};

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" void rc_dense_l2_error_constants(double* c) {
    c[0] = DENSE_L2_C_REL;
    c[1] = DENSE_L2_C_FLUSH;
    c[2] = DENSE_L2_C_UNDER;
}

extern "C" size_t rc_dense_l2_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_exact_ws_bytes<dense_l2_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_l2_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_l2_variant>(N, D, nq, k);
}

extern "C" int rc_dense_l2_search_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                        int k, int64_t id_offset, float* dist, int64_t* ids, void* ws, size_t ws_bytes,
                                        rc_stream_t stream) {
    return dense_exact_entry<dense_l2_variant>(h, x, ldx, N, D, q, nq, {}, false, 0, k, id_offset, dist, ids, ws, ws_bytes, stream);
}

extern "C" int rc_dense_l2_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                    const float* xsq, const float* xnorm_max, int k, int64_t id_offset, double sel_slack,
                                    float* dist, int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes,
                                    rc_stream_t stream) {
    return dense_search_entry<dense_l2_variant>(h, x, ldx, N, D, q, nq, {xsq}, xnorm_max, false, 0, k, id_offset, sel_slack, dist,
                                                ids, status, qstatus, ws, ws_bytes, stream);
}

extern "C" int rc_dense_l2_scores(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                  const float* xsq, float* out, rc_stream_t stream) {
    return dense_scores_entry<dense_l2_variant>(h, x, ldx, N, D, q, nq, {xsq}, out, nullptr, 0, stream);
}

extern "C" int rc_dense_l2_search_rows_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                             const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* dist, int64_t* ids,
                                             void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_l2_variant>(h, x, ldx, N, D, q, nq, {nullptr, nullptr, rows}, true, ns, k, id_offset, dist, ids,
                                               ws, ws_bytes, stream);
}

extern "C" int rc_dense_l2_search_rows_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                         const float* xsq, const float* xnorm_max, const int64_t* rows, int64_t ns, int k,
                                         int64_t id_offset, double sel_slack, float* dist, int64_t* ids, int* status, int* qstatus,
                                         void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_l2_variant>(h, x, ldx, N, D, q, nq, {xsq, nullptr, rows}, xnorm_max, true, ns, k, id_offset,
                                                sel_slack, dist, ids, status, qstatus, ws, ws_bytes, stream);
}
