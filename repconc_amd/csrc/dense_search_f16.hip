// Exact dense inner-product top-k search over an fp16 corpus (Faiss IndexFlatIP with useFloat16 = True): the corpus is half
// the bytes of dense_search.hip's and the screen runs on the f16 matrix cores, 16x the fp32 matrix rate.
//
// Score: x and q are IEEE fp16; s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f over the widened values —
// the definition of dense_search.hip applied to x.float(), q.float().  A product of two fp16 values is exact in fp32, but
// the f16 matrix instruction sums the products of a K step in an order of its own: what it computes is a SCREEN, s~, never a result.
//
// The route is dense_search_route (dense_screen.h) with this unit's variant: dense_f16_gemm_kernel (dense_f16_gemm.h) screens,
// the candidates are rescored by the chain and every answer carries a certificate (steps 4 and 6 there) with
//     E_q = DENSE_F16_ERR_C * D_pad * 2^-24 * ||q||_2 * X,   X >= the largest row norm of the corpus, D_pad = D up to 16:
// every |s~ - s| <= E_q, both are fp32 sums of the same D exact products and each errs by < D ulps of sum |q_d x_d|.
// Exact route: dense_gemm_kernel<STORE, PAD, _Float16> (dense_gemm.h), instantiated here alone.
#include "dense_f16_gemm.h"

#define DENSE_F16_ERR_C 4.0                              // the certificate's constant (rc_dense_f16_error_constant)

struct dense_f16_variant : dense_variant_defaults<dense_f16_variant> {
    typedef _Float16 T;
    typedef _Float16 Q;
    static constexpr bool approximate = true;
    static constexpr bool subset = true;
    template <int MODE, typename... A>
    static int launch_gemm(rc_handle_t h, const dense_operands& o, A... a) {
        return o.rows ? dense_f16_launch_gemm<MODE, false, true>(h, o, a...) : dense_f16_launch_gemm<MODE, false>(h, o, a...);
    }
    static int exact_rows(rc_handle_t h, const dense_operands& o, const T* x, int64_t ldx, int64_t N, int D, const T* q, int nq,
                          float* out, hipStream_t s) {
        return o.rows ? dense_launch_gemm<DENSE_STORE, T, true>(h, o, x, ldx, N, N, 0, q, nq, D, nullptr, out, nullptr, nullptr, s)
                      : dense_launch_gemm<DENSE_STORE, T>(h, o, x, ldx, N, N, 0, q, nq, D, nullptr, out, nullptr, nullptr, s);
    }
    __device__ static bool refuse(float, int) { return false; }
    __device__ static double eq(int D, double ss, double xnorm) {
        const double up = 1.0 + 0x1p-30;
        const int dpad = (D + 15) / 16 * 16;
        return DENSE_F16_ERR_C * (double)dpad * 0x1p-24 * (sqrt(ss) * up) * xnorm * up;
    }
};

static const _Float16* dense_f16_ptr(const uint16_t* p) { return reinterpret_cast<const _Float16*>(p); }

extern "C" double rc_dense_f16_error_constant(void) { return DENSE_F16_ERR_C; }
extern "C" int rc_dense_f16_screen_form(void) { return 16; }

extern "C" size_t rc_dense_f16_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_exact_ws_bytes<dense_f16_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_f16_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_f16_variant>(N, D, nq, k);
}

extern "C" int rc_dense_f16_search_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                         int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                         size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_f16_variant>(h, dense_f16_ptr(x), ldx, N, D, dense_f16_ptr(q), nq, {}, false, 0, k, id_offset,
                                                scores, ids, ws, ws_bytes, stream);
}

extern "C" int rc_dense_f16_scores(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                   float* out, rc_stream_t stream) {
    return dense_scores_entry<dense_f16_variant>(h, dense_f16_ptr(x), ldx, N, D, dense_f16_ptr(q), nq, {}, out, nullptr, 0, stream);
}

extern "C" int rc_dense_f16_search_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                     const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores,
                                     int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_f16_variant>(h, dense_f16_ptr(x), ldx, N, D, dense_f16_ptr(q), nq, {}, xnorm_max, false, 0, k,
                                                 id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream);
}

extern "C" int rc_dense_f16_search_rows_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                              int nq, const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* scores,
                                              int64_t* ids, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_f16_variant>(h, dense_f16_ptr(x), ldx, N, D, dense_f16_ptr(q), nq, {nullptr, nullptr, rows}, true,
                                                ns, k, id_offset, scores, ids, ws, ws_bytes, stream);
}

extern "C" int rc_dense_f16_search_rows_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                          int nq, const float* xnorm_max, const int64_t* rows, int64_t ns, int k, int64_t id_offset,
                                          double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus, void* ws,
                                          size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_f16_variant>(h, dense_f16_ptr(x), ldx, N, D, dense_f16_ptr(q), nq, {nullptr, nullptr, rows},
                                                 xnorm_max, true, ns, k, id_offset, sel_slack, scores, ids, status, qstatus, ws,
                                                 ws_bytes, stream);
}
