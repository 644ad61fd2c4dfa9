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
// The route of a search (sample -> threshold -> FILTER -> select, or the exact route for small N) is dense_search_route
// (dense_screen.h) with this unit's variant: the fp32 GEMM is sample screen, FILTER screen and exact route at once, its scores
// are the chain, so nothing is rescored or certified.  The GEMM kernel and the workspace layouts are in dense_gemm.h.
#include "dense_screen.h"

// the fp32 GEMM, through o.rows for a subset: the screen in both modes and the exact route's rows
template <int MODE, typename... A>
static int dense_f32_launch_gemm(rc_handle_t h, const dense_operands& o, A... a) {
    return o.rows ? dense_launch_gemm<MODE, float, true>(h, o, a...) : dense_launch_gemm<MODE, float>(h, o, a...);
}

int dense_exact_rows_f32(rc_handle_t h, const dense_operands& o, const float* x, int64_t ldx, int64_t N, int D, const float* q,
                         int nq, float* out, hipStream_t s) {
    return dense_f32_launch_gemm<DENSE_STORE>(h, o, x, ldx, N, N, 0, q, nq, D, nullptr, out, nullptr, nullptr, s);
}

// ---- the id map of the subset searches (declared in dense_screen.h, shared by the four units that serve them) -----------------
// ids [n]: the select's output over x[rows] with id_offset 0, a row of x[rows] or -1 -> id_offset + its corpus row, -1 stays
__global__ __launch_bounds__(256) void dense_map_ids_kernel(int64_t* __restrict__ ids, int64_t n,
                                                            const int64_t* __restrict__ rows, int64_t id_offset) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id >= 0) ids[i] = id_offset + rows[id];
}

int dense_launch_map_ids(rc_handle_t h, int64_t* ids, int64_t n, const int64_t* rows, int64_t id_offset, hipStream_t s) {
    hipLaunchKernelGGL(dense_map_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, n, rows, id_offset);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
// the same map for a caller that searched a selection itself (the ADC subset searches: rc_adc_select_rows, a search with
// id_offset 0, then this): ids[i] <- id_offset + rows[ids[i]] for the n ids >= 0, -1 stays
extern "C" int rc_map_ids(rc_handle_t h, int64_t* ids, int64_t n, const int64_t* rows, int64_t id_offset, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (n < 0) return RC_ESHAPE;
    if (!h || !ids || !rows) return RC_EINVAL;
    if (n == 0) return RC_OK;
    return dense_launch_map_ids(h, ids, n, rows, id_offset, (hipStream_t)stream);
}

struct dense_f32_variant : dense_variant_defaults<dense_f32_variant> {
    typedef float T;
    typedef float Q;
    static constexpr bool approximate = false;
    static constexpr bool subset = true;
    static constexpr bool screen_aligned = true;
    template <int MODE, typename... A>
    static int launch_gemm(A... a) { return dense_f32_launch_gemm<MODE>(a...); }
    static constexpr auto* exact_rows = &dense_exact_rows_f32;
};

extern "C" size_t rc_dense_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_exact_ws_bytes<dense_f32_variant>(N, D, nq, k);
}

extern "C" size_t rc_dense_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_f32_variant>(N, D, nq, k);
}

extern "C" int rc_dense_search_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                     int k, int64_t id_offset, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                                     rc_stream_t stream) {
    return dense_exact_entry<dense_f32_variant>(h, x, ldx, N, D, q, nq, {}, false, 0, k, id_offset, scores, ids, ws, ws_bytes,
                                                stream);
}

extern "C" int rc_dense_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                                 int64_t id_offset, double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus,
                                 void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_f32_variant>(h, x, ldx, N, D, q, nq, {}, nullptr, false, 0, k, id_offset, sel_slack, scores,
                                                 ids, status, qstatus, ws, ws_bytes, stream);
}

extern "C" int rc_dense_search_rows_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                          const int64_t* rows, int64_t ns, int k, int64_t id_offset, float* scores, int64_t* ids,
                                          void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_f32_variant>(h, x, ldx, N, D, q, nq, {nullptr, nullptr, rows}, true, ns, k, id_offset, scores,
                                                ids, ws, ws_bytes, stream);
}

extern "C" int rc_dense_search_rows_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                      const int64_t* rows, int64_t ns, int k, int64_t id_offset, double sel_slack, float* scores,
                                      int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_f32_variant>(h, x, ldx, N, D, q, nq, {nullptr, nullptr, rows}, nullptr, true, ns, k, id_offset,
                                                 sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream);
}
