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
// Fast route (N > 4 S):
//   1. dense_gemm_kernel<STORE> over the strided sample j -> row j N / S, S = min(N, 32768) rows: the same chain
//   2. adc_threshold_kernel (topk.hip): thr[q] = the r-th best sample score, r by the ADC formula (rc_adc_sample_rank)
//   3. dense_gemm_kernel<FILTER> over all N rows
//   4. adc_select_kernel (rc_adc_launch_select): sort + emit; qstatus bit0 = fewer than min(k, N) candidates, bit1 = overflow
// Exact route (small N, and the queries the fast route gives up on): dense_gemm_kernel<STORE> writes the full score rows of a
// chunk of queries, then the 8-pass radix select over the 64-bit keys of rc_adc_search_exact (rc_adc_launch_exact_select).
// It terminates with the same answer for any content (all rows identical, k >= N, ...).
// The GEMM kernel, the workspace layouts and the exact route are in dense_gemm.h, shared with the fp16-storage search.
#include "dense_gemm.h"

extern "C" size_t rc_dense_search_exact_ws_bytes(int64_t N, int D, int nq, int k) {
    if (N <= 0 || N > 0xFFFFFFFFll || D <= 0 || nq <= 0 || k <= 0 || k > ADC_CAND_CAP / 2) return 0;
    return dense_exact_ws(N, nq).sel.total;
}

extern "C" size_t rc_dense_search_ws_bytes(int64_t N, int D, int nq, int k) {
    if (N <= 0 || N > 0xFFFFFFFFll || D <= 0 || nq <= 0 || k <= 0 || k > ADC_CAND_CAP / 2) return 0;
    return dense_exact_route(N) ? dense_exact_ws(N, nq).sel.total : dense_fast_ws(N, nq).total;
}

extern "C" int rc_dense_search_exact(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq,
                                     int k, int64_t id_offset, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                                     rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int crc = dense_check(h, x, ldx, N, D, q, nq, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (nq == 0) return RC_OK;
    const dense_exact_layout L = dense_exact_ws(N, nq);
    if (!ws || ws_bytes < L.sel.total) return RC_EWORKSPACE;
    return dense_exact(h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, (char*)ws, L, (hipStream_t)stream);
}

extern "C" int rc_dense_search_q(rc_handle_t h, const float* x, int64_t ldx, int64_t N, int D, const float* q, int nq, int k,
                                 int64_t id_offset, double sel_slack, float* scores, int64_t* ids, int* status, int* qstatus,
                                 void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    const int crc = dense_check(h, x, ldx, N, D, q, nq, k, scores, ids);
    if (crc != RC_OK) return crc;
    if (!status) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    if (!ws || ws_bytes < rc_dense_search_ws_bytes(N, D, nq, k)) return RC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dense_exact_route(N)) return dense_exact(h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, (char*)ws, dense_exact_ws(N, nq), s);
    const dense_fast_layout L = dense_fast_ws(N, nq);
    char* w = (char*)ws;
    float* sample = (float*)(w + L.sample);
    float* thr = (float*)(w + L.thr);
    unsigned* cnt = (unsigned*)(w + L.cnt);
    unsigned long long* cand = (unsigned long long*)(w + L.cand);
    int rc = dense_launch_gemm<DENSE_STORE>(h, x, ldx, N, L.S, L.S, q, nq, D, nullptr, sample, nullptr, nullptr, s);
    if (rc != RC_OK) return rc;
    rc = rc_adc_launch_threshold(h, sample, L.S, nq, rc_adc_sample_rank(N, L.S, k, sel_slack), thr, s);
    if (rc != RC_OK) return rc;
    RC_HIP_CHECK(h, hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), s));
    rc = dense_launch_gemm<DENSE_FILTER>(h, x, ldx, N, N, 0, q, nq, D, thr, nullptr, cnt, cand, s);
    if (rc != RC_OK) return rc;
    return rc_adc_launch_select(h, cand, cnt, nq, N, k, id_offset, scores, ids, status, s, qstatus);
}
