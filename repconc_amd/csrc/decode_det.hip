// Deterministic backward of decode (modeling_repconc.py:168-184; autograd of the gather at :175): the centroid gradient summed
// in a fixed order instead of by fp32 atomics (decode_bwd_kernel, pq_misc.hip, whose result depends on the order in which the
// waves arrive).  The arithmetic is fixed on the OUTPUT, as for the JPQ scoring head (DESIGN.md "decode"):
//
//   grad_C[m, c, j] = fp32( sum over the rows r with (codes[r, m] & 255) == c, r ascending, of (double) grad_out[r, m*dsub + j] )
//
// every sum fp64, sequential from 0.0, rounded to fp32 once; an (m, c) that no row hits gets +0.0f.  So grad_C is a function of
// the inputs alone, whatever the launch, and it is OVERWRITTEN (the atomics entry adds into a zeroed buffer).
//
//   code_sort_*_kernel      stable counting sort of the rows by code, per sub-quantiser (code_sort.h, shared with the JPQ
//                           head): perm[m][.] = the rows of every (m, c) segment, ascending; no holes
//   decode_bwd_det_kernel   thread per (m, c, j): the one owner of its output adds its segment in order
//
// No atomics on values (the sort's integer LDS counts are order-free).  Every kernel walks its work with a grid-stride loop, so
// n < 2^31 needs no large grid, and nothing is sized by the shape except the caller's workspace.
#include "rc_common.h"
#include "code_sort.h"

#define DD_U 8                // independent loads in flight ahead of an ordered chain of adds

// the code of row r under m: the low 8 bits of either code dtype (decode reads the same bits)
template <typename CodeT>
struct decode_code_src {
    const CodeT* codes;
    int M;
    __device__ __forceinline__ int operator()(int64_t r, int m) const { return (int)codes[r * M + m] & (RC_K - 1); }
};

// thread per (m, c, j) — the only writer of grad_C[m, c, j] — adds its segment's rows in ascending r; the dsub threads of one
// (m, c) read one contiguous run of each row.  DD_U row numbers and values are fetched ahead of the chain of adds.  An empty
// segment stores (float)0.0 = +0.0f.
__global__ __launch_bounds__(256) void decode_bwd_det_kernel(const float* __restrict__ go, int64_t n, int M, int dsub,
                                                             const unsigned* __restrict__ perm, const unsigned* __restrict__ start,
                                                             const unsigned* __restrict__ count, float* __restrict__ gC) {
    const int64_t D = (int64_t)M * dsub;
    const int64_t total = D * RC_K;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t seg = e / dsub;                    // m * 256 + c
        const int j = (int)(e - seg * dsub);
        const int m = (int)(seg / RC_K);
        const unsigned cnt = count[seg];
        const unsigned* pm = perm + (size_t)m * n + start[seg];
        const float* gd = go + (int64_t)m * dsub + j;
        double acc = 0.0;
        unsigned i = 0;
        for (; i + DD_U <= cnt; i += DD_U) {
            unsigned rr[DD_U];
            float gg[DD_U];
#pragma unroll
            for (int u = 0; u < DD_U; ++u) rr[u] = pm[i + u];
#pragma unroll
            for (int u = 0; u < DD_U; ++u) gg[u] = gd[(int64_t)rr[u] * D];
#pragma unroll
            for (int u = 0; u < DD_U; ++u) acc = acc + (double)gg[u];
        }
        for (; i < cnt; ++i) acc = acc + (double)gd[(int64_t)pm[i] * D];
        gC[e] = (float)acc;
    }
}

extern "C" size_t rc_pq_decode_bwd_det_ws_bytes(int64_t n, int M) {
    if (n <= 0 || M <= 0 || n > 0x7FFFFFFFll) return 0;
    return code_sort_ws::bytes(n, M);
}

extern "C" int rc_pq_decode_bwd_det(rc_handle_t h, const void* codes, int code_dtype, const float* grad_out, int64_t n, int M, int K,
                                    int dsub, float* grad_C, void* ws, size_t ws_bytes, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (!h || !codes || !grad_out || !grad_C || n < 0 || M <= 0 || dsub <= 0) return RC_EINVAL;
    if (K != RC_K || n > 0x7FFFFFFFll || (int64_t)M * dsub > 0x7FFFFFFFll) return RC_ESHAPE;
    if (n == 0) return RC_OK;
    if (code_dtype != RC_CODE_U8 && code_dtype != RC_CODE_I64) return RC_EINVAL;
    if (!ws || ws_bytes < rc_pq_decode_bwd_det_ws_bytes(n, M)) return RC_EWORKSPACE;
    // test switch: the most blocks a launch of this entry may have, so that a small input walks every grid-stride loop
    int64_t max_grid = rc_env_int("RC_DECODE_DET_MAX_GRID", 65536);
    if (max_grid < 1 || max_grid > CS_MAX_GRID) max_grid = CS_MAX_GRID;
    hipStream_t s = (hipStream_t)stream;
    const code_sort_ws L(ws, n, M);
    int rc;
    if (code_dtype == RC_CODE_U8)
        rc = code_sort(h, decode_code_src<uint8_t>{(const uint8_t*)codes, M}, n, M, L, max_grid, s);
    else
        rc = code_sort(h, decode_code_src<int64_t>{(const int64_t*)codes, M}, n, M, L, max_grid, s);
    if (rc != RC_OK) return rc;
    hipLaunchKernelGGL(decode_bwd_det_kernel, dim3(cs_grid((int64_t)M * dsub, max_grid)), dim3(256), 0, s, grad_out, n, M, dsub,
                       (const unsigned*)L.perm, (const unsigned*)L.start, (const unsigned*)L.count, grad_C);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}
