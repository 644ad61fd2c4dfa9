// Exact dense inner-product top-k search over an fp16 corpus (Faiss IndexFlatIP with useFloat16 = True): the corpus is half
// the bytes of dense_search.hip's and the screen runs on the f16 matrix cores, 16x the fp32 matrix rate.
//
// Score: x and q are IEEE fp16; s(q, n) = fp32 fmaf chain over d = 0 .. D-1 ascending from +0.0f over the widened values —
// the definition of dense_search.hip applied to x.float(), q.float().  A product of two fp16 values is exact in fp32, but
// the f16 matrix instruction sums the products of a K step in an order of its own: what it computes is a SCREEN, s~, never a result.
//
// The route is dense_search_route (dense_screen.h) with this unit's variant: dense_f16_gemm_kernel screens, the candidates
// are rescored by the chain and every answer carries a certificate (steps 4 and 6 there) with
//     E_q = DENSE_F16_ERR_C * D_pad * 2^-24 * ||q||_2 * X,   X >= the largest row norm of the corpus, D_pad = D up to 16:
// every |s~ - s| <= E_q, both are fp32 sums of the same D exact products and each errs by < D ulps of sum |q_d x_d|.
// Exact route: dense_gemm_kernel<STORE, PAD, _Float16> (dense_gemm.h), instantiated here alone.
#include "dense_screen.h"

typedef _Float16 dense_f16x8 __attribute__((ext_vector_type(8)));
#define DENSE_F16_KC 64                                  // halves of K per LDS stage: 128-byte rows, 8 chunks of 16 bytes
#define DENSE_F16_ERR_C 4.0                              // the certificate's constant (rc_dense_f16_error_constant)

// grid: ceil(nrows / 128) blocks of 256 threads, two per CU (64 KB of LDS each).  Arguments as dense_gemm_kernel; x and q are
// fp16.  !PAD: D % 8 == 0, 16-byte aligned rows; PAD assembles its chunks element by element.  The block owns 128 corpus rows
// and walks every tile of 128 queries; tiling, operand map and epilogue of v_mfma_f32_16x16x32_f16 as laid out in
// dense_screen.h, one 16-byte LDS read per operand tile and K step.  (v_mfma_f32_32x32x16_f16 at 2 x 2 tiles per wave was
// measured slower, 28.0 ms against 27.1 ms per FILTER launch over 8 841 823 x 768, and is retired: DESIGN.md 4.9,
// profiles/dense_f16_form_ab.txt.)
template <int MODE, bool PAD>
__global__ __launch_bounds__(256, 2) void dense_f16_gemm_kernel(const _Float16* __restrict__ x, int64_t ldx, int64_t N,
                                                             int64_t nrows, int64_t smap, const _Float16* __restrict__ q,
                                                             int nq, int D, const float* __restrict__ thr,
                                                             float* __restrict__ out, unsigned* __restrict__ cnt,
                                                             unsigned long long* __restrict__ cand) {
    constexpr int TM = 16, NT = 4, KS = 32;
    __shared__ __attribute__((aligned(16))) unsigned char dense_f16_smem[DENSE_SCREEN_LDS_BYTES];
    unsigned char* sa = dense_f16_smem;                                     // [2][128 rows][128 bytes] queries
    unsigned char* sb = dense_f16_smem + 2 * DENSE_SCREEN_OPERAND_BYTES;    // [2][128 rows][128 bytes] corpus
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l % TM, grp = l / TM;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> chunk lc = tid % 8 of rows tid / 8 + 32 i, i < 4 (8 threads read 128 contiguous bytes of a row)
    const int lrow = tid >> 3, lc = tid & 7;
    const _Float16* xp[4];
    int so[4];                                                             // swizzled LDS offsets of the four chunks
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t jl = (j0 + lrow + 32 * i < nrows) ? j0 + lrow + 32 * i : nrows - 1;
        const int64_t xrow = smap ? (int64_t)((uint64_t)jl * (uint64_t)N / (uint64_t)smap) : jl;
        xp[i] = x + xrow * ldx;
        so[i] = dense_screen_lds_off(lrow + 32 * i, lc);
    }
    const int nkc = (D + DENSE_F16_KC - 1) / DENSE_F16_KC;
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        const _Float16* qp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qp[i] = q + (int64_t)((qt + lrow + 32 * i < nq) ? qt + lrow + 32 * i : nq - 1) * D;
        dense_f32x4 acc[NT][NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
        dense_f16x8 ra[4], rb[4];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_F16_KC + lc * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (PAD) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        ra[i][e] = (k0 + e < D) ? qp[i][k0 + e] : (_Float16)0;
                        rb[i][e] = (k0 + e < D) ? xp[i][k0 + e] : (_Float16)0;
                    }
                } else if (k0 < D) {                                        // D % 8 == 0: a chunk is inside or outside
                    ra[i] = *reinterpret_cast<const dense_f16x8*>(qp[i] + k0);
                    rb[i] = *reinterpret_cast<const dense_f16x8*>(xp[i] + k0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { ra[i][e] = (_Float16)0; rb[i][e] = (_Float16)0; }
                }
            }
        };
        auto sstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<dense_f16x8*>(sa + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = ra[i];
                *reinterpret_cast<dense_f16x8*>(sb + buf * DENSE_SCREEN_OPERAND_BYTES + so[i]) = rb[i];
            }
        };
        // query tiles that hold only padding skip their MFMAs, wave-uniformly (a call with <= 32 queries issues a quarter of
        // the matrix work and is bounded by the corpus read)
        bool act[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) act[a] = qt + wr * 64 + a * TM < nq;
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
            const unsigned char* pa = sa + buf * DENSE_SCREEN_OPERAND_BYTES;
            const unsigned char* pb = sb + buf * DENSE_SCREEN_OPERAND_BYTES;
#pragma unroll
            for (int ks = 0; ks < DENSE_F16_KC / KS; ++ks) {
                dense_f16x8 fa[NT], fb[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    fa[t] = *reinterpret_cast<const dense_f16x8*>(pa + dense_screen_lds_off(wr * 64 + t * TM + col, (KS / 8) * ks + grp));
                    fb[t] = *reinterpret_cast<const dense_f16x8*>(pb + dense_screen_lds_off(wc * 64 + t * TM + col, (KS / 8) * ks + grp));
                }
#pragma unroll
                for (int a = 0; a < NT; ++a)
                    if (act[a])
#pragma unroll
                        for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        const float* s_thr = dense_screen_stage_thr<MODE>(sa, nkc, thr, qt, nq, tid);
        dense_screen_epilogue<MODE>(acc, j0, wr, wc, col, grp, qt, nq, s_thr, nrows, out, cnt, cand, l);
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

static bool dense_f16_aligned(const void* x, int64_t ldx, const void* q, int D) {
    return D % 8 == 0 && ldx % 8 == 0 && !((uintptr_t)x & 15u) && !((uintptr_t)q & 15u);
}

template <int MODE>
static int dense_f16_launch_gemm(rc_handle_t h, const _Float16* x, int64_t ldx, int64_t N, int64_t nrows, int64_t smap,
                                 const _Float16* q, int nq, int D, const float* thr, float* out, unsigned* cnt,
                                 unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (dense_f16_aligned(x, ldx, q, D))
        hipLaunchKernelGGL((dense_f16_gemm_kernel<MODE, false>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand);
    else
        hipLaunchKernelGGL((dense_f16_gemm_kernel<MODE, true>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

struct dense_f16_variant : dense_variant_defaults {
    typedef _Float16 T;
    typedef _Float16 Q;
    static constexpr bool approximate = true;
    template <int MODE, typename... A>
    static int launch_gemm(const float*, A... a) { return dense_f16_launch_gemm<MODE>(a...); }
    static int exact_rows(rc_handle_t h, const T* x, int64_t ldx, int64_t N, int D, const T* q, int nq, float* out, hipStream_t s) {
        return dense_launch_gemm<DENSE_STORE, T>(h, x, ldx, N, N, 0, q, nq, D, nullptr, out, nullptr, nullptr, s);
    }
    __device__ static bool refuse(float, int) { return false; }
    __device__ static double eq(int D, double ss, double xnorm) {
        const double up = 1.0 + 0x1p-30;
        const int dpad = (D + 15) / 16 * 16;
        return DENSE_F16_ERR_C * (double)dpad * 0x1p-24 * (sqrt(ss) * up) * xnorm * up;
    }
};

extern "C" double rc_dense_f16_error_constant(void) { return DENSE_F16_ERR_C; }
extern "C" int rc_dense_f16_screen_form(void) { return 16; }

extern "C" size_t rc_dense_f16_search_exact_ws_bytes(int64_t N, int D, int nq, int k) { return dense_exact_ws_bytes(N, D, nq, k); }

extern "C" size_t rc_dense_f16_search_ws_bytes(int64_t N, int D, int nq, int k) {
    return dense_search_ws_bytes<dense_f16_variant>(N, D, nq, k);
}

extern "C" int rc_dense_f16_search_exact(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q,
                                         int nq, int k, int64_t id_offset, float* scores, int64_t* ids, void* ws,
                                         size_t ws_bytes, rc_stream_t stream) {
    return dense_exact_entry<dense_f16_variant>(h, reinterpret_cast<const _Float16*>(x), ldx, N, D,
                                                reinterpret_cast<const _Float16*>(q), nq, k, id_offset, scores, ids, ws, ws_bytes,
                                                stream);
}

extern "C" int rc_dense_f16_scores(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                   float* out, rc_stream_t stream) {
    rc_device_guard device_guard_(h);
    if (N > 0xFFFFFFFFll) return RC_ESHAPE;
    if (!h || !x || !q || !out || N <= 0 || D <= 0 || nq < 0 || ldx < D) return RC_EINVAL;
    if (nq == 0) return RC_OK;
    return dense_f16_launch_gemm<DENSE_STORE>(h, reinterpret_cast<const _Float16*>(x), ldx, N, N, 0,
                                              reinterpret_cast<const _Float16*>(q), nq, D, nullptr, out, nullptr, nullptr,
                                              (hipStream_t)stream);
}

extern "C" int rc_dense_f16_search_q(rc_handle_t h, const uint16_t* x, int64_t ldx, int64_t N, int D, const uint16_t* q, int nq,
                                     const float* xnorm_max, int k, int64_t id_offset, double sel_slack, float* scores,
                                     int64_t* ids, int* status, int* qstatus, void* ws, size_t ws_bytes, rc_stream_t stream) {
    return dense_search_entry<dense_f16_variant>(h, reinterpret_cast<const _Float16*>(x), ldx, N, D,
                                                 reinterpret_cast<const _Float16*>(q), nq, nullptr, xnorm_max, k, id_offset,
                                                 sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream);
}
