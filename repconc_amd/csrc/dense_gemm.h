// What the seven dense flat searches share (dense_search.hip, dense_search_f16.hip, dense_search_bf16x3.hip,
// dense_search_l2.hip, dense_search_l2_f16.hip, dense_search_l2_bf16x3.hip, dense_search_sq8.hip): the GEMM on the fp32 matrix cores whose result IS the inner-product score (the fp32 fmaf chain over d
// ascending) and, with one more operand, the L2 screen; the workspace layouts and the argument checks.  T is the storage
// type of x and q: float, or _Float16 widened to fp32 on load (exact).  Device code: every translation unit that uses it
// compiles its own copy, no -fgpu-rdc.  The route of a search, exact route included, and what the screened searches share
// on top of this are in dense_screen.h.
#pragma once
#include "topk.h"

#include <stdint.h>

typedef float dense_f32x16 __attribute__((ext_vector_type(16)));
#define DENSE_TILE 128
#define DENSE_KC 16
#define DENSE_LD (DENSE_KC + 1)
#define DENSE_STORE 0
#define DENSE_FILTER 1
#define DENSE_EXACT_MAX_N (4 * ADC_SAMPLE_MAX)      // up to here every call takes the exact route
#define DENSE_EXACT_SC_BYTES (256ull << 20)          // score rows of one exact round
#define DENSE_EXACT_QX_MAX 512

// 8 consecutive elements from a 16-byte aligned address (two 16-byte loads of fp32, one of fp16), widened to fp32
__device__ __forceinline__ void dense_load8(const float* p, float* r) {
    const float4* v = reinterpret_cast<const float4*>(p);
    const float4 a = v[0], b = v[1];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
}
__device__ __forceinline__ void dense_load8(const _Float16* p, float* r) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8 v = *reinterpret_cast<const h8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (float)v[i];
}

// The corpus row behind logical row j of a launch: row j N / smap of the strided sample (smap != 0), j otherwise; MAP (subset
// search): that row of the virtual matrix x[rows], rows [N] ascending.  One rows[] load: call it at block start, never in a K loop.
template <bool MAP>
__device__ __forceinline__ int64_t dense_corpus_row(int64_t j, int64_t N, int64_t smap, const int64_t* __restrict__ rows) {
    const int64_t r = smap ? (int64_t)((uint64_t)j * (uint64_t)N / (uint64_t)smap) : j;
    if constexpr (MAP) return rows[r];
    else return r;
}

// The epilogue of one accumulator element, shared by every screen kernel: score s of query qi and logical row j (jv: j is a
// row).  STORE: out[qi][j] = s.  FILTER: the key of every s >= thr joins qi's candidate list; the GW consecutive lanes that
// hold one query (32 for the 32x32 result layout, 16 for the 16x16 one) ballot and their first survivor takes the slots with
// one global atomic.  Called wave-uniformly (qi differs only between the groups of GW lanes).
template <int MODE, int GW>
__device__ __forceinline__ void dense_emit(float s, int64_t j, bool jv, int qi, int nq, float thr, int64_t nrows,
                                           float* __restrict__ out, unsigned* __restrict__ cnt,
                                           unsigned long long* __restrict__ cand, int l) {
    if constexpr (MODE == DENSE_STORE) {
        if (jv && qi < nq) out[(int64_t)qi * nrows + j] = s;
    } else {
        const bool pass = jv && qi < nq && s >= thr;
        const unsigned long long m = __ballot(pass);
        if (m) {                                                       // wave-uniform
            const int g = l / GW, c = l % GW;
            const unsigned gm = (unsigned)((m >> (g * GW)) & (GW == 32 ? 0xFFFFFFFFull : (1ull << GW) - 1ull));
            const int lead = gm ? __builtin_ctz(gm) : 0;
            unsigned base = 0;
            if (gm && c == lead) base = atomicAdd(cnt + qi, (unsigned)__popc(gm));
            base = __shfl(base, g * GW + lead);
            if (pass) {
                const unsigned slot = base + (unsigned)__popc(gm & ((1u << c) - 1u));
                if (slot < ADC_CAND_CAP) cand[(int64_t)qi * ADC_CAND_CAP + slot] = adc_exact_key(s, j);
            }
        }
    }
}

// The body of dense_gemm_kernel, and of the L2 screen's kernel (dense_search_l2.hip), which is this GEMM with one more
// operand and another epilogue: L2 emits sigma = fmaf(2, dot, -xsq[row]) instead of the dot, xsq [N] = the stored squared norm
// of every corpus row (a lane holds one corpus row per column tile: two values, loaded once per block).  !L2: xsq is unused.
// MAP (subset search): the matrix searched is x[rows], rows [N] ascending corpus rows; the row that the loader reads and the
// norm of the L2 epilogue go through rows[] once per thread at block start, everything else (keys, out) keeps the logical j.
template <int MODE, bool PAD, typename T, bool L2, bool MAP = false>
__device__ __forceinline__ void dense_gemm_body(const T* __restrict__ x, int64_t ldx, int64_t N, int64_t nrows, int64_t smap,
                                                const T* __restrict__ q, int nq, int D, const float* __restrict__ thr,
                                                float* __restrict__ out, unsigned* __restrict__ cnt,
                                                unsigned long long* __restrict__ cand, const float* __restrict__ xsq,
                                                const int64_t* __restrict__ rows = nullptr) {
    __shared__ float sa[2][DENSE_TILE * DENSE_LD];     // query chunk   [128][16 (+1)]
    __shared__ float sb[2][DENSE_TILE * DENSE_LD];     // corpus chunk  [128][16 (+1)]
    __shared__ float s_thr[DENSE_TILE];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int col = l & 31, half = l >> 5;
    const int64_t j0 = (int64_t)blockIdx.x * DENSE_TILE;
    // loader mapping: thread -> (row = tid / 2, 8 consecutive k = (tid & 1) * 8)
    const int lrow = tid >> 1, lk = (tid & 1) * 8;
    const int64_t jl = (j0 + lrow < nrows) ? j0 + lrow : nrows - 1;
    const T* xp = x + dense_corpus_row<MAP>(jl, N, smap, rows) * ldx;
    const int nkc = (D + DENSE_KC - 1) / DENSE_KC;
    float nxs[2] = {0.f, 0.f};                         // L2: minus the squared norm of this lane's row of column tile b
    if constexpr (L2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + wc * 64 + b * 32 + col;
            const int64_t jc = j < nrows ? j : nrows - 1;
            nxs[b] = -xsq[dense_corpus_row<MAP>(jc, N, smap, rows)];
        }
    }
    for (int qt = 0; qt < nq; qt += DENSE_TILE) {
        const int qrow = (qt + lrow < nq) ? qt + lrow : nq - 1;
        const T* qp = q + (int64_t)qrow * D;
        if (MODE == DENSE_FILTER && tid < DENSE_TILE) s_thr[tid] = (qt + tid < nq) ? thr[qt + tid] : INFINITY;
        dense_f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        float ra[8], rb[8];
        auto gload = [&](int kc) {
            const int k0 = kc * DENSE_KC + lk;
            if constexpr (PAD) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    ra[i] = (k0 + i < D) ? (float)qp[k0 + i] : 0.f;
                    rb[i] = (k0 + i < D) ? (float)xp[k0 + i] : 0.f;
                }
            } else {
                dense_load8(qp + k0, ra);
                dense_load8(xp + k0, rb);
            }
        };
        auto sstore = [&](int buf) {
            float* da = &sa[buf][lrow * DENSE_LD + lk];
            float* db = &sb[buf][lrow * DENSE_LD + lk];
#pragma unroll
            for (int i = 0; i < 8; ++i) { da[i] = ra[i]; db[i] = rb[i]; }
        };
        // row tiles of A that hold only padding (small query sets): their MFMAs are skipped, wave-uniformly — a call with
        // <= 32 queries issues a quarter of the matrix work of a full tile and is bounded by the corpus read instead
        const bool act[2] = {qt + wr * 64 < nq, qt + wr * 64 + 32 < nq};
        gload(0);
        sstore(0);
        __syncthreads();
        for (int kc = 0; kc < nkc; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nkc) gload(kc + 1);
#pragma unroll
            for (int ks = 0; ks < DENSE_KC / 2; ++ks) {
                float fa[2], fb[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    fa[t] = sa[buf][(wr * 64 + t * 32 + col) * DENSE_LD + 2 * ks + half];   // A[i = col][k = half]
                    fb[t] = sb[buf][(wc * 64 + t * 32 + col) * DENSE_LD + 2 * ks + half];   // B[k = half][j = col]
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (act[a])
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
            if (kc + 1 < nkc) sstore(buf ^ 1);
            __syncthreads();
        }
        // epilogue: this lane's row of column tile b is j0 + wc*64 + b*32 + col; its 16 queries of row tile a are
        // qt + wr*64 + a*32 + (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + wc * 64 + b * 32 + col;
            const bool jv = j < nrows;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qo = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const int qi = qt + qo;
                    const float sc = L2 ? __builtin_fmaf(2.f, acc[a][b][r], nxs[b]) : acc[a][b][r];
                    dense_emit<MODE, 32>(sc, j, jv, qi, nq, MODE == DENSE_FILTER ? s_thr[qo] : 0.f, nrows, out, cnt, cand, l);
                }
        }
        __syncthreads();                                           // the next query tile overwrites buffer 0 and s_thr
    }
}

// grid: ceil(nrows / 128) blocks of 256 threads.  Logical row j in [0, nrows) is corpus row (smap ? j N / smap : j).
// x: [N, ldx] (16-byte aligned rows unless PAD), q: [nq, D] contiguous.  STORE: out [nq][nrows].  FILTER: thr [nq],
// cnt [nq] (zeroed), cand [nq][ADC_CAND_CAP].  MAP: rows [N], x is indexed through it (dense_gemm_body); !MAP never reads rows.
template <int MODE, bool PAD, typename T, bool MAP = false>
__global__ __launch_bounds__(256) void dense_gemm_kernel(const T* __restrict__ x, int64_t ldx, int64_t N, int64_t nrows,
                                                         int64_t smap, const T* __restrict__ q, int nq, int D,
                                                         const float* __restrict__ thr, float* __restrict__ out,
                                                         unsigned* __restrict__ cnt, unsigned long long* __restrict__ cand,
                                                         const int64_t* __restrict__ rows) {
    dense_gemm_body<MODE, PAD, T, false, MAP>(x, ldx, N, nrows, smap, q, nq, D, thr, out, cnt, cand, nullptr, rows);
}

// What a search reads beside x and q, one bundle for every variant and every hook (dense_screen.h): a variant reads the
// fields it has and ignores the rest.  xsq [N]: the rows' squared norms (L2), dec [2][D]: the decoding vectors (coded),
// rows [N]: the rows of a subset search, null for the whole store.
struct dense_operands {
    const float* xsq = nullptr;
    const float* dec = nullptr;
    const int64_t* rows = nullptr;
};

// MAP is a template argument and not `o.rows != nullptr`: a unit that never searches a subset instantiates no mapped kernel.
// The variants that serve subsets choose between the two forms (V::subset, dense_screen.h).
template <int MODE, typename T, bool MAP = false>
static int dense_launch_gemm(rc_handle_t h, const dense_operands& o, const T* x, int64_t ldx, int64_t N, int64_t nrows,
                             int64_t smap, const T* q, int nq, int D, const float* thr, float* out, unsigned* cnt,
                             unsigned long long* cand, hipStream_t s) {
    const dim3 grid((unsigned)((nrows + DENSE_TILE - 1) / DENSE_TILE));
    if (D % DENSE_KC == 0)
        hipLaunchKernelGGL((dense_gemm_kernel<MODE, false, T, MAP>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand, o.rows);
    else
        hipLaunchKernelGGL((dense_gemm_kernel<MODE, true, T, MAP>), grid, dim3(256), 0, s, x, ldx, N, nrows, smap, q, nq, D, thr,
                           out, cnt, cand, o.rows);
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

static inline bool dense_exact_route(int64_t N) { return N <= DENSE_EXACT_MAX_N; }
static inline bool dense_shape_ok(int64_t N, int D, int nq, int k) {
    return N > 0 && N <= 0xFFFFFFFFll && D > 0 && nq > 0 && k > 0 && k <= ADC_CAND_CAP / 2;
}

struct dense_exact_layout { size_t sc; topk_exact_layout sel; int qx; };      // sel.total = bytes of the whole workspace
static inline dense_exact_layout dense_exact_ws(int64_t N, int nq) {
    dense_exact_layout L;
    int64_t qx = (int64_t)(DENSE_EXACT_SC_BYTES / ((uint64_t)N * sizeof(float)));
    if (qx < 1) qx = 1;
    if (qx > DENSE_EXACT_QX_MAX) qx = DENSE_EXACT_QX_MAX;
    if (qx > nq) qx = nq;
    L.qx = (int)qx;
    L.sc = 0;
    L.sel = topk_exact_ws(rc_align_up((size_t)qx * (size_t)N * sizeof(float), 256), L.qx);
    return L;
}

struct dense_fast_layout { size_t sample, thr, cnt, cand, total; int64_t S; };
static inline dense_fast_layout dense_fast_ws(int64_t N, int nq) {
    dense_fast_layout L;
    L.S = N < ADC_SAMPLE_MAX ? N : ADC_SAMPLE_MAX;
    size_t o = 0;
    L.sample = o; o += rc_align_up((size_t)nq * (size_t)L.S * sizeof(float), 256);
    L.thr = o;    o += rc_align_up((size_t)nq * sizeof(float), 256);
    L.cnt = o;    o += rc_align_up((size_t)nq * sizeof(unsigned), 256);
    L.cand = o;   o += rc_align_up((size_t)nq * ADC_CAND_CAP * sizeof(unsigned long long), 256);
    L.total = o;
    return L;
}

// Rows of D % 16 == 0 elements are read with 16-byte loads: x, q and the row pitch must be 16-byte aligned
template <typename X, typename T>
static bool dense_aligned(const X* x, int64_t ldx, int D, const T* q) {
    return D % DENSE_KC != 0 || (ldx % (16 / (int)sizeof(X)) == 0 && !((uintptr_t)x & 15u) && !((uintptr_t)q & 15u));
}

// argument checks shared by all entries: shapes first (pure arithmetic), then pointers, then dense_aligned (aligned = false: the
// variant has a form for the rest)
template <typename X, typename T>
static int dense_check(rc_handle_t h, const X* x, int64_t ldx, int64_t N, int D, const T* q, int nq, int k,
                       const float* scores, const int64_t* ids, bool aligned = true) {
    if (N > 0xFFFFFFFFll || k > ADC_CAND_CAP / 2) return RC_ESHAPE;
    if (!h || !x || !q || !scores || !ids || N <= 0 || D <= 0 || nq < 0 || k <= 0 || ldx < D) return RC_EINVAL;
    if (aligned && !dense_aligned(x, ldx, D, q)) return RC_EINVAL;
    return RC_OK;
}

// The exact route's score rows over an fp32 corpus, out [nq][N] (the exact_rows hook of a variant): dense_launch_gemm<DENSE_STORE,
// float>, through o.rows for a subset; defined once in dense_search.hip and shared with the bf16x3 unit, which so carries no
// fp32 GEMM of its own
int dense_exact_rows_f32(rc_handle_t h, const dense_operands& o, const float* x, int64_t ldx, int64_t N, int D, const float* q,
                         int nq, float* out, hipStream_t s);
