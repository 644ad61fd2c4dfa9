// Selections of the ADC searches (rc_adc_select_rows): the codes of the rows rows[0 .. ns) of an index, compact, and their
// permuted image in one of the three image layouts — what a subset search scans in place of the index (DESIGN.md 4.6 "Subset
// search, PQ").  Included by adc_search.hip (the flat layout, the entry) and ivf_lists.hip (the IVF screens' layouts); the
// layouts themselves are described next to the images' own kernels (adc_sel_flat: adc_screen16.h, adc_sel_rows: ivfs_screen8.h,
// adc_sel_rows16: ivfs_screen16.h).
//
// The image kernels of `add` (adc_q16_image_kernel, ivfs_image_kernel, ivfs16_image_kernel) move one byte per thread: a byte
// gather and a byte scatter, fine once per corpus.  A selection is built per selector, and its source rows are M bytes apart from
// nothing in particular.  Here a block takes ADC_SEL_ROWS consecutive rows of the selection: it reads their entries of rows[]
// once, fetches every row with 16-byte loads (M % 16 == 0 for every M with an image: the rows are 16-byte aligned), stores them
// to the compact codes as they arrive — consecutive pieces are consecutive bytes there — and to LDS, and then writes the block's
// part of the image in 16-byte pieces put together from LDS bytes.  In all three layouts the image of ADC_SEL_ROWS = 128 rows
// starting at a multiple of 128 is a set of whole 16-byte pieces (flat: 2 KiB per phase, a lane's 8 chunks of a step are 32
// contiguous bytes = two pieces; rows / rows16: the 16 M contiguous bytes of each chunk of 16 rows).
//
// A layout L says where a piece goes and which code bytes it holds:
//   L::dest(M, i0, o)                byte offset in the image of piece o (0 .. 8 M - 1) of the block whose first row is i0
//   L::src(M, o, b, row, m)          byte b of that piece = codes of the block's row `row` (0 .. 127), sub-quantiser m
// A piece whose rows all exist is one 16-byte store; in the selection's last block the bytes of the rows that exist are stored
// one by one, so no byte is written that the image kernels would not write for ns rows.  No atomics, no scratch, nothing read
// on the host; rows[] (ascending, unique, inside [0, N)) is the caller's word.
#pragma once
#include "adc_common.h"

#define ADC_SEL_ROWS 128
#define ADC_SEL_THREADS 256

template <int M, typename L>
__global__ __launch_bounds__(ADC_SEL_THREADS) void adc_select_rows_kernel(const uint8_t* __restrict__ codes,
                                                                          const int64_t* __restrict__ rows, int64_t ns,
                                                                          uint8_t* __restrict__ sel_codes,
                                                                          uint8_t* __restrict__ sel_image) {
    static_assert(M % 16 == 0, "16-byte pieces");
    constexpr int PR = M / 16;                                 // pieces per row
    constexpr int PIECES = ADC_SEL_ROWS * PR;                  // per block, of the codes and of the image alike
    __shared__ int64_t s_rows[ADC_SEL_ROWS];
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[ADC_SEL_ROWS * M];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * ADC_SEL_ROWS;
    const int nv = (ns - i0) < ADC_SEL_ROWS ? (int)(ns - i0) : ADC_SEL_ROWS;       // rows of this block that exist
    if (tid < nv) s_rows[tid] = rows[i0 + tid];
    __syncthreads();
    for (int t = tid; t < nv * PR; t += ADC_SEL_THREADS) {
        const int r = t / PR, part = t % PR;
        const uint4 v = reinterpret_cast<const uint4*>(codes + s_rows[r] * M)[part];
        reinterpret_cast<uint4*>(s_codes)[t] = v;
        if (sel_codes) reinterpret_cast<uint4*>(sel_codes + i0 * M)[t] = v;
    }
    if (!sel_image) return;
    __syncthreads();
    for (int o = tid; o < PIECES; o += ADC_SEL_THREADS) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
        int top = 0;                                           // the piece's highest row
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            int row, m;
            L::src(M, o, b, row, m);
            top = row > top ? row : top;
            if (row < nv) w[b >> 2] |= (unsigned)s_codes[row * M + m] << (8 * (b & 3));
        }
        uint8_t* out = sel_image + L::dest(M, i0, o);
        if (top < nv) {
            *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                int row, m;
                L::src(M, o, b, row, m);
                if (row < nv) out[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

// one launch for the M with an image (the caller has checked M, the pointers and their alignment; ns >= 1)
template <typename L>
static int adc_select_launch(rc_handle_t h, const uint8_t* codes, int M, const int64_t* rows, int64_t ns, uint8_t* sel_codes,
                             uint8_t* sel_image, hipStream_t s) {
    const dim3 grid((unsigned)((ns + ADC_SEL_ROWS - 1) / ADC_SEL_ROWS));
    switch (M) {
#define ADC_SEL_CASE(MM)                                                                                                  \
    case MM:                                                                                                              \
        hipLaunchKernelGGL((adc_select_rows_kernel<MM, L>), grid, dim3(ADC_SEL_THREADS), 0, s, codes, rows, ns, sel_codes, \
                           sel_image);                                                                                    \
        break;
        ADC_CF_WIDTHS(ADC_SEL_CASE)
#undef ADC_SEL_CASE
    default: return RC_ESHAPE;
    }
    RC_LAUNCH_CHECK(h);
    return RC_OK;
}

// ivf_lists.hip: the same launch for the IVF screens' layouts (wide = 0: rc_adc_scan_image_rows', 1: _rows16's)
int adc_select_rows_ivf(rc_handle_t h, const uint8_t* codes, int M, const int64_t* rows, int64_t ns, int wide, uint8_t* sel_codes,
                        uint8_t* sel_image, hipStream_t s);
