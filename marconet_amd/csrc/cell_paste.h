// The paste of ONE page pixel of a cell — a column's character cell, or a text line's whole rectangle as a cell (page_kernels.hip's as_cell) — and the
// list a cell's descriptor must pass to be followed, stated once for the per-descriptor kernels (page_kernels.hip's paste_cell: the destination is
// the page's pixel in memory) and for the page-tile compositor (mixed_kernels.hip: the destination is the pixel in registers).  The body comes in two
// halves: cell_foreground (the box average and the cubic gather of one pixel → three sums) and cell_blend (the sums → bytes, feathered into the
// pixel).  The arithmetic is page_blend.h's and page_tile.h's, unchanged; every translation unit that includes this header is compiled with
// -ffp-contract=off (build.sh), as lq_taps.h requires of the taps the caller stages.
// Bounds: with a followed cell (cell_followed) and taps staged by pt_stage_taps for its box-reduced slice [rows / k] x [ceil(src_w / k)], every tap
// index is clamped into that slice, whose boxes lie inside [rows] x [src_x0, src_x0 + src_w) of line line_index < n_lines, src_x0 + src_w <= line_w;
// the feather coordinates lie in [0, fw) x [0, fh) because the rectangle lies inside the feather rectangle; d is the caller's, one pixel of three
// bytes, read and written by the calling thread only.
#pragma once
#include "../../include/marconet_hip_columns.h"
#include "page_tile.h"
#include "page_blend.h"

// a cell is followed only if it passes this list (include/marconet_hip.h, include/marconet_hip_columns.h); every thread decides from the same bytes
__device__ __forceinline__ bool cell_followed(const mnet_column_paste& R, int n_lines, int rows, int line_w, int page_h, int page_w) {
    const int k = R.k, rw = R.rw, rh = R.rh;
    return R.line_index >= 0 && R.line_index < n_lines && R.src_x0 >= 0 && R.src_w >= 1 && (long long)R.src_x0 + R.src_w <= line_w && rw >= 1 &&
           rh >= 1 && R.x0 >= 0 && R.y0 >= 0 && (long long)R.x0 + rw <= page_w && (long long)R.y0 + rh <= page_h && R.feather >= 0 &&
           R.feather <= PAGE_MAX_FEATHER && (k == 1 || k == 2 || k == 4 || k == 8) && rows % k == 0 && R.fw >= 1 && R.fh >= 1 && R.fx0 <= R.x0 &&
           R.fy0 <= R.y0 && (long long)R.x0 + rw <= (long long)R.fx0 + R.fw && (long long)R.y0 + rh <= (long long)R.fy0 + R.fh;
}

// The paste body, first half: the foreground of one pixel of a cell as the cubic's three sums (BGR, before pt_round_clip).  `line`: the first
// column of the cell's slice of its line, src_w columns wide and row_bytes apart; (ci, ct) / (ri, rt): the pixel's column and row taps over the
// box-reduced slice.  Each of the 16 taps is the box average of k x c line bytes, rounded to a byte before it enters the cubic sum.
__device__ __forceinline__ void cell_foreground(const unsigned char* line, size_t row_bytes, int k, int src_w, const PtI4& ci, const PtI4& ct, const PtI4& ri,
                                                const PtI4& rt, int acc[3]) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned char* top = line + (size_t)(ri.v[j] * k) * row_bytes;
        int hor[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int xs = ci.v[a] * k, c = min(k, src_w - xs);          // the box's columns [xs, xs + c) of the slice: 1 <= c <= k
            unsigned sum[3] = {0u, 0u, 0u};
            for (int dy = 0; dy < k; ++dy) {
                const unsigned char* p = top + (size_t)dy * row_bytes + (size_t)xs * 3;
                for (int dx = 0; dx < c; ++dx, p += 3) { sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2]; }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) hor[ch] += (int)page_box_avg(sum[ch], (unsigned)(k * c)) * ct.v[a];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += hor[ch] * rt.v[j];
    }
}

// ... second half: the three sums → bytes, blended into the pixel d (RGB; in memory or in registers) under the feather weights (fa, fb)
__device__ __forceinline__ void cell_blend(unsigned char* d, const int acc[3], unsigned fa, unsigned fb, unsigned F) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned fg = (unsigned)pt_round_clip(acc[2 - ch]);       // the line is BGR, the page RGB
        d[ch] = (unsigned char)(F ? page_feather(d[ch], fg, fa, fb, F) : fg);
    }
}

// what a thread needs of a followed cell beside its taps: the slice, and the feather's origin.  The feather's coordinates are the feather
// rectangle's: 0 <= x0 - fx0 + u < fw, 0 <= y0 - fy0 + v < fh (the rectangle lies inside it)
struct CellView { const unsigned char* line; size_t row_bytes; unsigned F, fu0, fv0; };

__device__ __forceinline__ CellView cell_view(const mnet_column_paste& R, const unsigned char* __restrict__ lines, int rows, int line_w) {
    const size_t row_bytes = (size_t)line_w * 3;
    return {lines + (size_t)R.line_index * rows * row_bytes + (size_t)R.src_x0 * 3, row_bytes, (unsigned)R.feather, (unsigned)((long long)R.x0 - R.fx0),
            (unsigned)((long long)R.y0 - R.fy0)};
}
