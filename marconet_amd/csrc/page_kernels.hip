// The page: every restored text line of a page (long_lines.compose_lines leaves them on the device, uint8 BGR at height `rows`) brought to its
// rectangle of the enlarged page and blended into it, for all regions of the page in ONE launch (mnet_paste_u8) — and the same for the character
// cells of vertical columns (mnet_column_paste_u8: every restored character brought back to its own cell).  The definition is the host's, byte for
// byte — marconet_amd/pages.py::paste_host and marconet_amd/columns.py::paste_column_host: a k x k box average of the line (page_blend.h), the 8-bit
// INTER_CUBIC resample of that intermediate to exactly rw x rh (taps from lq_taps.h, both passes in integers, one rounding shift by 22 bits:
// page_tile.h), BGR → RGB, and the integer feather of page_blend.h against the background the page already holds.
//
// There is ONE body, stated for a column's cell in two halves — cell_foreground (the box average and the cubic gather of one pixel → three sums) and
// cell_blend (the sums → bytes, feathered into the pixel) —, which paste_cell joins for the two kernels above: a mnet_paste_region is a
// mnet_column_paste whose slice starts at column 0 and whose feather rectangle is its own (as_cell).  paste_u8_kernel passes those as facts the
// compiler sees, so the cell's extra terms fold away.
// mnet_paste_ordered_u8 (include/marconet_hip_ordered.h) calls the same two halves from a third kernel whose workgroups belong to the PAGE's tiles,
// not to descriptors: overlapping cells are composited in the caller's order, in registers, and the work follows the covered area (see the kernel).
//
// Launch shape: page_tile.h's tile over one descriptor's rectangle, counted from the rectangle's own corner; the grid is n descriptors x the tiles of
// the page (a rectangle inside the page needs no more); a workgroup whose tile lies outside its rectangle returns before it loads anything.  Each of
// the 16 taps of a pixel is the box average of k x c line bytes, rounded to a byte before it enters the cubic sum, as the two-step definition
// requires: at most 16 line reads per line pixel (k > 1) or per page pixel (k = 1).  Line and page bytes are read with byte loads (3-byte pixels at
// any offset); the pass is tiny next to the forward.
// Bounds: a descriptor is followed only if it passes paste_cell's checks (the lists: include/marconet_hip.h, include/marconet_hip_columns.h) — every
// workgroup of a descriptor takes the same decision from the same bytes; then every tap index is clamped into the box-reduced slice [rows / k] x
// [ceil(src_w / k)], whose boxes lie inside [rows] x [src_x0, src_x0 + src_w) of line line_index < n_lines, src_x0 + src_w <= line_w; every store lies
// inside the rectangle, which lies inside the page; the feather coordinates lie in [0, fw) x [0, fh) because the rectangle lies inside the feather
// rectangle.  The page is read and written at the thread's own pixel only.
#include "common.h"
#include "../../include/marconet_hip_columns.h"
#include "../../include/marconet_hip_ordered.h"
#include "page_tile.h"
#include "page_blend.h"

namespace {

__device__ __forceinline__ mnet_column_paste as_cell(const mnet_paste_region& R) {
    return {R.line_index, 0, R.src_w, R.x0, R.y0, R.rw, R.rh, R.feather, R.k, R.x0, R.y0, R.rw, R.rh, 0, R.scale_x, R.scale_y};
}

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

// mixed_kernels.hip includes this file for the body above alone (MNET_PAGE_CELL_ONLY), so that a cell's arithmetic stays stated once, here
#ifndef MNET_PAGE_CELL_ONLY

__device__ __forceinline__ void paste_cell(PtTaps& s, const PtTile T, const mnet_column_paste R, const unsigned char* __restrict__ lines, int n_lines, int rows,
                                  int line_w, unsigned char* page, int page_h, int page_w) {
    const int k = R.k, rw = R.rw, rh = R.rh;
    if (!cell_followed(R, n_lines, rows, line_w, page_h, page_w) || T.x0 >= rw || T.y0 >= rh) return;         // uniform over the workgroup
    pt_stage_taps(s, T, (R.src_w + k - 1) / k, R.scale_x, rows / k, R.scale_y, 0, 1, 0);
    const int t = (int)threadIdx.x, tx = t & (PT_TX - 1), ty = t / PT_TX;
    const int u = T.x0 + tx;
    if (u >= rw) return;
    const CellView V = cell_view(R, lines, rows, line_w);
    const unsigned fa = V.F ? page_feather_axis(V.fu0 + (unsigned)u, (unsigned)R.fw, V.F) : 0u;
    const PtI4 ci = s.ci[tx], ct = s.ct[tx];
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        const int r = ty + 4 * i, v = T.y0 + r;
        if (v >= rh) break;
        int acc[3];
        cell_foreground(V.line, V.row_bytes, k, R.src_w, ci, ct, s.ri[r], s.rt[r], acc);
        const unsigned fb = V.F ? page_feather_axis(V.fv0 + (unsigned)v, (unsigned)R.fh, V.F) : 0u;
        cell_blend(page + ((size_t)(R.y0 + v) * page_w + (size_t)(R.x0 + u)) * 3, acc, fa, fb, V.F);
    }
}

__global__ void __launch_bounds__(256) paste_u8_kernel(const unsigned char* __restrict__ lines, int n_lines, int rows, int line_w,
                                                       const mnet_paste_region* __restrict__ regions, int tiles_x, int tiles_y,
                                                       unsigned char* page, int page_h, int page_w) {
    __shared__ PtTaps s;
    const PtTile T = pt_tile(tiles_x, tiles_y);
    paste_cell(s, T, as_cell(regions[T.desc]), lines, n_lines, rows, line_w, page, page_h, page_w);
}

__global__ void __launch_bounds__(256) column_paste_u8_kernel(const unsigned char* __restrict__ lines, int n_lines, int rows, int line_w,
                                                              const mnet_column_paste* __restrict__ cells, int tiles_x, int tiles_y,
                                                              unsigned char* page, int page_h, int page_w) {
    __shared__ PtTaps s;
    const PtTile T = pt_tile(tiles_x, tiles_y);
    paste_cell(s, T, cells[T.desc], lines, n_lines, rows, line_w, page, page_h, page_w);
}

// The ordered compositor: the workgroup owns tile blockIdx.x of the PAGE (64 x 16, counted from the page's origin, row-major), keeps its pixels in
// registers, walks the cells order[first .. first + count) of its span in sequence and stores once.  The tap stage is reused per cell: one barrier
// before it is staged again (every lane has read the last cell's taps), pt_stage_taps' own after.  Every condition that skips a span or a cell is
// uniform over the workgroup, and after the first barrier no lane returns before the last: a lane outside a cell's rectangle is predicated.
// The tile's origin counted from the cell's corner may be negative or beyond the rectangle: lq_cubic_taps clamps every index for any coordinate,
// and those lanes' taps are not used.
__global__ void __launch_bounds__(256) paste_ordered_u8_kernel(const unsigned char* __restrict__ lines, int n_lines, int rows, int line_w,
                                                               const mnet_column_paste* __restrict__ cells, int n_cells,
                                                               const mnet_tile_span* __restrict__ spans, const int* __restrict__ order, int n_order,
                                                               int tiles_x, unsigned char* page, int page_h, int page_w) {
    __shared__ PtTaps s;
    const mnet_tile_span sp = spans[blockIdx.x];                               // the launcher has checked: one record per workgroup
    if (sp.count <= 0 || sp.first < 0 || (long long)sp.first + sp.count > n_order) return;      // uniform; nothing loaded, no barrier met
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * PT_TX, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * PT_TY;
    const int t = (int)threadIdx.x, tx = t & (PT_TX - 1), ty = t / PT_TX;
    const bool in_x = tx < page_w - X0;                                          // X0 + tx itself could pass 2^31 in a page's last tile
    unsigned char pix[PT_TY / 4][3] = {};
    unsigned covered = 0u;                                                       // bit i: row ty + 4 i of the tile was covered by a followed cell
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        if (in_x && ty + 4 * i < page_h - Y0) {
            const unsigned char* d = page + ((size_t)(Y0 + ty + 4 * i) * page_w + (size_t)(X0 + tx)) * 3;
            pix[i][0] = d[0]; pix[i][1] = d[1]; pix[i][2] = d[2];
        }
    }
    for (int e = 0; e < sp.count; ++e) {
        const int c = order[sp.first + e];
        if (c < 0 || c >= n_cells) continue;                                     // uniform
        const mnet_column_paste R = cells[c];
        if (!cell_followed(R, n_lines, rows, line_w, page_h, page_w)) continue;   // uniform
        // the rectangle lies inside the page (followed), so its ends fit an int; a cell that does not touch the tile is skipped
        if (R.x0 - X0 >= PT_TX || R.x0 + R.rw <= X0 || R.y0 - Y0 >= PT_TY || R.y0 + R.rh <= Y0) continue;      // uniform
        const int k = R.k;
        const PtTile T = {X0 - R.x0, Y0 - R.y0, c};
        __syncthreads();
        pt_stage_taps(s, T, (R.src_w + k - 1) / k, R.scale_x, rows / k, R.scale_y, 0, 1, 0);
        const int u = T.x0 + tx;
        if (in_x && u >= 0 && u < R.rw) {
            const CellView V = cell_view(R, lines, rows, line_w);
            const unsigned fa = V.F ? page_feather_axis(V.fu0 + (unsigned)u, (unsigned)R.fw, V.F) : 0u;
            const PtI4 ci = s.ci[tx], ct = s.ct[tx];
#pragma unroll
            for (int i = 0; i < PT_TY / 4; ++i) {
                const int r = ty + 4 * i, v = T.y0 + r;
                if (v >= 0 && v < R.rh) {
                    int acc[3];
                    cell_foreground(V.line, V.row_bytes, k, R.src_w, ci, ct, s.ri[r], s.rt[r], acc);
                    const unsigned fb = V.F ? page_feather_axis(V.fv0 + (unsigned)v, (unsigned)R.fh, V.F) : 0u;
                    cell_blend(pix[i], acc, fa, fb, V.F);
                    covered |= 1u << i;
                }
            }
        }
    }
    // a covered pixel lies inside a followed cell's rectangle, which lies inside the page
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        if (covered & (1u << i)) {
            unsigned char* d = page + ((size_t)(Y0 + ty + 4 * i) * page_w + (size_t)(X0 + tx)) * 3;
            d[0] = pix[i][0]; d[1] = pix[i][1]; d[2] = pix[i][2];
        }
    }
}

// the launcher of the two per-descriptor kernels: `who` is the entry point's name, `what` its word for a descriptor
template <typename Desc>
int paste_launch(void (*kernel)(const unsigned char*, int, int, int, const Desc*, int, int, unsigned char*, int, int), const char* who, const char* what,
                 const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const Desc* table, int32_t n, uint8_t* page, int32_t page_h,
                 int32_t page_w, void* stream) {
    MNET_CHECK_ARG(lines && table && page, "%s: null pointer", who);
    MNET_CHECK_ARG(n_lines >= 1 && rows >= 1 && line_w >= 1 && n >= 1 && page_h >= 1 && page_w >= 1,
                   "%s: bad shape (n_lines=%d, rows=%d, line_w=%d, n_%s=%d, page_h=%d, page_w=%d)", who, n_lines, rows, line_w, what, n, page_h, page_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(table) & 7) == 0, "%s: %s must be 8-byte aligned", who, what);
    const PtGrid g = pt_grid(n, page_w, page_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "%s: page too large (%lld tiles)", who, g.blocks);
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), lines, n_lines, rows, line_w, table,
                       (int)g.tiles_x, (int)g.tiles_y, page, page_h, page_w);
    MNET_LAUNCH_CHECK(who);
    return MNET_OK;
}

int ordered_launch(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                   const mnet_tile_span* spans, int32_t n_spans, const int32_t* order, int32_t n_order, uint8_t* page, int32_t page_h, int32_t page_w,
                   void* stream) {
    const char* who = "paste_ordered_u8";
    MNET_CHECK_ARG(lines && cells && spans && order && page, "%s: null pointer", who);
    MNET_CHECK_ARG(n_lines >= 1 && rows >= 1 && line_w >= 1 && n_cells >= 1 && n_order >= 1 && page_h >= 1 && page_w >= 1,
                   "%s: bad shape (n_lines=%d, rows=%d, line_w=%d, n_cells=%d, n_order=%d, page_h=%d, page_w=%d)", who, n_lines, rows, line_w, n_cells,
                   n_order, page_h, page_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(cells) & 7) == 0, "%s: cells must be 8-byte aligned", who);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(spans) & 3) == 0 && (reinterpret_cast<uintptr_t>(order) & 3) == 0,
                     "%s: spans and order must be 4-byte aligned", who);
    const PtGrid g = pt_grid(1, page_w, page_h);                                 // one workgroup per tile of the page
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "%s: page too large (%lld tiles)", who, g.blocks);
    // a launch of more than 2^32 - 1 threads runs only a part of its workgroups here, without an error: refuse it (2^24 tiles are 17 gigapixels)
    MNET_CHECK_ARG(g.blocks * 256 <= 0xffffffffll, "%s: page too large (%lld tiles of 256 threads are 2^32 threads or more)", who, g.blocks);
    MNET_CHECK_ARG((long long)n_spans == g.blocks, "%s: %d spans for a page of %lld tiles (%d x %d)", who, n_spans, g.blocks, page_w, page_h);
    hipLaunchKernelGGL(paste_ordered_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), lines, n_lines, rows,
                       line_w, cells, n_cells, spans, order, n_order, (int)g.tiles_x, page, page_h, page_w);
    MNET_LAUNCH_CHECK(who);
    return MNET_OK;
}

#endif  // MNET_PAGE_CELL_ONLY

}  // namespace

#ifndef MNET_PAGE_CELL_ONLY

extern "C" int mnet_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_paste_region* regions, int32_t n_regions,
                             uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    return paste_launch(paste_u8_kernel, "paste_u8", "regions", lines, n_lines, rows, line_w, regions, n_regions, page, page_h, page_w, stream);
}

extern "C" int mnet_column_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                                    uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    return paste_launch(column_paste_u8_kernel, "column_paste_u8", "cells", lines, n_lines, rows, line_w, cells, n_cells, page, page_h, page_w, stream);
}

extern "C" int mnet_paste_ordered_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                                     const mnet_tile_span* spans, int32_t n_spans, const int32_t* order, int32_t n_order, uint8_t* page, int32_t page_h,
                                     int32_t page_w, void* stream) {
    return ordered_launch(lines, n_lines, rows, line_w, cells, n_cells, spans, n_spans, order, n_order, page, page_h, page_w, stream);
}

#endif  // MNET_PAGE_CELL_ONLY
