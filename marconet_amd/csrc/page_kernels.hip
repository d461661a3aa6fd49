// The page: every restored text line of a page (long_lines.compose_lines leaves them on the device, uint8 BGR at height `rows`) brought to its
// rectangle of the enlarged page and blended into it, for all regions of the page in ONE launch (mnet_paste_u8) — and the same for the character
// cells of vertical columns (mnet_column_paste_u8: every restored character brought back to its own cell).  The definition is the host's, byte for
// byte — marconet_amd/pages.py::paste_host and marconet_amd/columns.py::paste_column_host: a k x k box average of the line (page_blend.h), the 8-bit
// INTER_CUBIC resample of that intermediate to exactly rw x rh (taps from lq_taps.h, both passes in integers, one rounding shift by 22 bits:
// page_tile.h), BGR → RGB, and the integer feather of page_blend.h against the background the page already holds.
//
// There is ONE body, stated for a column's cell in two halves (cell_paste.h: cell_foreground and cell_blend), which paste_cell joins for the two
// kernels above: a mnet_paste_region is a mnet_column_paste whose slice starts at column 0 and whose feather rectangle is its own (as_cell).
// paste_u8_kernel passes those as facts the compiler sees, so the cell's extra terms fold away.  The page-tile compositor (mixed_kernels.hip) calls
// the same two halves for cells it composites in the caller's order, in registers.
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
#include "page_tile.h"
#include "page_blend.h"
#include "cell_paste.h"

namespace {

__device__ __forceinline__ mnet_column_paste as_cell(const mnet_paste_region& R) {
    return {R.line_index, 0, R.src_w, R.x0, R.y0, R.rw, R.rh, R.feather, R.k, R.x0, R.y0, R.rw, R.rh, 0, R.scale_x, R.scale_y};
}

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

}  // namespace

extern "C" int mnet_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_paste_region* regions, int32_t n_regions,
                             uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    return paste_launch(paste_u8_kernel, "paste_u8", "regions", lines, n_lines, rows, line_w, regions, n_regions, page, page_h, page_w, stream);
}

extern "C" int mnet_column_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                                    uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    return paste_launch(column_paste_u8_kernel, "column_paste_u8", "cells", lines, n_lines, rows, line_w, cells, n_cells, page, page_h, page_w, stream);
}
