// Vertical text columns of a page, made of upright stacked characters: the gather in (mnet_column_gather_u8: every character cell of every window of
// every column resized on its own and laid side by side as the horizontal strip mnet_lq_from_u8 reads), for all columns of the page in ONE launch.  The
// definition is the host's, byte for byte: marconet_amd/columns.py's virtual_strip.  The arithmetic is lq_from_u8_kernel's: the 8-bit INTER_CUBIC
// resample with the taps of lq_taps.h, both passes in integers, one rounding shift by 22 bits (page_tile.h).  The scatter out, mnet_column_paste_u8,
// stands beside its twin in page_kernels.hip; a cell's per-pixel body is cell_paste.h's.
//
// Launch shape: page_tile.h's tile over one cell's output, counted from the cell's own corner; the grid is n cells x the tiles of max_dw x dst_h; a
// workgroup whose tile lies outside its cell returns before it loads anything.  Bytes are read and written with byte loads and stores (3-byte pixels
// at any offset).
// Bounds: a descriptor is followed only if it passes the checks below (the list: include/marconet_hip_columns.h) — every workgroup of a descriptor takes
// the same decision from the same bytes.  Every tap index is clamped into [0, sh) x [0, sw) and shifted by (sy, sx), inside the page; every store lies in
// columns [dx, dx + dw) of rows [0, dst_h) of the window's image, which lies inside [0, dst_bytes).
#include "common.h"
#include "../../include/marconet_hip_columns.h"
#include "page_tile.h"

namespace {

__global__ void __launch_bounds__(256) column_gather_u8_kernel(const unsigned char* __restrict__ page, int page_h, int page_w,
                                                               const mnet_column_cell* __restrict__ cells, int tiles_x, int tiles_y, int max_dw, int dst_h,
                                                               unsigned char* __restrict__ dst, long long dst_bytes) {
    __shared__ PtTaps s;
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const mnet_column_cell C = cells[T.desc];
    const int dw = C.dw, sw = C.sw, sh = C.sh, win_w = C.win_w;
    const bool ok = sw >= 1 && sh >= 1 && C.sx >= 0 && C.sy >= 0 && (long long)C.sx + sw <= page_w && (long long)C.sy + sh <= page_h && dw >= 1 &&
                    dw <= max_dw && C.dx >= 0 && (long long)C.dx + dw <= win_w && C.offset >= 0 && C.offset <= dst_bytes &&
                    (long long)win_w * dst_h <= (dst_bytes - C.offset) / 3 && isfinite(C.scale_x) && isfinite(C.scale_y);
    if (!ok || T.x0 >= dw || T.y0 >= dst_h) return;      // uniform over the workgroup
    pt_stage_taps(s, T, sw, C.scale_x, sh, C.scale_y, C.sx, 3, C.sy);
    const int t = (int)threadIdx.x, tx = t & (PT_TX - 1), ty = t / PT_TX;
    const int u = T.x0 + tx;
    if (u >= dw) return;
    const size_t row_bytes = (size_t)page_w * 3;
    unsigned char* out = dst + C.offset;
    const PtI4 ci = s.ci[tx], ct = s.ct[tx];
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        const int r = ty + 4 * i, v = T.y0 + r;
        if (v >= dst_h) break;
        const PtI4 ri = s.ri[r], rt = s.rt[r];
        int acc[3];
        pt_cubic_rgb(page, row_bytes, ci, ct, ri, rt, acc);
        unsigned char* d = out + ((size_t)v * win_w + (size_t)(C.dx + u)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (unsigned char)pt_round_clip(acc[c]);
    }
}

}  // namespace

extern "C" int mnet_column_gather_u8(const uint8_t* page, int32_t page_h, int32_t page_w, const mnet_column_cell* cells, int32_t n_cells, int32_t max_dw,
                                     int32_t dst_h, uint8_t* dst, int64_t dst_bytes, void* stream) {
    MNET_CHECK_ARG(page && cells && dst, "column_gather_u8: null pointer");
    MNET_CHECK_ARG(page_h >= 1 && page_w >= 1 && n_cells >= 1 && max_dw >= 1 && dst_h >= 1 && dst_bytes >= 1,
                   "column_gather_u8: bad shape (page_h=%d, page_w=%d, n_cells=%d, max_dw=%d, dst_h=%d, dst_bytes=%lld)", page_h, page_w, n_cells, max_dw, dst_h,
                   (long long)dst_bytes);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(cells) & 7) == 0, "column_gather_u8: cells must be 8-byte aligned");
    const PtGrid g = pt_grid(n_cells, max_dw, dst_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "column_gather_u8: batch too large (%d cells of %lld x %lld tiles)", n_cells, g.tiles_x, g.tiles_y);
    hipLaunchKernelGGL(column_gather_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), page, page_h, page_w, cells,
                       (int)g.tiles_x, (int)g.tiles_y, max_dw, dst_h, dst, (long long)dst_bytes);
    MNET_LAUNCH_CHECK("column_gather_u8");
    return MNET_OK;
}
