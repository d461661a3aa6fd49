// Vertical text columns of a page, made of upright stacked characters: the gather in (mnet_column_gather_u8: every character cell of every window of
// every column resized on its own and laid side by side as the horizontal strip mnet_lq_from_u8 reads) and the scatter out (mnet_column_paste_u8: every
// restored character brought back to its own cell of the enlarged page), each for all columns of the page in ONE launch.  The definition is the host's,
// byte for byte: marconet_amd/columns.py's virtual_strip / paste_column_host.  The arithmetic is the siblings': the 8-bit INTER_CUBIC resample with the
// taps of lq_taps.h, both passes in integers, one rounding shift by 22 bits (lq_kernels.hip's int32 bound), and for the paste page_kernels.hip's box
// average, channel flip and integer feather (page_blend.h) — the feather taken relative to the whole column's rectangle, not the cell's.
//
// Launch shape (as lq_from_u8_kernel / paste_u8_kernel): one thread per output pixel, x fastest; a workgroup takes a 64-column x 16-row tile of one
// descriptor's output, counted from the cell's own corner, and computes the tile's 64 column taps and 16 row taps once into LDS.  The launcher does not see
// the device table, so the grid is n descriptors x the tiles of max_dw x dst_h (gather) or of the page (paste); a workgroup whose tile lies outside its
// cell returns before it loads anything.  Bytes are read and written with byte loads and stores (3-byte pixels at any offset).
// Bounds: a descriptor is followed only if it passes the checks below (the list: include/marconet_hip_columns.h) — every workgroup of a descriptor takes
// the same decision from the same bytes.  Gather: every tap index is clamped into [0, sh) x [0, sw) and shifted by (sy, sx), inside the page; every store
// lies in columns [dx, dx + dw) of rows [0, dst_h) of the window's image, which lies inside [0, dst_bytes).  Paste: every tap index is clamped into the
// box-reduced slice, whose boxes lie inside [rows] x [src_x0, src_x0 + src_w) of line line_index < n_lines, src_x0 + src_w <= line_w; every store lies
// inside the cell's rectangle, which lies inside the page; the feather coordinates lie in [0, fw) x [0, fh) because the cell lies inside the feather
// rectangle.
#include "common.h"
#include "../../include/marconet_hip_columns.h"
#include "lq_taps.h"
#include "page_blend.h"

namespace {

constexpr int CL_TX = 64, CL_TY = 16;      // tile: 64 columns x 16 rows, 256 threads x 4 rows each

struct alignas(16) ClI4 { int v[4]; };

__global__ void __launch_bounds__(256) column_gather_u8_kernel(const unsigned char* __restrict__ page, int page_h, int page_w,
                                                               const mnet_column_cell* __restrict__ cells, int tiles_x, int tiles_y, int max_dw, int dst_h,
                                                               unsigned char* __restrict__ dst, long long dst_bytes) {
    __shared__ ClI4 s_ci[CL_TX], s_ct[CL_TX], s_ri[CL_TY], s_rt[CL_TY];
    const int bid = (int)blockIdx.x;
    const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y;
    const mnet_column_cell C = cells[bid / (tiles_x * tiles_y)];
    const int dw = C.dw, sw = C.sw, sh = C.sh, win_w = C.win_w;
    const bool ok = sw >= 1 && sh >= 1 && C.sx >= 0 && C.sy >= 0 && (long long)C.sx + sw <= page_w && (long long)C.sy + sh <= page_h && dw >= 1 &&
                    dw <= max_dw && C.dx >= 0 && (long long)C.dx + dw <= win_w && C.offset >= 0 && C.offset <= dst_bytes &&
                    (long long)win_w * dst_h <= (dst_bytes - C.offset) / 3 && isfinite(C.scale_x) && isfinite(C.scale_y);
    const int u0 = tile_x * CL_TX, v0 = tile_y * CL_TY;
    if (!ok || u0 >= dw || v0 >= dst_h) return;          // uniform over the workgroup
    const int t = (int)threadIdx.x, tx = t & (CL_TX - 1), ty = t / CL_TX;
    if (t < CL_TX) {
        const LqTaps c = lq_cubic_taps(u0 + t, sw, C.scale_x);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s_ci[t].v[j] = (C.sx + c.idx[j]) * 3; s_ct[t].v[j] = c.tap[j]; }
    } else if (t < CL_TX + CL_TY) {
        const int r = t - CL_TX;
        const LqTaps c = lq_cubic_taps(v0 + r, sh, C.scale_y);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s_ri[r].v[j] = C.sy + c.idx[j]; s_rt[r].v[j] = c.tap[j]; }
    }
    __syncthreads();
    const int u = u0 + tx;
    if (u >= dw) return;
    const size_t row_bytes = (size_t)page_w * 3;
    unsigned char* out = dst + C.offset;
    const ClI4 ci = s_ci[tx], ct = s_ct[tx];
#pragma unroll
    for (int i = 0; i < CL_TY / 4; ++i) {
        const int r = ty + 4 * i, v = v0 + r;
        if (v >= dst_h) break;
        const ClI4 ri = s_ri[r], rt = s_rt[r];
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned char* row = page + (size_t)ri.v[j] * row_bytes;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int hor = (int)row[(size_t)ci.v[0] + c] * ct.v[0] + (int)row[(size_t)ci.v[1] + c] * ct.v[1] + (int)row[(size_t)ci.v[2] + c] * ct.v[2] +
                                (int)row[(size_t)ci.v[3] + c] * ct.v[3];
                acc[c] += hor * rt.v[j];
            }
        }
        unsigned char* d = out + ((size_t)v * win_w + (size_t)(C.dx + u)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (unsigned char)min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
    }
}

__global__ void __launch_bounds__(256) column_paste_u8_kernel(const unsigned char* __restrict__ lines, int n_lines, int rows, int line_w,
                                                              const mnet_column_paste* __restrict__ cells, int tiles_x, int tiles_y,
                                                              unsigned char* page, int page_h, int page_w) {
    __shared__ ClI4 s_ci[CL_TX], s_ct[CL_TX], s_ri[CL_TY], s_rt[CL_TY];
    const int bid = (int)blockIdx.x;
    const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y;
    const mnet_column_paste R = cells[bid / (tiles_x * tiles_y)];
    const int k = R.k, rw = R.rw, rh = R.rh;
    const bool ok = R.line_index >= 0 && R.line_index < n_lines && R.src_x0 >= 0 && R.src_w >= 1 && (long long)R.src_x0 + R.src_w <= line_w && rw >= 1 &&
                    rh >= 1 && R.x0 >= 0 && R.y0 >= 0 && (long long)R.x0 + rw <= page_w && (long long)R.y0 + rh <= page_h && R.feather >= 0 &&
                    R.feather <= PAGE_MAX_FEATHER && (k == 1 || k == 2 || k == 4 || k == 8) && rows % k == 0 && R.fw >= 1 && R.fh >= 1 && R.fx0 <= R.x0 &&
                    R.fy0 <= R.y0 && (long long)R.x0 + rw <= (long long)R.fx0 + R.fw && (long long)R.y0 + rh <= (long long)R.fy0 + R.fh;
    const int u0 = tile_x * CL_TX, v0 = tile_y * CL_TY;
    if (!ok || u0 >= rw || v0 >= rh) return;             // uniform over the workgroup
    const int src_w = R.src_w, nx = (src_w + k - 1) / k, ny = rows / k;
    const int t = (int)threadIdx.x, tx = t & (CL_TX - 1), ty = t / CL_TX;
    if (t < CL_TX) {
        const LqTaps c = lq_cubic_taps(u0 + t, nx, R.scale_x);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s_ci[t].v[j] = c.idx[j]; s_ct[t].v[j] = c.tap[j]; }
    } else if (t < CL_TX + CL_TY) {
        const int r = t - CL_TX;
        const LqTaps c = lq_cubic_taps(v0 + r, ny, R.scale_y);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s_ri[r].v[j] = c.idx[j]; s_rt[r].v[j] = c.tap[j]; }
    }
    __syncthreads();
    const int u = u0 + tx;
    if (u >= rw) return;
    const unsigned F = (unsigned)R.feather;
    // the feather's coordinates are the column's: 0 <= x0 - fx0 + u < fw, 0 <= y0 - fy0 + v < fh (the cell lies inside the feather rectangle)
    const unsigned fu0 = (unsigned)((long long)R.x0 - R.fx0), fv0 = (unsigned)((long long)R.y0 - R.fy0);
    const unsigned fa = F ? page_feather_axis(fu0 + (unsigned)u, (unsigned)R.fw, F) : 0u;
    const size_t row_bytes = (size_t)line_w * 3;
    const unsigned char* line = lines + (size_t)R.line_index * rows * row_bytes + (size_t)R.src_x0 * 3;      // the slice's first column
    const ClI4 ci = s_ci[tx], ct = s_ct[tx];
#pragma unroll
    for (int i = 0; i < CL_TY / 4; ++i) {
        const int r = ty + 4 * i, v = v0 + r;
        if (v >= rh) break;
        const ClI4 ri = s_ri[r], rt = s_rt[r];
        int acc[3] = {0, 0, 0};
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
        unsigned char* d = page + ((size_t)(R.y0 + v) * page_w + (size_t)(R.x0 + u)) * 3;
        const unsigned fb = F ? page_feather_axis(fv0 + (unsigned)v, (unsigned)R.fh, F) : 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned fg = (unsigned)min(max((acc[2 - ch] + (1 << 21)) >> 22, 0), 255);       // the line is BGR, the page RGB
            d[ch] = (unsigned char)(F ? page_feather(d[ch], fg, fa, fb, F) : fg);
        }
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
    const long long tiles_x = ((long long)max_dw + CL_TX - 1) / CL_TX, tiles_y = ((long long)dst_h + CL_TY - 1) / CL_TY;
    MNET_CHECK_ARG(tiles_x * tiles_y <= 0x7fffffffll && (long long)n_cells * tiles_x * tiles_y <= 0x7fffffffll,
                   "column_gather_u8: batch too large (%d cells of %lld x %lld tiles)", n_cells, tiles_x, tiles_y);
    const long long grid = (long long)n_cells * tiles_x * tiles_y;
    hipLaunchKernelGGL(column_gather_u8_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), page, page_h, page_w, cells,
                       (int)tiles_x, (int)tiles_y, max_dw, dst_h, dst, (long long)dst_bytes);
    MNET_LAUNCH_CHECK("column_gather_u8");
    return MNET_OK;
}

extern "C" int mnet_column_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                                    uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    MNET_CHECK_ARG(lines && cells && page, "column_paste_u8: null pointer");
    MNET_CHECK_ARG(n_lines >= 1 && rows >= 1 && line_w >= 1 && n_cells >= 1 && page_h >= 1 && page_w >= 1,
                   "column_paste_u8: bad shape (n_lines=%d, rows=%d, line_w=%d, n_cells=%d, page_h=%d, page_w=%d)", n_lines, rows, line_w, n_cells, page_h, page_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(cells) & 7) == 0, "column_paste_u8: cells must be 8-byte aligned");
    const int tiles_x = (page_w + CL_TX - 1) / CL_TX, tiles_y = (page_h + CL_TY - 1) / CL_TY;
    const long long grid = (long long)n_cells * tiles_x * tiles_y;
    MNET_CHECK_ARG(grid <= 0x7fffffffll, "column_paste_u8: page too large (%lld tiles)", grid);
    hipLaunchKernelGGL(column_paste_u8_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), lines, n_lines, rows, line_w, cells,
                       tiles_x, tiles_y, page, page_h, page_w);
    MNET_LAUNCH_CHECK("column_paste_u8");
    return MNET_OK;
}
