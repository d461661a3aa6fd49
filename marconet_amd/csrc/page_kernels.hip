// The page: every restored text line of a page (long_lines.compose_lines leaves them on the device, uint8 BGR at height `rows`) brought to its
// rectangle of the enlarged page and blended into it, for all regions of the page in ONE launch.  The definition is the host's:
// marconet_amd/pages.py::paste_host, byte for byte — a k x k box average of the line (page_blend.h), the 8-bit INTER_CUBIC resample of that
// intermediate to exactly rw x rh (taps from lq_taps.h, both passes in integers, one rounding shift by 22 bits: lq_kernels.hip's arithmetic and
// its int32 bound), BGR → RGB, and the integer feather of page_blend.h against the background the page already holds.
//
// Launch shape (as lq_from_u8_kernel): one thread per output pixel, x fastest; a workgroup takes a 64-column x 16-row tile of one region's
// rectangle, counted from the rectangle's own corner, and computes the tile's 64 column taps and 16 row taps once into LDS.  The launcher does not
// see the device table, so the grid is n_regions x the tiles of the page (a rectangle inside the page needs no more); a workgroup whose tile lies
// outside its region's rectangle returns before it loads anything.  Each of the 16 taps of a pixel is the box average of k x c line bytes,
// rounded to a byte before it enters the cubic sum, as the two-step definition requires: at most 16 line reads per line pixel (k > 1) or per page
// pixel (k = 1).  Line and page bytes are read with byte loads (3-byte pixels at any offset); the pass is tiny next to the forward.
// Bounds: a region is followed only if line_index, src_w, the rectangle, feather and k pass the checks below (the list: include/marconet_hip.h) —
// every workgroup of the region takes the same decision from the same descriptor; then every tap index is clamped into the intermediate
// [rows / k] x [ceil(src_w / k)], whose boxes lie inside [rows] x [src_w <= line_w] of line line_index < n_lines, and every store lies inside the
// rectangle, which lies inside the page.  The page is read and written at the thread's own pixel only.
#include "common.h"
#include "lq_taps.h"
#include "page_blend.h"

namespace {

constexpr int PG_TX = 64, PG_TY = 16;      // tile: 64 columns x 16 rows, 256 threads x 4 rows each

struct alignas(16) PgI4 { int v[4]; };

__global__ void __launch_bounds__(256) paste_u8_kernel(const unsigned char* __restrict__ lines, int n_lines, int rows, int line_w,
                                                       const mnet_paste_region* __restrict__ regions, int tiles_x, int tiles_y,
                                                       unsigned char* page, int page_h, int page_w) {
    __shared__ PgI4 s_ci[PG_TX], s_ct[PG_TX], s_ri[PG_TY], s_rt[PG_TY];
    const int bid = (int)blockIdx.x;
    const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y;
    const mnet_paste_region R = regions[bid / (tiles_x * tiles_y)];
    const int k = R.k, rw = R.rw, rh = R.rh;
    const bool ok = R.line_index >= 0 && R.line_index < n_lines && R.src_w >= 1 && R.src_w <= line_w && rw >= 1 && rh >= 1 && R.x0 >= 0 && R.y0 >= 0 &&
                    (long long)R.x0 + rw <= page_w && (long long)R.y0 + rh <= page_h && R.feather >= 0 && R.feather <= PAGE_MAX_FEATHER &&
                    (k == 1 || k == 2 || k == 4 || k == 8) && rows % k == 0;
    const int u0 = tile_x * PG_TX, v0 = tile_y * PG_TY;
    if (!ok || u0 >= rw || v0 >= rh) return;             // uniform over the workgroup
    const int src_w = R.src_w, nx = (src_w + k - 1) / k, ny = rows / k;
    const int t = (int)threadIdx.x, tx = t & (PG_TX - 1), ty = t / PG_TX;
    if (t < PG_TX) {
        const LqTaps c = lq_cubic_taps(u0 + t, nx, R.scale_x);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s_ci[t].v[j] = c.idx[j]; s_ct[t].v[j] = c.tap[j]; }
    } else if (t < PG_TX + PG_TY) {
        const int r = t - PG_TX;
        const LqTaps c = lq_cubic_taps(v0 + r, ny, R.scale_y);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s_ri[r].v[j] = c.idx[j]; s_rt[r].v[j] = c.tap[j]; }
    }
    __syncthreads();
    const int u = u0 + tx;
    if (u >= rw) return;
    const unsigned F = (unsigned)R.feather;
    const unsigned fa = F ? page_feather_axis((unsigned)u, (unsigned)rw, F) : 0u;
    const size_t row_bytes = (size_t)line_w * 3;
    const unsigned char* line = lines + (size_t)R.line_index * rows * row_bytes;
    const PgI4 ci = s_ci[tx], ct = s_ct[tx];
#pragma unroll
    for (int i = 0; i < PG_TY / 4; ++i) {
        const int r = ty + 4 * i, v = v0 + r;
        if (v >= rh) break;
        const PgI4 ri = s_ri[r], rt = s_rt[r];
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned char* top = line + (size_t)(ri.v[j] * k) * row_bytes;
            int hor[3] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int xs = ci.v[a] * k, c = min(k, src_w - xs);          // the box's columns [xs, xs + c): 1 <= c <= k
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
        const unsigned fb = F ? page_feather_axis((unsigned)v, (unsigned)rh, F) : 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned fg = (unsigned)min(max((acc[2 - ch] + (1 << 21)) >> 22, 0), 255);       // the line is BGR, the page RGB
            d[ch] = (unsigned char)(F ? page_feather(d[ch], fg, fa, fb, F) : fg);
        }
    }
}

}  // namespace

extern "C" int mnet_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_paste_region* regions, int32_t n_regions,
                             uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    MNET_CHECK_ARG(lines && regions && page, "paste_u8: null pointer");
    MNET_CHECK_ARG(n_lines >= 1 && rows >= 1 && line_w >= 1 && n_regions >= 1 && page_h >= 1 && page_w >= 1,
                   "paste_u8: bad shape (n_lines=%d, rows=%d, line_w=%d, n_regions=%d, page_h=%d, page_w=%d)", n_lines, rows, line_w, n_regions, page_h, page_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(regions) & 7) == 0, "paste_u8: regions must be 8-byte aligned");
    const int tiles_x = (page_w + PG_TX - 1) / PG_TX, tiles_y = (page_h + PG_TY - 1) / PG_TY;
    const long long grid = (long long)n_regions * tiles_x * tiles_y;
    MNET_CHECK_ARG(grid <= 0x7fffffffll, "paste_u8: page too large (%lld tiles)", grid);
    hipLaunchKernelGGL(paste_u8_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), lines, n_lines, rows, line_w, regions,
                       tiles_x, tiles_y, page, page_h, page_w);
    MNET_LAUNCH_CHECK("paste_u8");
    return MNET_OK;
}
