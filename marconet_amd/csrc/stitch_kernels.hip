// Long text lines: the restored windows of a line (marconet_amd/long_lines.py::plan_windows cuts a line wider than the reference's 512-px limit
// into overlapping windows; each is restored as a strip of its own) joined into one image, for every line of a batch in ONE launch.  The
// definition is the host's: long_lines.stitch_host, byte for byte — a column that lies in one window is that window's byte, a column in two is
// the integer cross-fade of stitch_blend.h.  sr is the uint8 BGR result the SR net's post-processing leaves on the device; dst keeps its order.
//
// Launch shape (as panel_u8_kernel): one thread per output pixel, x fastest; a workgroup takes a 64-column x 16-row tile of one line and
// resolves what depends on the column alone once into LDS: which window or window pair covers it, where the column lies in each, and the
// overlap's (t, D).  The per-pixel path is then two byte loads per channel, the header's blend and one store.  A tile wholly at columns >= the
// line's width loads nothing from sr and writes 0.  The pass is tiny and HBM-side: each output byte is read at most twice and written once.
// Bounds: every store is bounded by (rows, out_w); a column is read from window w only where 0 <= x - offset < show_w <= sr_w and
// 0 <= sr_index < n_sr.  The scan walks the line's windows [win0, win0 + n_win) once per workgroup — the lines' descriptors are the caller's
// statement of what lies inside `windows`; a line whose descriptors cannot be followed (the list: include/marconet_hip.h) is written as fill by
// every one of its workgroups, because each of them evaluates the whole line, not only its own 64 columns.
#include "common.h"
#include "stitch_blend.h"

namespace {

constexpr int STITCH_TX = 64, STITCH_TY = 16;   // tile: 64 columns x 16 rows, 256 threads x 4 rows each
constexpr int STITCH_MAX_WIN = 1 << 16;         // bounds the scan of a line's windows

struct alignas(8) StitchCol {
    unsigned long long pa, pb;   // pixel index of the column in row 0 of its first / second window's SR image
    int t, D;                    // D >= 1: two windows, column A + t of the D-column overlap; D == 0: one window; D < 0: fill
};

__global__ void __launch_bounds__(256) stitch_u8_kernel(const unsigned char* __restrict__ sr, int n_sr, int rows, int sr_w,
                                                        const mnet_stitch_line* __restrict__ lines, const mnet_stitch_window* __restrict__ windows,
                                                        int out_w, int tiles_x, int tiles_y, unsigned char* __restrict__ dst) {
    __shared__ StitchCol s_col[STITCH_TX];
    const int bid = (int)blockIdx.x;
    const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y, k = bid / (tiles_x * tiles_y);
    const mnet_stitch_line L = lines[k];
    const bool head = L.n_win >= 1 && L.n_win <= STITCH_MAX_WIN && L.win0 >= 0 && L.out_w >= 0 && L.out_w <= out_w;
    const int line_w = head ? L.out_w : 0;
    const int x0 = tile_x * STITCH_TX, y0 = tile_y * STITCH_TY;
    const int t = (int)threadIdx.x, tx = t & (STITCH_TX - 1), ty = t / STITCH_TX;
    const int x = x0 + tx;
    const bool live = x0 < line_w;                               // uniform over the workgroup
    if (live) {
        if (t < STITCH_TX) {
            // one pass over the line's windows: the line's validity (the same answer in every thread of every workgroup of the line) and
            // this column's cover.  Offsets increase strictly, so the windows that hold a column come in table order.
            bool ok = true;
            long long prev_off = -1, m1 = 0, m2 = 0;             // the two largest window ends so far
            int cover = 0;
            long long end_a = 0;
            StitchCol c = {0ull, 0ull, 0, -1};
            const mnet_stitch_window* w = windows + L.win0;
            for (int j = 0; j < L.n_win; ++j) {
                const mnet_stitch_window W = w[j];
                if (W.sr_index < 0 || W.sr_index >= n_sr || W.show_w < 1 || W.show_w > sr_w || W.offset < 0 || (long long)W.offset <= prev_off) {
                    ok = false;
                    break;
                }
                const long long off = W.offset, end = off + W.show_w;
                if ((off > m1 && m1 < line_w) || (off < m2 && off < line_w)) {    // a column of the line that no window holds (m1), or one that three hold (off)
                    ok = false;
                    break;
                }
                prev_off = off;
                if (end > m1) { m2 = m1; m1 = end; } else if (end > m2) { m2 = end; }
                if (x >= off && x < end) {
                    const unsigned long long p = ((unsigned long long)W.sr_index * (unsigned)rows) * (unsigned)sr_w + (unsigned)(x - (int)off);
                    if (cover == 0) { c.pa = p; end_a = end; }
                    else { c.pb = p; c.t = x - (int)off; c.D = (int)(end_a - off); }
                    ++cover;
                }
            }
            if (ok && m1 < line_w) ok = false;                   // the line's last columns are not covered
            if (ok && x < line_w && cover >= 1) { if (cover == 1) c.D = 0; } else c.D = -1;
            s_col[t] = c;
        }
        __syncthreads();
    }
    if (x >= out_w) return;
#pragma unroll
    for (int i = 0; i < STITCH_TY / 4; ++i) {
        const int y = y0 + ty + 4 * i;
        if (y >= rows) break;
        unsigned px[3] = {0u, 0u, 0u};                           // the fill: black
        if (live) {
            const StitchCol c = s_col[tx];
            if (c.D >= 0) {
                const unsigned char* a = sr + (c.pa + (unsigned long long)y * (unsigned)sr_w) * 3;
                if (c.D == 0) {
                    px[0] = a[0]; px[1] = a[1]; px[2] = a[2];
                } else {
                    const unsigned char* b = sr + (c.pb + (unsigned long long)y * (unsigned)sr_w) * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) px[ch] = stitch_blend(a[ch], b[ch], (unsigned)c.t, (unsigned)c.D);
                }
            }
        }
        unsigned char* d = dst + (((size_t)k * rows + y) * out_w + x) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) d[ch] = (unsigned char)px[ch];
    }
}

}  // namespace

extern "C" int mnet_stitch_u8(const uint8_t* sr, int32_t n_sr, int32_t rows, int32_t sr_w, const mnet_stitch_line* lines,
                              const mnet_stitch_window* windows, int32_t n_lines, int32_t out_w, uint8_t* dst, void* stream) {
    MNET_CHECK_ARG(sr && lines && windows && dst, "stitch_u8: null pointer");
    MNET_CHECK_ARG(n_lines > 0 && rows >= 1 && sr_w >= 1 && out_w >= 1 && n_sr >= 1, "stitch_u8: bad shape (n_lines=%d, rows=%d, sr_w=%d, out_w=%d, n_sr=%d)",
                   n_lines, rows, sr_w, out_w, n_sr);
    MNET_CHECK_ARG(sr_w <= STITCH_MAX_D, "stitch_u8: sr_w %d too large (the blend's 32-bit arithmetic holds up to %d columns)", sr_w, STITCH_MAX_D);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(lines) & 3) == 0 && (reinterpret_cast<uintptr_t>(windows) & 3) == 0,
                     "stitch_u8: lines and windows must be 4-byte aligned");
    const int tiles_x = (out_w + STITCH_TX - 1) / STITCH_TX, tiles_y = (rows + STITCH_TY - 1) / STITCH_TY;
    const long long grid = (long long)n_lines * tiles_x * tiles_y;
    MNET_CHECK_ARG(grid <= 0x7fffffffll, "stitch_u8: batch too large (%lld tiles)", grid);
    hipLaunchKernelGGL(stitch_u8_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), sr, n_sr, rows, sr_w, lines, windows,
                       out_w, tiles_x, tiles_y, dst);
    MNET_LAUNCH_CHECK("stitch_u8");
    return MNET_OK;
}
