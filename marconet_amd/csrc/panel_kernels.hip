// a17, the output side of the script's driver glue on the device (test_sr.py:203-232): the panel the script saves per strip — preview | preview
// with box marks | SR | structure images — for a whole batch in ONE launch, as the uint8 RGB array cv2.imwrite's file holds.  The definition is
// the host's: lq_io.panel_rgb_u8(lq_io.panel(...)), bit for bit.  Three row blocks are byte moves (the marks are two constant colours); the
// fourth is lq_io.resize_linear over the strip's structure images side by side — two taps per column from panel_taps.h, the source value
// p * 0.5 + 0.5, the blend p0 (1 - t) + p1 t and the * 255 each rounded operation by operation in fp32 (this file is compiled with
// -ffp-contract=off), then cv2's saturate_cast<uchar> (rintf: half to even).  resize_linear's vertical pass is the identity for 128 → 128 rows
// (t = 0: hor * 1 + hor * 0), so there is none here and the row height is fixed.
//
// Launch shape (as lq_from_u8_kernel): one thread per output pixel, x fastest; a workgroup takes a 64-column x 16-row tile of one strip — 128 is
// a multiple of 16, so the row block (and the half of the marks block) is uniform per workgroup — and computes what depends on the column alone
// once into LDS: the 64 taps of a structure tile, the 64 mark flags of a marks tile (a scan of the strip's intervals).  The prior is read as one
// aligned 16-byte load per tap (NHWC, 4 floats per pixel).  A tile wholly at columns >= show_w loads nothing and writes 0.  The kernel is tiny
// and HBM-side: at most ~4 MiB read and 3 MiB written per strip.
// Bounds: every store is bounded by (512, out_w); x < show_w <= out_w <= preview_w and the SR column is clamped into [0, sr_w); tap columns lie
// in [0, 128 n_glyphs).  A descriptor with show_w outside [0, out_w], a negative index or a glyph count outside [1, PANEL_MAX_GLYPHS] is
// written as fill and not followed — a table whose (preview_index, glyph0, n_glyphs) lie inside the tensors cannot take the kernel out of range.
#include "common.h"
#include "panel_taps.h"

namespace {

constexpr int PANEL_TX = 64, PANEL_TY = 16;     // tile: 64 columns x 16 rows, 256 threads x 4 rows each
constexpr int PANEL_ROW_H = 128, PANEL_H = 4 * PANEL_ROW_H;
constexpr int PANEL_MAX_GLYPHS = 1 << 16;       // keeps 128 * n_glyphs (and the per-strip pixel offsets) far inside int32

struct alignas(16) PanelF4 { float v[4]; };
struct alignas(16) PanelCol { int o0, o1; float w0, w1; };   // pixel offsets of the two taps within the strip's glyphs; weights 1 - t, t

__device__ inline int panel_u8(float v) {                    // saturate_cast<uchar>(v * 255)
    return (int)fminf(fmaxf(rintf(__fmul_rn(v, 255.0f)), 0.0f), 255.0f);
}

__global__ void __launch_bounds__(256) panel_u8_kernel(const unsigned char* __restrict__ preview, int preview_w, const unsigned char* __restrict__ sr_bgr,
                                                       int sr_w, const PanelF4* __restrict__ prior, const mnet_panel_strip* __restrict__ strips,
                                                       const int* __restrict__ marks, int out_w, int tiles_x, unsigned char* __restrict__ dst) {
    __shared__ PanelCol s_col[PANEL_TX];
    __shared__ int s_flag[PANEL_TX];
    constexpr int tiles_y = PANEL_H / PANEL_TY;
    const int bid = (int)blockIdx.x;
    const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y, k = bid / (tiles_x * tiles_y);
    const mnet_panel_strip s = strips[k];
    const bool ok = s.show_w >= 0 && s.show_w <= out_w && s.preview_index >= 0 && s.glyph0 >= 0 && s.n_glyphs >= 1 && s.n_glyphs <= PANEL_MAX_GLYPHS;
    const int show_w = ok ? s.show_w : 0;
    const int x0 = tile_x * PANEL_TX, y0 = tile_y * PANEL_TY;
    const int t = (int)threadIdx.x, tx = t & (PANEL_TX - 1), ty = t / PANEL_TX;
    const int x = x0 + tx;
    const int block = y0 / PANEL_ROW_H, yb = y0 % PANEL_ROW_H;   // uniform over the workgroup
    const bool live = x0 < show_w;
    if (live && block == 1) {
        if (t < PANEL_TX) {
            // upper half: the red interval [a, b) of every glyph; lower half: the blue interval [r, t)
            const int* m = marks + (size_t)s.glyph0 * 4 + (yb < PANEL_ROW_H / 2 ? 0 : 2);
            int hit = 0;
            for (int g = 0; g < s.n_glyphs; ++g) hit |= (x >= m[4 * g] && x < m[4 * g + 1]) ? 1 : 0;
            s_flag[t] = hit;
        }
        __syncthreads();
    } else if (live && block == 3) {
        if (t < PANEL_TX) {
            const PanelTap p = panel_linear_tap(x, PANEL_ROW_H * s.n_glyphs, s.step);
            PanelCol c;
            c.o0 = (p.i0 / PANEL_ROW_H) * (PANEL_ROW_H * PANEL_ROW_H) + p.i0 % PANEL_ROW_H;
            c.o1 = (p.i1 / PANEL_ROW_H) * (PANEL_ROW_H * PANEL_ROW_H) + p.i1 % PANEL_ROW_H;
            c.w0 = __fsub_rn(1.0f, p.t);
            c.w1 = p.t;
            s_col[t] = c;
        }
        __syncthreads();
    }
    if (x >= out_w) return;
#pragma unroll
    for (int i = 0; i < PANEL_TY / 4; ++i) {
        const int r = yb + ty + 4 * i, y = y0 + ty + 4 * i;      // r: row within the block's 128
        int px[3] = {0, 0, 0};                                    // the fill: black
        if (x < show_w) {
            if (block < 2) {
                const unsigned char* p = preview + (((size_t)s.preview_index * PANEL_ROW_H + r) * preview_w + x) * 3;
                if (block == 1 && s_flag[tx]) {
                    px[0] = yb < PANEL_ROW_H / 2 ? 255 : 0;
                    px[2] = yb < PANEL_ROW_H / 2 ? 0 : 255;
                } else {
                    px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
                }
            } else if (block == 2) {
                const unsigned char* p = sr_bgr + (((size_t)k * PANEL_ROW_H + r) * sr_w + min(x, sr_w - 1)) * 3;
                px[0] = p[2]; px[1] = p[1]; px[2] = p[0];
            } else {
                const PanelCol c = s_col[tx];
                const PanelF4* row = prior + ((size_t)s.glyph0 * PANEL_ROW_H + r) * PANEL_ROW_H;
                const PanelF4 a = row[c.o0], b = row[c.o1];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {                  // file channel ch = prior channel 2 - ch: the script stacks this row unflipped
                    const float p0 = __fadd_rn(__fmul_rn(a.v[2 - ch], 0.5f), 0.5f), p1 = __fadd_rn(__fmul_rn(b.v[2 - ch], 0.5f), 0.5f);
                    px[ch] = panel_u8(__fadd_rn(__fmul_rn(p0, c.w0), __fmul_rn(p1, c.w1)));
                }
            }
        }
        unsigned char* d = dst + (((size_t)k * PANEL_H + y) * out_w + x) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) d[ch] = (unsigned char)px[ch];
    }
}

}  // namespace

extern "C" int mnet_panel_u8(const uint8_t* preview, int32_t preview_w, const uint8_t* sr_bgr, int32_t sr_w, const float* prior_nhwc4,
                             const mnet_panel_strip* strips, const int32_t* marks, int32_t n, int32_t out_w, uint8_t* dst, void* stream) {
    MNET_CHECK_ARG(preview && sr_bgr && prior_nhwc4 && strips && marks && dst, "panel_u8: null pointer");
    MNET_CHECK_ARG(n > 0 && out_w >= 1 && preview_w >= out_w && sr_w >= 1, "panel_u8: bad shape (n=%d, out_w=%d, preview_w=%d, sr_w=%d)", n, out_w,
                   preview_w, sr_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(prior_nhwc4) & 15) == 0 && (reinterpret_cast<uintptr_t>(strips) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(marks) & 3) == 0, "panel_u8: prior_nhwc4 must be 16-byte, strips 8-byte, marks 4-byte aligned");
    const int tiles_x = (out_w + PANEL_TX - 1) / PANEL_TX;
    const long long grid = (long long)n * tiles_x * (PANEL_H / PANEL_TY);
    MNET_CHECK_ARG(grid <= 0x7fffffffll, "panel_u8: batch too large (%lld tiles)", grid);
    hipLaunchKernelGGL(panel_u8_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), preview, preview_w, sr_bgr, sr_w,
                       reinterpret_cast<const PanelF4*>(prior_nhwc4), strips, marks, out_w, tiles_x, dst);
    MNET_LAUNCH_CHECK("panel_u8");
    return MNET_OK;
}
