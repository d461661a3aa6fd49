// The encoder's input straight from WINDOWS of images on the device (include/marconet_hip_windows.h): lq_kernels.hip's form 0 for a source that is
// a view — a first byte, a row pitch and a size — so that the overlapping probe windows of a line, and the windows of a page that is uploaded anyway,
// need no second copy of their pixels.  The arithmetic is lq_kernels.hip's own, through page_tile.h: the taps are those of the WINDOW's w columns
// and h rows, so BORDER_REPLICATE clamps into the window and not into the image around it, and pt_cubic_rgb takes the window's first byte and the
// image's pitch separately; the result is mnet_lq_from_u8's for the same pixels copied out tightly, bit for bit (tests/test_window_kernels_gpu.py).
//
// Launch shape: page_tile.h's tile over one window's canvas, one launch for all windows.  A tile wholly at columns >= dw loads nothing.
// Bounds: every source index is clamped into its window (row index < h, column byte < 3 w <= pitch) and the window's last byte,
// offset + (h - 1) pitch + 3 w, is checked against src_bytes in 64 bits; a descriptor that fails — or has h < 1, w < 1, pitch < 3 w or a negative
// offset — is written as fill.  Every store is bounded by (dst_h, canvas_w).
#include "common.h"
#include "../../include/marconet_hip_windows.h"
#include "page_tile.h"

namespace {

__device__ __forceinline__ bool window_ok(const mnet_lq_window& wd, long long src_bytes) {
    if (wd.h < 1 || wd.w < 1 || wd.offset < 0 || (long long)wd.pitch < 3ll * wd.w) return false;
    // offset <= src_bytes first: the sum below then stays far inside 64 bits (pitch, h < 2^31)
    return wd.offset <= src_bytes && (long long)(wd.h - 1) * wd.pitch + 3ll * wd.w <= src_bytes - wd.offset;
}

__global__ void __launch_bounds__(256) lq_windows_u8_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                            const mnet_lq_window* __restrict__ windows, int dst_h, int canvas_w, int tiles_x, int tiles_y,
                                                            float* __restrict__ dst) {
    __shared__ PtTaps s;
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const int win = T.desc;
    const mnet_lq_window wd = windows[win];
    const int dw = window_ok(wd, src_bytes) ? min(max(wd.dw, 0), canvas_w) : 0;
    const int t = (int)threadIdx.x, tx = t & (PT_TX - 1), ty = t / PT_TX;
    const int x = T.x0 + tx;
    if (T.x0 < dw) pt_stage_taps(s, T, wd.w, wd.scale, wd.h, wd.scale, 0, 3, 0);      // uniform over the workgroup
    if (x >= canvas_w) return;
    const size_t row_bytes = (size_t)wd.pitch;
    const unsigned char* base = src + wd.offset;
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        const int r = ty + 4 * i, y = T.y0 + r;
        if (y >= dst_h) break;
        int px[3] = {0, 0, 0};                        // the fill: black
        if (x < dw) {
            int acc[3];
            pt_cubic_rgb(base, row_bytes, s.ci[tx], s.ct[tx], s.ri[r], s.rt[r], acc);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = pt_round_clip(acc[c]);
        }
        // ToTensor + Normalize(0.5, 0.5) as torch evaluates them in fp32, as lq_from_u8_kernel's form 0 states them
        float* d = dst + (((size_t)win * 3) * dst_h + y) * canvas_w + x;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            d[(size_t)c * dst_h * canvas_w] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)px[c], 255.0f), 0.5f), 0.5f);
    }
}

}  // namespace

extern "C" int mnet_lq_windows_u8(const uint8_t* src, int64_t src_bytes, const mnet_lq_window* windows, int32_t n, int32_t dst_h, int32_t canvas_w,
                                  void* dst, int32_t form, void* stream) {
    MNET_CHECK_ARG(src && windows && dst, "lq_windows_u8: null pointer");
    MNET_CHECK_ARG(n > 0 && dst_h >= 1 && canvas_w >= 1 && src_bytes >= 1, "lq_windows_u8: bad shape (n=%d, dst_h=%d, canvas_w=%d, src_bytes=%lld)", n,
                   dst_h, canvas_w, (long long)src_bytes);
    MNET_CHECK_ARG(form == MNET_LQ_FORM_F32_NCHW, "lq_windows_u8: form %d (fp32 NCHW, %d, is the only one)", form, (int)MNET_LQ_FORM_F32_NCHW);
    MNET_CHECK_ALIGN(reinterpret_cast<uintptr_t>(windows) % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
                     "lq_windows_u8: the window table must be 8-byte aligned and dst 4-byte aligned");
    const PtGrid g = pt_grid(n, canvas_w, dst_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "lq_windows_u8: batch too large (%lld tiles)", g.blocks);
    hipLaunchKernelGGL(lq_windows_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, (long long)src_bytes,
                       windows, dst_h, canvas_w, (int)g.tiles_x, (int)g.tiles_y, reinterpret_cast<float*>(dst));
    MNET_LAUNCH_CHECK("lq_windows_u8");
    return MNET_OK;
}
