// a17, the input side of the script's driver glue on the device (test_sr.py:98-115): a ragged batch of tightly packed uint8 RGB strips →
// the encoder's input (form 0) or the panel's preview (form 1), in ONE launch.  The arithmetic is marconet_amd/lq_io.py::resize_cubic — the
// project's statement of cv2.resize(INTER_CUBIC) on an 8-bit image — bit for bit: taps from lq_taps.h, both passes in integers, one rounding
// shift by 22 bits (page_tile.h: the cubic and its int32 bound).
//
// Launch shape: page_tile.h's tile over one image's canvas (each NCHW plane is written coalesced).  A tile wholly at columns >= dw loads nothing
// and writes the fill value.  Source bytes are read with byte loads (an image's offset in the packed buffer is odd in general); the kernel is
// tiny next to the forward (16 source pixels per output pixel, 2 MiB of output per 32 strips).
// Bounds: every source index is clamped into its image and every store is bounded by (dst_h, canvas_w); dw is clamped into [0, canvas_w] and an
// image with h < 1, w < 1 or a negative offset is written as fill — a table whose (offset, h, w) lie inside the source buffer cannot take the
// kernel out of range.
#include "common.h"
#include "page_tile.h"

namespace {

template <int FORM>
__global__ void __launch_bounds__(256) lq_from_u8_kernel(const unsigned char* __restrict__ src, const mnet_lq_image* __restrict__ images, int dst_h,
                                                         int canvas_w, int tiles_x, int tiles_y, void* __restrict__ dst) {
    __shared__ PtTaps s;
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const int img = T.desc;
    const mnet_lq_image im = images[img];
    const int h = im.h, w = im.w;
    const int dw = (h < 1 || w < 1 || im.offset < 0) ? 0 : min(max(im.dw, 0), canvas_w);
    const int t = (int)threadIdx.x, tx = t & (PT_TX - 1), ty = t / PT_TX;
    const int x = T.x0 + tx;
    if (T.x0 < dw) pt_stage_taps(s, T, w, im.scale, h, im.scale, 0, 3, 0);      // uniform over the workgroup
    if (x >= canvas_w) return;
    const size_t row_bytes = (size_t)w * 3;
    const unsigned char* base = src + im.offset;
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
        if constexpr (FORM == 0) {
            // ToTensor + Normalize(0.5, 0.5) as torch evaluates them in fp32: (u8 / 255 - 0.5) / 0.5, every step correctly rounded
            float* d = reinterpret_cast<float*>(dst) + (((size_t)img * 3) * dst_h + y) * canvas_w + x;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[(size_t)c * dst_h * canvas_w] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)px[c], 255.0f), 0.5f), 0.5f);
        } else {
            unsigned char* d = reinterpret_cast<unsigned char*>(dst) + (((size_t)img * dst_h + y) * canvas_w + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = (unsigned char)px[c];
        }
    }
}

}  // namespace

extern "C" int mnet_lq_from_u8(const uint8_t* src, const mnet_lq_image* images, int32_t n, int32_t dst_h, int32_t canvas_w, void* dst,
                               int32_t form, void* stream) {
    MNET_CHECK_ARG(src && images && dst, "lq_from_u8: null pointer");
    MNET_CHECK_ARG(n > 0 && dst_h >= 1 && canvas_w >= 1, "lq_from_u8: bad shape (n=%d, dst_h=%d, canvas_w=%d)", n, dst_h, canvas_w);
    MNET_CHECK_ARG(form == MNET_LQ_FORM_F32_NCHW || form == MNET_LQ_FORM_U8_HWC, "lq_from_u8: unknown form %d", form);
    const PtGrid g = pt_grid(n, canvas_w, dst_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "lq_from_u8: batch too large (%lld tiles)", g.blocks);
    const int tiles_x = (int)g.tiles_x, tiles_y = (int)g.tiles_y;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (form == MNET_LQ_FORM_F32_NCHW)
        hipLaunchKernelGGL(lq_from_u8_kernel<0>, dim3((unsigned)g.blocks), dim3(256), 0, st, src, images, dst_h, canvas_w, tiles_x, tiles_y, dst);
    else
        hipLaunchKernelGGL(lq_from_u8_kernel<1>, dim3((unsigned)g.blocks), dim3(256), 0, st, src, images, dst_h, canvas_w, tiles_x, tiles_y, dst);
    MNET_LAUNCH_CHECK("lq_from_u8");
    return MNET_OK;
}
