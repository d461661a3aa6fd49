// a17, the input side of the script's driver glue on the device (test_sr.py:98-115): a ragged batch of tightly packed uint8 RGB strips →
// the encoder's input (form 0) or the panel's preview (form 1), in ONE launch.  The arithmetic is marconet_amd/lq_io.py::resize_cubic — the
// project's statement of cv2.resize(INTER_CUBIC) on an 8-bit image — bit for bit: taps from lq_taps.h, both passes in integers, one rounding
// shift by 22 bits.  With sum |taps| <= 2816 per axis, |v| <= 255 * 2816^2 and v + 2^21 <= 2 024 210 432 < 2^31: int32 holds every sum
// (tests/test_lq_device.py asserts the tap bound), and integer sums are exact in any order.
//
// Launch shape: one thread per output pixel, x fastest (each NCHW plane is written coalesced); a workgroup takes a 64-column x 16-row tile of one
// image and computes the tile's 64 column taps and 16 row taps once into LDS (fp64 sample positions: 80 lanes, not 1024 pixels).  A tile wholly at
// columns >= dw loads nothing and writes the fill value.  Source bytes are read with byte loads (an image's offset in the packed buffer is odd in
// general); the kernel is tiny next to the forward (16 source pixels per output pixel, 2 MiB of output per 32 strips).
// Bounds: every source index is clamped into its image and every store is bounded by (dst_h, canvas_w); dw is clamped into [0, canvas_w] and an
// image with h < 1, w < 1 or a negative offset is written as fill — a table whose (offset, h, w) lie inside the source buffer cannot take the
// kernel out of range.
#include "common.h"
#include "lq_taps.h"

namespace {

constexpr int LQ_TX = 64, LQ_TY = 16;      // tile: 64 columns x 16 rows, 256 threads x 4 rows each

struct alignas(16) LqI4 { int v[4]; };

template <int FORM>
__global__ void __launch_bounds__(256) lq_from_u8_kernel(const unsigned char* __restrict__ src, const mnet_lq_image* __restrict__ images, int dst_h,
                                                         int canvas_w, int tiles_x, int tiles_y, void* __restrict__ dst) {
    __shared__ LqI4 s_ci[LQ_TX], s_ct[LQ_TX], s_ri[LQ_TY], s_rt[LQ_TY];
    const int bid = (int)blockIdx.x;
    const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y, img = bid / (tiles_x * tiles_y);
    const mnet_lq_image im = images[img];
    const int h = im.h, w = im.w;
    const int dw = (h < 1 || w < 1 || im.offset < 0) ? 0 : min(max(im.dw, 0), canvas_w);
    const int x0 = tile_x * LQ_TX, y0 = tile_y * LQ_TY;
    const int t = (int)threadIdx.x, tx = t & (LQ_TX - 1), ty = t / LQ_TX;
    const int x = x0 + tx;
    const bool live = x0 < dw;                       // uniform over the workgroup
    if (live) {
        if (t < LQ_TX) {
            const LqTaps c = lq_cubic_taps(x0 + t, w, im.scale);
#pragma unroll
            for (int k = 0; k < 4; ++k) { s_ci[t].v[k] = c.idx[k] * 3; s_ct[t].v[k] = c.tap[k]; }
        } else if (t < LQ_TX + LQ_TY) {
            const int r = t - LQ_TX;
            const LqTaps c = lq_cubic_taps(y0 + r, h, im.scale);
#pragma unroll
            for (int k = 0; k < 4; ++k) { s_ri[r].v[k] = c.idx[k]; s_rt[r].v[k] = c.tap[k]; }
        }
        __syncthreads();
    }
    if (x >= canvas_w) return;
    const size_t row_bytes = (size_t)w * 3;
    const unsigned char* base = src + im.offset;
#pragma unroll
    for (int i = 0; i < LQ_TY / 4; ++i) {
        const int r = ty + 4 * i, y = y0 + r;
        if (y >= dst_h) break;
        int px[3] = {0, 0, 0};                        // the fill: black
        if (x < dw) {
            const LqI4 ci = s_ci[tx], ct = s_ct[tx], ri = s_ri[r], rt = s_rt[r];
            int acc[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned char* row = base + (size_t)ri.v[j] * row_bytes;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int hor = (int)row[ci.v[0] + c] * ct.v[0] + (int)row[ci.v[1] + c] * ct.v[1] + (int)row[ci.v[2] + c] * ct.v[2] +
                                    (int)row[ci.v[3] + c] * ct.v[3];
                    acc[c] += hor * rt.v[j];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
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
    const int tiles_x = (canvas_w + LQ_TX - 1) / LQ_TX, tiles_y = (dst_h + LQ_TY - 1) / LQ_TY;
    const long long grid = (long long)n * tiles_x * tiles_y;
    MNET_CHECK_ARG(grid <= 0x7fffffffll, "lq_from_u8: batch too large (%lld tiles)", grid);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (form == MNET_LQ_FORM_F32_NCHW)
        hipLaunchKernelGGL(lq_from_u8_kernel<0>, dim3((unsigned)grid), dim3(256), 0, st, src, images, dst_h, canvas_w, tiles_x, tiles_y, dst);
    else
        hipLaunchKernelGGL(lq_from_u8_kernel<1>, dim3((unsigned)grid), dim3(256), 0, st, src, images, dst_h, canvas_w, tiles_x, tiles_y, dst);
    MNET_LAUNCH_CHECK("lq_from_u8");
    return MNET_OK;
}
