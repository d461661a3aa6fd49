// Text regions that are convex quadrilaterals of a page: the gather in (mnet_quad_crop_u8: every window of every region rectified into the ragged
// batch mnet_lq_from_u8 reads) and the gather out (mnet_quad_paste_u8: every region's upright foreground pasted into its quadrilateral of the
// enlarged page), each for all regions of the page in ONE launch.  The definition is the host's, byte for byte: marconet_amd/quads.py's
// warp_crop_host / warp_paste_host.  The projective maps are nine doubles per descriptor, computed on the host; per pixel there are six
// multiplications, six additions and two IEEE divisions in fp64 (quad_map.h: every operation rounded separately, hence -ffp-contract=off for this
// translation unit — the expansion of the division keeps its own fused operations, which is what makes it correctly rounded), a bilinear mix in
// integers, and for the paste the integer feather of page_blend.h.
//
// Launch shape: page_tile.h's tile over one descriptor's output; the grid is n descriptors x the tiles of the largest one, whose size the caller
// passes; a workgroup whose tile lies outside its descriptor returns before it loads anything.  The descriptor is read uniformly per workgroup;
// sources are read with byte loads (3-byte pixels at any offset), no LDS is needed.
// Bounds: a descriptor is followed only if it passes the checks below (the list: include/marconet_hip_quad.h) — every workgroup of a descriptor
// takes the same decision from the same bytes.  Crop: every page index is clamped into [0, page_h) x [0, page_w), every store lies in
// [offset, offset + 3 w h) of dst, which lies inside [0, dst_bytes).  Paste: every atlas index is clamped into the foreground's rectangle, which
// lies inside the atlas; the page is read and written at the thread's own pixel only, inside the bounding box, which lies inside the page.
#include "common.h"
#include "../../include/marconet_hip_quad.h"
#include "quad_map.h"
#include "page_blend.h"
#include "page_tile.h"
#include "warp_paste.h"

namespace {

__global__ void __launch_bounds__(256) quad_crop_u8_kernel(const unsigned char* __restrict__ page, int page_h, int page_w,
                                                           const mnet_quad_crop* __restrict__ crops, int tiles_x, int tiles_y,
                                                           unsigned char* __restrict__ dst, long long dst_bytes) {
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const mnet_quad_crop C = crops[T.desc];
    const int w = C.w, h = C.h;
    const bool ok = w >= 1 && h >= 1 && C.c0 >= 0 && C.offset >= 0 && C.offset <= dst_bytes && (long long)w * h <= (dst_bytes - C.offset) / 3 &&
                    quad_finite9(C.m);
    const int i0 = T.x0, j0 = T.y0;
    if (!ok || i0 >= w || j0 >= h) return;               // uniform over the workgroup
    const int t = (int)threadIdx.x, i = i0 + (t & (PT_TX - 1)), ty = t / PT_TX;
    if (i >= w) return;
    const double x = LQ_DADD((double)((long long)C.c0 + i), 0.5);
    const size_t row_bytes = (size_t)page_w * 3;
    unsigned char* out = dst + C.offset;
#pragma unroll
    for (int r = 0; r < PT_TY / 4; ++r) {
        const int j = j0 + ty + 4 * r;
        if (j >= h) break;
        const QuadPos p = quad_pos(C.m, x, LQ_DADD((double)j, 0.5));
        unsigned char* d = out + ((size_t)j * w + (size_t)i) * 3;
        if (!p.valid) {
            d[0] = 0; d[1] = 0; d[2] = 0;
            continue;
        }
        const QuadTaps q = quad_taps(quad_fix(p.u), quad_fix(p.v), page_w, page_h);
        const unsigned char* r0 = page + (size_t)q.y0 * row_bytes;
        const unsigned char* r1 = page + (size_t)q.y1 * row_bytes;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            d[ch] = (unsigned char)quad_mix(r0[(size_t)q.x0 * 3 + ch], r0[(size_t)q.x1 * 3 + ch], r1[(size_t)q.x0 * 3 + ch], r1[(size_t)q.x1 * 3 + ch], q.ax, q.ay);
    }
}

__global__ void __launch_bounds__(256) quad_paste_u8_kernel(const unsigned char* __restrict__ atlas, int atlas_h, int atlas_w,
                                                            const mnet_quad_region* __restrict__ regions, int tiles_x, int tiles_y,
                                                            unsigned char* page, int page_h, int page_w) {
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const mnet_quad_region R = regions[T.desc];
    const int rw = R.rw, rh = R.rh, bw = R.bw, bh = R.bh;
    const int i0 = T.x0, j0 = T.y0;
    if (!quad_region_followed(R, atlas_h, atlas_w, page_h, page_w) || i0 >= bw || j0 >= bh) return;             // uniform over the workgroup
    const int t = (int)threadIdx.x, i = i0 + (t & (PT_TX - 1)), ty = t / PT_TX;
    if (i >= bw) return;
    const int X = R.bx0 + i;
    const double x = LQ_DADD((double)X, 0.5);
    const size_t row_bytes = (size_t)atlas_w * 3;
    const unsigned char* fg0 = atlas + ((size_t)R.ay0 * atlas_w + (size_t)R.ax0) * 3;
#pragma unroll
    for (int r = 0; r < PT_TY / 4; ++r) {
        const int j = j0 + ty + 4 * r;
        if (j >= bh) break;
        const int Y = R.by0 + j;
        quad_paste_pixel(R.n, rw, rh, (unsigned)R.feather, fg0, row_bytes, x, LQ_DADD((double)Y, 0.5), page + ((size_t)Y * page_w + (size_t)X) * 3);
    }
}

}  // namespace

extern "C" int mnet_quad_crop_u8(const uint8_t* page, int32_t page_h, int32_t page_w, const mnet_quad_crop* crops, int32_t n, int32_t max_w, int32_t max_h,
                                 uint8_t* dst, int64_t dst_bytes, void* stream) {
    MNET_CHECK_ARG(page && crops && dst, "quad_crop_u8: null pointer");
    MNET_CHECK_ARG(page_h >= 1 && page_w >= 1 && n >= 1 && max_w >= 1 && max_h >= 1 && dst_bytes >= 1,
                   "quad_crop_u8: bad shape (page_h=%d, page_w=%d, n=%d, max_w=%d, max_h=%d, dst_bytes=%lld)", page_h, page_w, n, max_w, max_h, (long long)dst_bytes);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(crops) & 7) == 0, "quad_crop_u8: crops must be 8-byte aligned");
    const PtGrid g = pt_grid(n, max_w, max_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "quad_crop_u8: batch too large (%d crops of %lld x %lld tiles)", n, g.tiles_x, g.tiles_y);
    hipLaunchKernelGGL(quad_crop_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), page, page_h, page_w, crops,
                       (int)g.tiles_x, (int)g.tiles_y, dst, (long long)dst_bytes);
    MNET_LAUNCH_CHECK("quad_crop_u8");
    return MNET_OK;
}

extern "C" int mnet_quad_paste_u8(const uint8_t* atlas, int32_t atlas_h, int32_t atlas_w, const mnet_quad_region* regions, int32_t n, int32_t max_bw,
                                  int32_t max_bh, uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    MNET_CHECK_ARG(atlas && regions && page, "quad_paste_u8: null pointer");
    MNET_CHECK_ARG(atlas_h >= 1 && atlas_w >= 1 && n >= 1 && max_bw >= 1 && max_bh >= 1 && page_h >= 1 && page_w >= 1,
                   "quad_paste_u8: bad shape (atlas_h=%d, atlas_w=%d, n=%d, max_bw=%d, max_bh=%d, page_h=%d, page_w=%d)", atlas_h, atlas_w, n, max_bw, max_bh, page_h, page_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(regions) & 7) == 0, "quad_paste_u8: regions must be 8-byte aligned");
    const PtGrid g = pt_grid(n, max_bw, max_bh);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "quad_paste_u8: batch too large (%d regions of %lld x %lld tiles)", n, g.tiles_x, g.tiles_y);
    hipLaunchKernelGGL(quad_paste_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), atlas, atlas_h, atlas_w, regions,
                       (int)g.tiles_x, (int)g.tiles_y, page, page_h, page_w);
    MNET_LAUNCH_CHECK("quad_paste_u8");
    return MNET_OK;
}
