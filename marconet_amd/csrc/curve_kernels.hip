// Text regions that are curved strips of a page — polygons of 2K points, a chain of K - 1 bilinear segments: the gather in (mnet_curve_crop_u8: every
// window of every region rectified into the ragged batch mnet_lq_from_u8 reads) and the gather out (mnet_curve_paste_u8: every region's upright
// foreground pasted back along its curve), each for all regions of the page in ONE launch.  The definition is the host's, byte for byte:
// marconet_amd/curves.py's warp_crop_host / warp_paste_host.  A segment is eight doubles, computed on the host; per pixel the crop takes eight
// multiplications and six additions in fp64, the paste — per segment whose box holds the pixel — the inverse of curve_map.h: a quadratic's root, one
// square root and two IEEE divisions (every operation rounded separately, hence -ffp-contract=off for this translation unit — the expansions of the
// division and of the square root keep their own fused operations, which is what makes them correctly rounded); then quad_map.h's bilinear mix in
// integers, and for the paste the integer feather of page_blend.h.
//
// Launch shape: page_tile.h's tile over one descriptor's output; the grid is n descriptors x the tiles of the largest one, whose size the caller
// passes; a workgroup whose tile lies outside its descriptor returns before it loads anything.  The descriptor is read uniformly per workgroup; its
// segments (at most 32 x 88 bytes) are staged in LDS once per workgroup, one thread each, with the two cross products of the inverse that depend on
// the segment alone.  In the crop a thread's column fixes its segment once for all its rows; in the paste a thread rejects a segment by its integer
// box before any fp64, and a workgroup whose tile meets no segment box returns before it loads a pixel.  ONE thread runs a page pixel's whole loop
// over the segments, so a seam cannot have two writers.
// Bounds: a descriptor is followed only if it passes the checks below (the list: include/marconet_hip_curve.h) — every workgroup of a descriptor
// takes the same decision from the same bytes: the descriptor's own fields first, then — only when seg0 >= 0, 1 <= nseg <= 32 and
// seg0 + nseg <= n_segs, so that every segment index lies in [0, n_segs) — its segments', combined over the workgroup by a barrier that votes.  Every
// return before a barrier is uniform over the workgroup.  LDS: thread t < nseg <= 32 writes record t of 32; every later index is < nseg.
// Crop: the column c0 + i < c0 + w <= the sum of the widths, so the search for its segment ends inside the chain; every page index is clamped into
// [0, page_h) x [0, page_w); every store lies in [offset, offset + 3 w h) of dst, which lies inside [0, dst_bytes).  Paste: every atlas index is
// clamped into the foreground's rectangle ([0, rw) x [0, rh), the widths sum to rw), which lies inside the atlas; the feather's pixel is
// (u0 + floor u, floor v) with 0 <= u < w_s and 0 <= v < rh, integer sums, so it lies inside the rectangle too; the page is read and written at the
// thread's own pixel only, inside the region's bounding box, which lies inside the page.
#include "common.h"
#include "../../include/marconet_hip_curve.h"
#include "curve_map.h"
#include "page_blend.h"
#include "page_tile.h"
#include "warp_paste.h"

namespace {

static_assert(CURVE_MAX_SEGS == MNET_CURVE_MAX_SEGS, "curve_map.h and marconet_hip_curve.h disagree");
static_assert(sizeof(mnet_curve_seg) == 88 && sizeof(mnet_curve_crop) == 32 && sizeof(mnet_curve_region) == 48, "descriptor layout");

__global__ void __launch_bounds__(256) curve_crop_u8_kernel(const unsigned char* __restrict__ page, int page_h, int page_w,
                                                            const mnet_curve_crop* __restrict__ crops, const mnet_curve_seg* __restrict__ segs,
                                                            int n_segs, int tiles_x, int tiles_y, unsigned char* __restrict__ dst, long long dst_bytes) {
    __shared__ CurveSegL S[CURVE_MAX_SEGS];
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const mnet_curve_crop C = crops[T.desc];
    const int w = C.w, h = C.h, nseg = C.nseg;
    const bool ok = w >= 1 && h >= 1 && C.c0 >= 0 && C.offset >= 0 && C.offset <= dst_bytes && (long long)w * h <= (dst_bytes - C.offset) / 3 &&
                    C.seg0 >= 0 && nseg >= 1 && nseg <= CURVE_MAX_SEGS && (long long)C.seg0 + nseg <= n_segs;
    const int i0 = T.x0, j0 = T.y0;
    if (!ok || i0 >= w || j0 >= h) return;               // uniform over the workgroup
    const int t = (int)threadIdx.x;
    bool good = true;
    if (t < nseg) {
        mnet_curve_seg g;
        good = curve_stage(S, segs, C.seg0, t, g);
    }
    if (!__syncthreads_and(good ? 1 : 0)) return;        // the vote is the barrier: S is visible, and the decision is uniform
    if ((long long)C.c0 + w > (long long)S[nseg - 1].u0 + S[nseg - 1].w) return;
    const int i = i0 + (t & (PT_TX - 1)), ty = t / PT_TX;
    if (i >= w) return;
    const long long col = (long long)C.c0 + i;           // < the sum of the widths: the search ends at k < nseg
    int k = 0;
    while (k < nseg - 1 && col >= (long long)S[k].u0 + S[k].w) ++k;
    double c[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) c[m] = S[k].c[m];
    const double u = LQ_DADD((double)(col - S[k].u0), 0.5);
    const size_t row_bytes = (size_t)page_w * 3;
    unsigned char* out = dst + C.offset;
#pragma unroll
    for (int r = 0; r < PT_TY / 4; ++r) {
        const int j = j0 + ty + 4 * r;
        if (j >= h) break;
        const CurvePos p = curve_pos(c, u, LQ_DADD((double)j, 0.5));
        unsigned char* d = out + ((size_t)j * w + (size_t)i) * 3;
        if (!p.valid) {
            d[0] = 0; d[1] = 0; d[2] = 0;
            continue;
        }
        const QuadTaps q = quad_taps(quad_fix(p.x), quad_fix(p.y), page_w, page_h);
        const unsigned char* r0 = page + (size_t)q.y0 * row_bytes;
        const unsigned char* r1 = page + (size_t)q.y1 * row_bytes;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            d[ch] = (unsigned char)quad_mix(r0[(size_t)q.x0 * 3 + ch], r0[(size_t)q.x1 * 3 + ch], r1[(size_t)q.x0 * 3 + ch], r1[(size_t)q.x1 * 3 + ch], q.ax, q.ay);
    }
}

__global__ void __launch_bounds__(256) curve_paste_u8_kernel(const unsigned char* __restrict__ atlas, int atlas_h, int atlas_w,
                                                             const mnet_curve_region* __restrict__ regions, const mnet_curve_seg* __restrict__ segs,
                                                             int n_segs, int tiles_x, int tiles_y, unsigned char* page, int page_h, int page_w) {
    __shared__ CurveSegL S[CURVE_MAX_SEGS];
    const PtTile T = pt_tile(tiles_x, tiles_y);
    const mnet_curve_region R = regions[T.desc];
    const int rw = R.rw, rh = R.rh, bw = R.bw, bh = R.bh, nseg = R.nseg;
    const int i0 = T.x0, j0 = T.y0;
    if (!curve_region_followed(R, atlas_h, atlas_w, page_h, page_w, n_segs) || i0 >= bw || j0 >= bh) return;    // uniform over the workgroup
    const int t = (int)threadIdx.x;
    bool good = true, hit = false;
    if (t < nseg) {
        mnet_curve_seg g;
        good = curve_stage(S, segs, R.seg0, t, g) && curve_seg_in_region(g, R);
        hit = curve_seg_hits(g, (long long)R.bx0 + i0, (long long)R.by0 + j0, PT_TX, PT_TY);      // the tile's page pixels
    }
    if (!__syncthreads_and(good ? 1 : 0)) return;        // the vote is the barrier: S is visible, and the decision is uniform
    if ((long long)S[nseg - 1].u0 + S[nseg - 1].w != rw) return;
    if (!__syncthreads_or(hit ? 1 : 0)) return;          // the tile meets no segment's box: nothing to paste here
    const int i = i0 + (t & (PT_TX - 1)), ty = t / PT_TX;
    if (i >= bw) return;
    const int X = R.bx0 + i;
    const double x = LQ_DADD((double)X, 0.5);
    const size_t row_bytes = (size_t)atlas_w * 3;
    const unsigned char* fg0 = atlas + ((size_t)R.ay0 * atlas_w + (size_t)R.ax0) * 3;
#pragma unroll 1
    for (int r = 0; r < PT_TY / 4; ++r) {
        const int j = j0 + ty + 4 * r;
        if (j >= bh) break;
        const int Y = R.by0 + j;
        curve_paste_pixel(S, nseg, rw, rh, (unsigned)R.feather, fg0, row_bytes, X, Y, x, LQ_DADD((double)Y, 0.5), page + ((size_t)Y * page_w + (size_t)X) * 3);
    }
}

}  // namespace

extern "C" int mnet_curve_crop_u8(const uint8_t* page, int32_t page_h, int32_t page_w, const mnet_curve_crop* crops, int32_t n, const mnet_curve_seg* segs,
                                  int32_t n_segs, int32_t max_w, int32_t max_h, uint8_t* dst, int64_t dst_bytes, void* stream) {
    MNET_CHECK_ARG(page && crops && segs && dst, "curve_crop_u8: null pointer");
    MNET_CHECK_ARG(page_h >= 1 && page_w >= 1 && n >= 1 && n_segs >= 1 && max_w >= 1 && max_h >= 1 && dst_bytes >= 1,
                   "curve_crop_u8: bad shape (page_h=%d, page_w=%d, n=%d, n_segs=%d, max_w=%d, max_h=%d, dst_bytes=%lld)", page_h, page_w, n, n_segs, max_w, max_h,
                   (long long)dst_bytes);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(crops) & 7) == 0 && (reinterpret_cast<uintptr_t>(segs) & 7) == 0,
                     "curve_crop_u8: crops and segs must be 8-byte aligned");
    const PtGrid g = pt_grid(n, max_w, max_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "curve_crop_u8: batch too large (%d crops of %lld x %lld tiles)", n, g.tiles_x, g.tiles_y);
    hipLaunchKernelGGL(curve_crop_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), page, page_h, page_w, crops, segs,
                       n_segs, (int)g.tiles_x, (int)g.tiles_y, dst, (long long)dst_bytes);
    MNET_LAUNCH_CHECK("curve_crop_u8");
    return MNET_OK;
}

extern "C" int mnet_curve_paste_u8(const uint8_t* atlas, int32_t atlas_h, int32_t atlas_w, const mnet_curve_region* regions, int32_t n,
                                   const mnet_curve_seg* segs, int32_t n_segs, int32_t max_bw, int32_t max_bh, uint8_t* page, int32_t page_h, int32_t page_w,
                                   void* stream) {
    MNET_CHECK_ARG(atlas && regions && segs && page, "curve_paste_u8: null pointer");
    MNET_CHECK_ARG(atlas_h >= 1 && atlas_w >= 1 && n >= 1 && n_segs >= 1 && max_bw >= 1 && max_bh >= 1 && page_h >= 1 && page_w >= 1,
                   "curve_paste_u8: bad shape (atlas_h=%d, atlas_w=%d, n=%d, n_segs=%d, max_bw=%d, max_bh=%d, page_h=%d, page_w=%d)", atlas_h, atlas_w, n, n_segs,
                   max_bw, max_bh, page_h, page_w);
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(regions) & 7) == 0 && (reinterpret_cast<uintptr_t>(segs) & 7) == 0,
                     "curve_paste_u8: regions and segs must be 8-byte aligned");
    const PtGrid g = pt_grid(n, max_bw, max_bh);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "curve_paste_u8: batch too large (%d regions of %lld x %lld tiles)", n, g.tiles_x, g.tiles_y);
    hipLaunchKernelGGL(curve_paste_u8_kernel, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), atlas, atlas_h, atlas_w, regions,
                       segs, n_segs, (int)g.tiles_x, (int)g.tiles_y, page, page_h, page_w);
    MNET_LAUNCH_CHECK("curve_paste_u8");
    return MNET_OK;
}
