/* marconet_hip_curve.h — the two entry points libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its
 * 43 entry points define and which stays as it is) for text regions that are curved strips of a page — polygons of 2K points, a chain of K - 1 segments: a
 * gather in and a gather out.  Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream,
 * returns 0 or a negative MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, CURVE_SYMBOLS.  The definition is the host's, byte
 * for byte: marconet_amd/curves.py (warp_crop_host, warp_paste_host); the per-pixel arithmetic both share is csrc/curve_map.h. */
#ifndef MARCONET_HIP_CURVE_H
#define MARCONET_HIP_CURVE_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MNET_CURVE_MAX_SEGS 32

/* One segment of a region: a bilinear patch.  The point (u, v) of the segment's w x h rectangle (h: the height of its region's strip) lies at
 *   X = ((Ex u + Fx v) + (Gx u) v) + Ax,  Y = ((Ey u + Fy v) + (Gy u) v) + Ay
 * with every fp64 operation rounded separately.  The eight doubles are the host's (curves.segment_coeffs): nothing of the map is derived on the device but
 * the two cross products of the inverse that depend on the segment alone.  A region's segments lie one after the other in the table `segs`, their columns
 * chained: u0 of the first is 0 and u0 of the next is u0 + w. */
typedef struct {
    double c[8];                /* Ax, Ex, Fx, Gx, Ay, Ey, Fy, Gy                                               */
    int32_t u0, w;              /* the segment's first column in its region's strip, and its width (>= 1)       */
    int32_t bx0, by0, bw, bh;   /* paste: the segment's bounding box, clipped to the page (bw or bh 0: it claims
                                   nothing); 0 in a crop table                                                  */
} mnet_curve_seg;               /* 88 bytes */

/* The gather in: ONE launch rectifies every window of every curved region of a page.  page: uint8 RGB [page_h][page_w][3] on the device; dst: a ragged
 * batch of tightly packed [h][w][3] images in one flat buffer of dst_bytes bytes — exactly the src that mnet_lq_from_u8 reads.  Column i of crop k is column
 * c0 + i of its region's strip and lies in the segment s with u0_s <= c0 + i < u0_s + w_s; pixel (i, j) is, per channel, the bilinear sample (1/64-pixel
 * positions, integer mix, indices clamped into the page: BORDER_REPLICATE) of the page at the segment's (X, Y) for u = (c0 + i - u0_s) + 0.5, v = j + 0.5;
 * 0 where X or Y is not finite.  A position on a page pixel's centre gives that pixel's byte, so an integer axis-aligned box cut at integer abscissae gives
 * page[y1:y2, x1:x2]; a one-segment parallelogram gives mnet_quad_crop_u8's bytes.
 * `crops`, `segs`: DEVICE tables of n descriptors and n_segs segments, 8-byte aligned.  The launcher does not see them, so the caller passes the largest w
 * and h of the crop table (max_w, max_h): the grid is n x the 64 x 16 tiles of max_w x max_h, and a descriptor larger than that is written only up to it.
 * A descriptor is followed only if w, h >= 1, c0 >= 0, offset >= 0, offset + 3 w h <= dst_bytes, seg0 >= 0, 1 <= nseg <= 32, seg0 + nseg <= n_segs, and of
 * its segments every coefficient is finite, every w >= 1, the columns chain (u0 = 0, then u0 + w) and c0 + w <= the sum of their widths — every workgroup
 * of the descriptor takes the same decision from the same bytes; otherwise its bytes of dst are left untouched and its neighbours stand.  No table can take
 * the kernel out of page, dst or segs.
 * MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, page_h, page_w, n, n_segs, max_w, max_h or dst_bytes < 1, or more than
 * 2^31 - 1 tiles; MNET_E_ALIGN for a table that is not 8-byte aligned. */
typedef struct {
    int64_t offset;             /* byte offset of the crop's first pixel in dst (any alignment)                 */
    int32_t w, h;               /* the crop's size                                                              */
    int32_t c0;                 /* the first column of this window in its region's strip                        */
    int32_t seg0, nseg;         /* the region's segments: segs[seg0 .. seg0 + nseg)                             */
    int32_t reserved;           /* 0                                                                            */
} mnet_curve_crop;              /* 32 bytes */
int mnet_curve_crop_u8(const uint8_t* page, int32_t page_h, int32_t page_w, const mnet_curve_crop* crops, int32_t n, const mnet_curve_seg* segs,
                       int32_t n_segs, int32_t max_w, int32_t max_h, uint8_t* dst, int64_t dst_bytes, void* stream);

/* The gather out: ONE launch pastes every region's upright foreground back along its curve.  atlas: uint8 RGB [atlas_h][atlas_w][3], holding each region's
 * foreground (rw x rh, what mnet_paste_u8 with feather 0 makes of a restored line) at (ax0, ay0); page: uint8 RGB [page_h][page_w][3], holding the
 * background, modified IN PLACE inside the regions only.  For page pixel (X, Y) of the region's bounding box the region's segments are tried in order by
 * ONE thread; segment s claims the pixel iff the pixel lies in the segment's box and the inverse of its patch at p = (X + 0.5, Y + 0.5) — with q = p - A,
 * cross(a, b) = ax by - ay bx:
 *   a2 = cross(F, G), a1 = cross(F, E) - cross(q, G), a0 = -cross(q, E), disc = a1 a1 - (4 a2) a0, r = sqrt(disc),
 *   v = a0 / (0.5 (r - a1)) where a1 <= 0, (-0.5 (a1 + r)) / a2 where a1 > 0;  d = E + v G;  u = (qx - v Fx) / dx where |dx| >= |dy|, else (qy - v Fy) / dy
 * (every operation rounded separately, IEEE division and square root) — has disc >= 0, u and v finite, 0 <= u < w_s and 0 <= v < rh.  The first claim wins;
 * a pixel no segment claims keeps the background.  fg = the bilinear sample of the foreground rectangle at (u0_s + u, v), its indices clamped inside the
 * WHOLE rectangle (the interpolation runs across seams); the byte is fg for feather = 0, else mnet_paste_u8's integer feather of fg against the byte the
 * page holds, with the weights of foreground pixel (u0_s + floor u, floor v) in rw x rh: the ramp follows the curved outline.  Regions whose segments
 * intersect give unspecified bytes inside the intersection and nothing outside it.
 * `regions`, `segs`: DEVICE tables, 8-byte aligned; max_bw, max_bh: the largest bw and bh of the region table (the grid is n x the 64 x 16 tiles of
 * max_bw x max_bh).  A region is followed only if mnet_quad_paste_u8's conditions hold (rw, rh, bw, bh >= 1, ax0, ay0, bx0, by0 >= 0, the foreground inside
 * the atlas, the box inside the page, 0 <= feather <= 1024), seg0 >= 0, 1 <= nseg <= 32, seg0 + nseg <= n_segs, and of its segments every coefficient is
 * finite, every w >= 1, the columns chain from 0, their widths sum to rw, and every segment's box has bw, bh >= 0 and lies inside the region's box;
 * otherwise it keeps the background.  No table can take the kernel out of atlas, page or segs.  MNET_E_ARG / MNET_E_ALIGN as above (atlas_h, atlas_w, n,
 * n_segs, max_bw, max_bh, page_h, page_w < 1). */
typedef struct {
    int32_t ax0, ay0, rw, rh;   /* the foreground's rectangle in the atlas                                      */
    int32_t bx0, by0, bw, bh;   /* the region's bounding box, clipped to the page                               */
    int32_t feather;            /* 0 .. 1024: width of the blend ramp in foreground pixels, 0 for none          */
    int32_t seg0, nseg;         /* the region's segments: segs[seg0 .. seg0 + nseg)                             */
    int32_t reserved;           /* 0                                                                            */
} mnet_curve_region;            /* 48 bytes */
int mnet_curve_paste_u8(const uint8_t* atlas, int32_t atlas_h, int32_t atlas_w, const mnet_curve_region* regions, int32_t n, const mnet_curve_seg* segs,
                        int32_t n_segs, int32_t max_bw, int32_t max_bh, uint8_t* page, int32_t page_h, int32_t page_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_CURVE_H */
