/* marconet_hip_quad.h — the two entry points libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its
 * 43 entry points define and which stays as it is) for text regions that are convex quadrilaterals of a page: a gather in and a gather out.  Plain C, like
 * marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream, returns 0 or a negative MNET_E_*, message via
 * mnet_last_error().  ctypes binding: marconet_amd/_lib.py, QUAD_SYMBOLS.  The definition is the host's, byte for byte: marconet_amd/quads.py
 * (warp_crop_host, warp_paste_host); the per-pixel arithmetic both share is csrc/quad_map.h. */
#ifndef MARCONET_HIP_QUAD_H
#define MARCONET_HIP_QUAD_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gather in: ONE launch rectifies every window of every quadrilateral region of a page.  page: uint8 RGB [page_h][page_w][3] on the device; dst: a
 * ragged batch of tightly packed [h][w][3] images in one flat buffer of dst_bytes bytes — exactly the src that mnet_lq_from_u8 reads.  Pixel (i, j) of
 * crop k is, per channel, the bilinear sample (1/64-pixel positions, integer mix, indices clamped into the page: BORDER_REPLICATE) of the page at
 *   (u, v) = (X / D, Y / D),  X = (m0 x + m1 y) + m2,  Y = (m3 x + m4 y) + m5,  D = (m6 x + m7 y) + m8,  x = (c0 + i) + 0.5,  y = j + 0.5
 * with every fp64 operation rounded separately and the IEEE division; 0 where the position is invalid (D <= 0, or X, Y or D not finite).  The nine doubles
 * are the host's (quads.quad_map: rectified pixel → page pixel): nothing of the map is derived on the device.  A position on a page pixel's centre gives
 * that pixel's byte, so an integer axis-aligned box gives page[y1:y2, x1:x2] and its right-angle rotations np.rot90 of it.
 * `crops`: a DEVICE table of n descriptors, 8-byte aligned.  The launcher does not see it, so the caller passes the largest w and h of the table (max_w,
 * max_h): the grid is n x the 64 x 16 tiles of max_w x max_h, and a descriptor larger than that is written only up to it.  A descriptor is followed only if
 * w, h >= 1, c0 >= 0, offset >= 0, offset + 3 w h <= dst_bytes and its nine doubles are finite — every workgroup of the descriptor takes the same decision
 * from the same bytes; otherwise its bytes of dst are left untouched and its neighbours stand.  No table can take the kernel out of page or dst.
 * MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, page_h, page_w, n, max_w, max_h or dst_bytes < 1, or more than 2^31 - 1
 * tiles; MNET_E_ALIGN for a table that is not 8-byte aligned. */
typedef struct {
    int64_t offset;             /* byte offset of the crop's first pixel in dst (any alignment)               */
    int32_t w, h;               /* the crop's size                                                              */
    int32_t c0;                 /* the first column of this window in its region's rectified crop               */
    int32_t reserved;           /* 0                                                                            */
    double m[9];                /* rectified pixel → page pixel, row-major (quads.quad_map)                     */
} mnet_quad_crop;
int mnet_quad_crop_u8(const uint8_t* page, int32_t page_h, int32_t page_w, const mnet_quad_crop* crops, int32_t n, int32_t max_w, int32_t max_h,
                      uint8_t* dst, int64_t dst_bytes, void* stream);

/* The gather out: ONE launch pastes every region's upright foreground into its quadrilateral of the page.  atlas: uint8 RGB [atlas_h][atlas_w][3], holding
 * each region's foreground (rw x rh, what mnet_paste_u8 with feather 0 makes of a restored line) at (ax0, ay0); page: uint8 RGB [page_h][page_w][3], holding
 * the background, modified IN PLACE inside the quadrilaterals only.  For page pixel (X, Y) of the region's bounding box [bx0, bx0 + bw) x [by0, by0 + bh):
 *   (u, v) = the position of (X + 0.5, Y + 0.5) under n[9] (page pixel → foreground coordinates: quads.inverse_map of the region's map), as above;
 * the pixel is written iff the position is valid and 0 <= u < rw, 0 <= v < rh.  The SCALE of n matters: validity is the sign of its denominator, so n must
 * be scaled to be positive over the quadrilateral — the true inverse (adjugate / determinant) is, an arbitrary multiple of it need not be.  fg = the bilinear sample of the foreground rectangle at (u, v), its
 * indices clamped inside that rectangle; the byte is fg for feather = 0, else mnet_paste_u8's integer feather of fg against the byte the page holds, with the
 * weights of foreground pixel (floor u, floor v) in rw x rh.  A pixel centre that lies exactly on the shared edge of two touching quadrilaterals belongs to
 * either (its u or v is 0 or rw or rh up to one rounding); quadrilaterals whose interiors intersect give unspecified bytes inside the intersection and
 * nothing outside it.
 * `regions`: a DEVICE table of n descriptors, 8-byte aligned; max_bw, max_bh: the largest bw and bh of the table (the grid is n x the 64 x 16 tiles of
 * max_bw x max_bh).  A region is followed only if rw, rh, bw, bh >= 1, ax0, ay0, bx0, by0 >= 0, ax0 + rw <= atlas_w, ay0 + rh <= atlas_h, bx0 + bw <= page_w,
 * by0 + bh <= page_h, 0 <= feather <= 1024 and its nine doubles are finite; otherwise it keeps the background.  No table can take the kernel out of atlas or
 * page.  MNET_E_ARG / MNET_E_ALIGN as above (atlas_h, atlas_w, n, max_bw, max_bh, page_h, page_w < 1). */
typedef struct {
    int32_t ax0, ay0, rw, rh;   /* the foreground's rectangle in the atlas                                      */
    int32_t bx0, by0, bw, bh;   /* the quadrilateral's bounding box, clipped to the page                        */
    int32_t feather;            /* 0 .. 1024: width of the blend ramp in foreground pixels, 0 for none          */
    int32_t reserved;           /* 0                                                                            */
    double n[9];                /* page pixel → foreground coordinates, row-major (quads.inverse_map)           */
} mnet_quad_region;
int mnet_quad_paste_u8(const uint8_t* atlas, int32_t atlas_h, int32_t atlas_w, const mnet_quad_region* regions, int32_t n, int32_t max_bw, int32_t max_bh,
                       uint8_t* page, int32_t page_h, int32_t page_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_QUAD_H */
