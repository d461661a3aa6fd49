/* marconet_hip_boxink.h — the entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its entry
 * points define and which stays as it is) for BOTH INK PROFILES of boxes of a page that is on the device: per row and per column of a box the total
 * horizontal variation of its integer luma above a noise floor.  A page's text lines are found by cutting boxes at the blank runs of these profiles
 * (marconet_amd/layout.py::xy_cut).  Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given
 * stream, returns 0 or a negative MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, BOXINK_SYMBOLS.  The definition is
 * marconet_amd/layout.py::box_ink, exact integer sums: the device equals it with ==, whatever the order of its additions. */
#ifndef MARCONET_HIP_BOXINK_H
#define MARCONET_HIP_BOXINK_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One box: h rows of w RGB pixels whose first byte is src[offset] and whose rows lie `pitch` bytes apart — a view, as mnet_ink_box is. */
typedef struct {
    int64_t offset;             /* byte of the box's first pixel in src           */
    int32_t pitch;              /* bytes between two rows                         */
    int32_t h, w;               /* the box in pixels                              */
    int32_t out_rows;           /* index in dst of the row profile's first entry  */
    int32_t out_cols;           /* index in dst of the column profile's first one */
    int32_t reserved;           /* 0                                              */
} mnet_ink_box2;                /* 32 bytes, 8-byte aligned                       */

/* src: uint8 [src_bytes] on the device; boxes: a DEVICE table of n descriptors, 8-byte aligned; dst: int32 [dst_len] on the device.  With
 *     Y = (77 R + 150 G + 29 B + 128) >> 8,   d(x, r) = |Y(x + 1, r) - Y(x, r)|,   e(x, r) = d(x, r) if d(x, r) >= floor, else 0
 * every box ADDS, in ONE launch,
 *     dst[out_rows + r] += sum over x = 0 .. w - 2 of e(x, r)      for r < h,
 *     dst[out_cols + x] += sum over r = 0 .. h - 1 of e(x, r)      for x <= w - 2     (entry w - 1 gets nothing: the column profile's last entry is 0)
 * floor: 0 .. 255; 0 and 1 are the same (a difference of 0 adds nothing).  THE CALLER ZEROES dst (or fills it with what the profiles are to be
 * added to) before the call: the kernel only adds, by integer atomics, and an element no box owns is not touched.  Two boxes may read the same
 * pixels; their output ranges are the caller's and disjoint.  Grid (ceil(max_w / 256), ceil(max_h / 32), n): what lies at x >= 256 ceil(max_w / 256)
 * or r >= 32 ceil(max_h / 32) of a box is not computed: max_h, max_w are the largest h, w of the table.
 * A descriptor is followed only if 1 <= h, w < 2^23 (the sums then stay below 2^31), offset >= 0, pitch >= 3 w and its last row ends inside src
 * (offset + (h - 1) pitch + 3 w <= src_bytes, in 64 bits).  Where the source fails but both [out_rows, out_rows + h) and [out_cols, out_cols + w)
 * lie inside [0, dst_len), their entries are SET to -1 (those the grid covers); where either range fails, or h or w is below 1, the box writes
 * nothing: no table can take the kernel out of src or dst.
 * MNET_E_ARG (nothing enqueued) for a null pointer, n, src_bytes or dst_len < 1, max_h or max_w outside [1, 2^23), n > 65535, floor outside
 * 0 .. 255, or a grid of more than 65535 row tiles or 2^32 - 1 threads; MNET_E_ALIGN for a table that is not 8-byte aligned or a dst that is
 * not 4-byte aligned. */
int mnet_box_ink_u8(const uint8_t* src, int64_t src_bytes, const mnet_ink_box2* boxes, int32_t n, int32_t max_h, int32_t max_w, int32_t floor,
                    int32_t* dst, int64_t dst_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_BOXINK_H */
