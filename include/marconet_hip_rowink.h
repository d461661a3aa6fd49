/* marconet_hip_rowink.h — the entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its entry
 * points define and which stays as it is) for the INK PROFILE of boxes of a page that is on the device: per row of a box the total horizontal variation
 * of its integer luma.  A vertical text column of unknown text is cut into character cells at the rows where this profile dips
 * (marconet_amd/blind_columns.py::first_cuts).  Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the
 * given stream, returns 0 or a negative MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, ROWINK_SYMBOLS.  The definition
 * is marconet_amd/blind_columns.py::row_ink, an exact integer sum: the device equals it with ==. */
#ifndef MARCONET_HIP_ROWINK_H
#define MARCONET_HIP_ROWINK_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One box: h rows of w RGB pixels whose first byte is src[offset] and whose rows lie `pitch` bytes apart — a view, as mnet_lq_window is. */
typedef struct {
    int64_t offset;             /* byte of the box's first pixel in src     */
    int32_t pitch;              /* bytes between two rows                   */
    int32_t h, w;               /* the box in pixels                        */
    int32_t out;                /* index in dst of the box's first row      */
} mnet_ink_box;                 /* 24 bytes, 8-byte aligned                 */

/* src: uint8 [src_bytes] on the device; boxes: a DEVICE table of n descriptors, 8-byte aligned; dst: int32 [dst_len] on the device.
 *     dst[out + r] = sum over x = 0 .. w - 2 of |Y(x + 1, r) - Y(x, r)|,   Y = (77 R + 150 G + 29 B + 128) >> 8       (0 for w == 1)
 * for every row r < h of every box, in ONE launch: grid (ceil(max_h / 4), n), one wave of 64 lanes per row, no atomics; dst needs no clearing and
 * an element no box owns is not touched (two boxes that own the same element race: the caller's ranges are disjoint).  Rows >= max_h of a box are not
 * computed: max_h is the largest h of the table.
 * A descriptor is followed only if h >= 1, w >= 1, w < 2^23, offset >= 0, pitch >= 3 w and its last row ends inside src
 * (offset + (h - 1) pitch + 3 w <= src_bytes, in 64 bits).  Where the source fails but [out, out + h) lies inside [0, dst_len), the rows are
 * written as -1; where that range fails (out < 0 or out + h > dst_len) nothing is written: no table can take the kernel out of src or dst.
 * MNET_E_ARG (nothing enqueued) for a null pointer, n, max_h, src_bytes or dst_len < 1, n > 65535, or a grid of more than 2^32 - 1 threads;
 * MNET_E_ALIGN for a table that is not 8-byte aligned or a dst that is not 4-byte aligned. */
int mnet_row_ink_u8(const uint8_t* src, int64_t src_bytes, const mnet_ink_box* boxes, int32_t n, int32_t max_h, int32_t* dst, int64_t dst_len,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_ROWINK_H */
