/* marconet_hip_skewink.h — the entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its entry
 * points define and which stays as it is) for BOTH INK PROFILES of boxes of a SHEARED FRAME of a page that is on the device: what
 * marconet_hip_boxink.h's entry point computes for boxes of the page, in the coordinates a page scanned skewed is upright in.  The skew of a page is
 * found from the row profiles of the whole page at many slopes, its text lines by cutting frame boxes at the blank runs of their profiles
 * (marconet_amd/skew.py).  Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream,
 * returns 0 or a negative MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, SKEWINK_SYMBOLS.  The definition is
 * marconet_amd/skew.py::frame_ink, exact integer sums: the device equals it with ==, whatever the order of its additions. */
#ifndef MARCONET_HIP_SKEWINK_H
#define MARCONET_HIP_SKEWINK_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One record: a frame box at a slope, where its two profiles go, and the rectangle of the page whose pixels are tried for it. */
typedef struct {
    int32_t c1, r1, c2, r2;     /* frame box, half-open; coordinates may be negative            */
    int32_t slope;              /* Q16, |slope| <= 8192                                         */
    int32_t out_rows;           /* index in dst of the row profile's first entry; -1: not wanted */
    int32_t out_cols;           /* index in dst of the column profile's first one; -1: not wanted */
    int32_t px1, py1, px2, py2; /* page rectangle to scan, half-open                             */
    int32_t reserved;           /* 0                                                             */
} mnet_skew_box;                /* 48 bytes; the table is 8-byte aligned                         */

/* page: uint8 RGB [H, W, 3], contiguous, on the device, 1 <= H, W < 2^17; boxes: a DEVICE table of n records, 8-byte aligned; dst: int32 [dst_len]
 * on the device.  With sh(v) = floor((v slope + 32768) / 65536) — the product fits 32 bits for v < 2^17 — page pixel (x, r) has the frame
 * coordinates r' = r - sh(x), c' = x + sh(r).  With
 *     Y = (77 R + 150 G + 29 B + 128) >> 8,   d(x, r) = |Y(x + 1, r) - Y(x, r)|,   e(x, r) = d(x, r) if d(x, r) >= floor, else 0
 * every record ADDS, in ONE launch, for every pair (x, r) with px1 <= x < px2, x <= W - 2, py1 <= r < py2, r1 <= r' < r2 and c1 <= c', c' + 1 < c2
 *     dst[out_rows + (r' - r1)] += e(x, r)      (out_rows != -1)
 *     dst[out_cols + (c' - c1)] += e(x, r)      (out_cols != -1; entry c2 - c1 - 1 gets nothing: a pair is filed under its left pixel)
 * floor: 0 .. 255; 0 and 1 are the same.  A scan rectangle that holds every pixel whose frame coordinates lie in the box (skew.py::scan_rect, or the
 * whole page) gives the box's full profiles; a smaller one gives the sums over its own pixels.  A bin holds at most one pair per column (or per row)
 * of the page: it stays below 2^25.  THE CALLER ZEROES dst (or fills it with what the profiles are to be added to) before the call: the kernel only
 * adds, by integer atomics, and an element no record owns is not touched.  Two records may read the same pixels; their output ranges are the caller's
 * and disjoint.  Grid (ceil(max_w / 256), ceil(max_h / 32), n): what lies at x >= px1 + 256 ceil(max_w / 256) or r >= py1 + 32 ceil(max_h / 32) of a
 * scan rectangle is not tried: max_h, max_w are the largest scan rectangle of the table (at least 1).
 * A record is followed only if its box is not empty (c1 < c2, r1 < r2), |slope| <= 8192, its scan rectangle lies inside the page (0 <= px1 <= px2 <= W,
 * 0 <= py1 <= py2 <= H; an empty one adds nothing) and every WANTED output range — [out_rows, out_rows + r2 - r1), [out_cols, out_cols + c2 - c1) —
 * lies inside [0, dst_len) (an index below -1 fails).  A record that fails SETS the entries of its wanted ranges that do lie inside [0, dst_len) to -1
 * (an empty box has none), each by a single writer, and writes nothing else: no table can take the kernel out of page or dst.
 * MNET_E_ARG (nothing enqueued) for a null pointer, H or W outside [1, 2^17), n or dst_len < 1, max_h or max_w outside [1, 2^17), n > 65535, floor
 * outside 0 .. 255, or a grid of more than 65535 row tiles or 2^32 - 1 threads; MNET_E_ALIGN for a table that is not 8-byte aligned or a dst that
 * is not 4-byte aligned. */
int mnet_skew_ink_u8(const uint8_t* page, int32_t H, int32_t W, const mnet_skew_box* boxes, int32_t n, int32_t max_h, int32_t max_w, int32_t floor,
                     int32_t* dst, int64_t dst_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_SKEWINK_H */
