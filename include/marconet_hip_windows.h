/* marconet_hip_windows.h — the entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its entry
 * points define and which stays as it is) for the encoder's input taken straight from WINDOWS of images that are on the device already: a window is a
 * view — a first byte, a row pitch and a size — so overlapping windows of a line, and windows of a page that is uploaded anyway, cost no second copy of
 * their pixels.  Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream, returns 0 or a
 * negative MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, WINDOW_SYMBOLS.  The definition is mnet_lq_from_u8's, bit for
 * bit, of the window's pixels copied out tightly (marconet_amd/lq_io.py::lq_from_image). */
#ifndef MARCONET_HIP_WINDOWS_H
#define MARCONET_HIP_WINDOWS_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One window: h rows of w RGB pixels whose first byte is src[offset] and whose rows lie `pitch` bytes apart (the bytes per row of the image the window
 * lies in; 3 w for a tightly packed image of its own).  dw, scale: as in mnet_lq_image — the window's width at height dst_h and the sampling step. */
typedef struct {
    int64_t offset;             /* byte of the window's first pixel in src                        */
    int32_t pitch;              /* bytes between two rows of the window                           */
    int32_t h, w;               /* the window's size in source pixels                             */
    int32_t dw;                 /* its width in the output, min(max(dw, 0), canvas_w) columns     */
    double  scale;              /* the sampling step, 1.0 / (dst_h / h) as the host computes it   */
} mnet_lq_window;

/* src: uint8 [src_bytes] on the device; windows: a DEVICE table of n descriptors, 8-byte aligned; dst: fp32 [n][3][dst_h][canvas_w], every element of
 * which is written (form: MNET_LQ_FORM_F32_NCHW, the only one).  Window k's output is mnet_lq_from_u8's for the image {0, h, w, dw, scale} over the
 * window's pixels copied out tightly: BORDER_REPLICATE clamps into the WINDOW, not into the image around it; columns >= dw hold the fill (-1).
 * One launch for all windows, tiled as mnet_lq_from_u8 is.  A descriptor with h < 1, w < 1, pitch < 3 w, a negative offset, or a last row that ends
 * beyond src_bytes (offset + (h - 1) pitch + 3 w > src_bytes, in 64 bits) is written as fill: no table can take the kernel out of src or dst.
 * MNET_E_ARG (nothing enqueued) for a null pointer, n, dst_h, canvas_w or src_bytes < 1, another form, or more than 2^31 - 1 tiles;
 * MNET_E_ALIGN for a table that is not 8-byte aligned or a dst that is not 4-byte aligned. */
int mnet_lq_windows_u8(const uint8_t* src, int64_t src_bytes, const mnet_lq_window* windows, int32_t n, int32_t dst_h, int32_t canvas_w, void* dst,
                       int32_t form, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_WINDOWS_H */
