/* marconet_hip_columns.h — the two entry points libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its
 * entry points define and which stays as it is) for vertical text columns of a page, made of upright stacked characters: a gather that lays a column's
 * character cells side by side as the horizontal strip the encoder expects, and a paste that brings each restored character back to its own cell.  Plain
 * C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream, returns 0 or a negative MNET_E_*,
 * message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, COLUMN_SYMBOLS.  The definition is the host's, byte for byte:
 * marconet_amd/columns.py (virtual_strip, paste_column_host). */
#ifndef MARCONET_HIP_COLUMNS_H
#define MARCONET_HIP_COLUMNS_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gather: ONE launch makes every window of every column of a page.  page: uint8 RGB [page_h][page_w][3] on the device; dst: a ragged batch of tightly
 * packed window images [dst_h][win_w][3] in one flat buffer of dst_bytes bytes — exactly the src that mnet_lq_from_u8 reads.  A descriptor is one character
 * cell of one window: columns [dx, dx + dw) of the window's image become the 8-bit INTER_CUBIC resize (mnet_lq_from_u8's arithmetic: lq_taps.h's taps, both
 * passes in integers, one (v + 2^21) >> 22 and a clip) of the page rectangle [sy, sy + sh) x [sx, sx + sw) to dw x dst_h, with the sampling steps scale_x =
 * 1.0 / (dw / sw) and scale_y = 1.0 / (dst_h / sh) as the host's doubles.  Every tap index is clamped into the CELL (BORDER_REPLICATE at the cell's border,
 * not the page's): the cells of a column do not bleed into one another.
 * `cells`: a DEVICE table of n_cells descriptors, 8-byte aligned.  The launcher does not see it, so the caller passes the largest dw of the table (max_dw):
 * the grid is n_cells x the 64 x 16 tiles of max_dw x dst_h.  A descriptor is followed only if sw, sh >= 1, sx, sy >= 0, sx + sw <= page_w, sy + sh <= page_h,
 * 1 <= dw <= max_dw, dx >= 0, dx + dw <= win_w, offset >= 0, offset + 3 dst_h win_w <= dst_bytes and both steps are finite — every workgroup of the
 * descriptor takes the same decision from the same bytes; otherwise its bytes of dst are left untouched and its neighbours stand.  The bytes between the
 * images, and the columns of an image no descriptor names, are never written.  No table can take the kernel out of page or dst.
 * MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, page_h, page_w, n_cells, max_dw, dst_h or dst_bytes < 1, or more than
 * 2^31 - 1 tiles; MNET_E_ALIGN for a table that is not 8-byte aligned. */
typedef struct {
    int64_t offset;             /* byte offset of the window's image in dst (any alignment)                     */
    int32_t win_w;              /* the window's width: the image is [dst_h][win_w][3]                           */
    int32_t dx, dw;             /* the cell's columns [dx, dx + dw) in that image                               */
    int32_t sx, sy, sw, sh;     /* the cell's rectangle in the page                                             */
    int32_t reserved;           /* 0                                                                            */
    double scale_x, scale_y;    /* 1.0 / (dw / sw), 1.0 / (dst_h / sh)                                          */
} mnet_column_cell;
int mnet_column_gather_u8(const uint8_t* page, int32_t page_h, int32_t page_w, const mnet_column_cell* cells, int32_t n_cells, int32_t max_dw, int32_t dst_h,
                          uint8_t* dst, int64_t dst_bytes, void* stream);

/* The paste: ONE launch brings every restored character of every column back to its cell of the enlarged page.  lines / page as mnet_paste_u8 takes them
 * (uint8 BGR [n_lines][rows][line_w][3]; uint8 RGB [page_h][page_w][3] holding the background, modified IN PLACE at the thread's own pixel only).  A
 * descriptor is one cell: mnet_paste_u8's region whose line is the slice [src_x0, src_x0 + src_w) of line line_index — the k x k box reduction (ragged at
 * the SLICE's right edge) and every tap clamp stay inside that slice — and whose feather is taken relative to the rectangle (fx0, fy0, fw, fh), the whole
 * column's: the ramp follows the column's outer edge and there is none between cells.  scale_x = 1.0 / (rw / ceil(src_w / k)), scale_y = 1.0 / (rh /
 * (rows / k)).
 * `cells`: a DEVICE table of n_cells descriptors, 8-byte aligned; the grid is n_cells x the 64 x 16 tiles of the page.  A descriptor is followed only if it
 * passes mnet_paste_u8's checks (0 <= line_index < n_lines, src_w >= 1, rw, rh >= 1, x0, y0 >= 0, x0 + rw <= page_w, y0 + rh <= page_h, 0 <= feather <=
 * 1024, k in {1, 2, 4, 8} dividing rows) and src_x0 >= 0, src_x0 + src_w <= line_w, fw, fh >= 1, fx0 <= x0, fy0 <= y0, x0 + rw <= fx0 + fw, y0 + rh <=
 * fy0 + fh; otherwise it keeps the background.  No table can take the kernel out of lines or page.  MNET_E_ARG / MNET_E_ALIGN as mnet_paste_u8. */
typedef struct {
    int32_t line_index;         /* which line of `lines`                                                        */
    int32_t src_x0, src_w;      /* the cell's columns [src_x0, src_x0 + src_w) of that line                     */
    int32_t x0, y0, rw, rh;     /* the cell's rectangle in the page                                             */
    int32_t feather;            /* 0 .. 1024: width of the blend ramp in page pixels, 0 for none                */
    int32_t k;                  /* the box reduction: 1, 2, 4 or 8                                              */
    int32_t fx0, fy0, fw, fh;   /* the feather rectangle: the whole column's rectangle in the page              */
    int32_t reserved;           /* 0                                                                            */
    double scale_x, scale_y;    /* the cubic's sampling steps over the box-reduced slice                        */
} mnet_column_paste;
int mnet_column_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                         uint8_t* page, int32_t page_h, int32_t page_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_COLUMNS_H */
