/* marconet_hip_ordered.h — the entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its entry
 * points define and which stays as it is) for a page whose text regions may OVERLAP: one launch pastes every region and every column cell of the page in
 * the caller's order (painter's order: a later cell is blended, under its own feather ramp, into what the page holds at that moment, earlier cells
 * included).  Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream, returns 0 or a
 * negative MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, ORDERED_SYMBOLS.  The definition is the host's, byte for byte:
 * marconet_amd/pages.py (its head states the order; compose_host, columns.compose_columns_host with overlap="order"). */
#ifndef MARCONET_HIP_ORDERED_H
#define MARCONET_HIP_ORDERED_H

#include "marconet_hip_columns.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lines / page as mnet_paste_u8 takes them (uint8 BGR [n_lines][rows][line_w][3]; uint8 RGB [page_h][page_w][3] holding the background, modified IN PLACE
 * at the thread's own pixel only).  `cells`: a DEVICE table of n_cells mnet_column_paste descriptors, 8-byte aligned; a plain region (mnet_paste_region) is
 * the cell whose slice starts at column 0 and whose feather rectangle is its own (src_x0 = 0, fx0 = x0, fy0 = y0, fw = rw, fh = rh), so one table holds
 * lines and column cells together.  A cell's arithmetic is mnet_column_paste_u8's.
 * The workgroups belong to the PAGE's 64 x 16 tiles, counted from the page's origin, row-major: tile t covers columns [64 (t % tx), +64) and rows
 * [16 (t / tx), +16), tx = ceil(page_w / 64).  `spans`: a DEVICE array of one record per tile, n_spans = ceil(page_w / 64) * ceil(page_h / 16) of them,
 * 4-byte aligned; `order`: a DEVICE array of n_order int32 indices into `cells`, 4-byte aligned.  Tile t keeps its pixels in registers, composites the
 * cells order[first .. first + count) in that sequence and stores, once, exactly the pixels that at least one followed cell covered.  One workgroup owns
 * a tile and the table cannot name a tile twice, so no two workgroups touch one pixel; one thread does all blends of a pixel, so the order is defined.
 * Followed: a span with first >= 0, count >= 0 and first + count <= n_order (the sum in 64 bits); an entry in [0, n_cells); a cell that passes
 * mnet_column_paste_u8's checks and whose rectangle touches the tile.  Skipped, each on its own, the neighbours in the sequence standing: an entry outside
 * [0, n_cells), a cell that fails those checks, a cell listed in a tile it does not touch.  A span that cannot be followed, and a span of count 0, keep
 * the tile's background (a workgroup of count 0 returns before it loads anything).  No table can take the kernel out of lines, page, cells, spans or order.
 * MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, n_lines, rows, line_w, n_cells, n_order, page_h or page_w < 1, 2^24 tiles
 * or more (the launch's 256-thread workgroups must stay under 2^32 threads), or n_spans other than the page's tile count; MNET_E_ALIGN for cells that are not 8-byte aligned, spans or order not 4-byte aligned. */
typedef struct {
    int32_t first;              /* the tile's first entry of `order`                                            */
    int32_t count;              /* how many entries it composites, in sequence; 0: the tile keeps its pixels    */
} mnet_tile_span;
int mnet_paste_ordered_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                          const mnet_tile_span* spans, int32_t n_spans, const int32_t* order, int32_t n_order, uint8_t* page, int32_t page_h,
                          int32_t page_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_ORDERED_H */
