/* marconet_hip_mixed.h — the entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its entry
 * points define and which stays as it is) for a page that MIXES kinds of text region — lines and column cells, quadrilaterals, curved strips — which may
 * overlap one another: one launch pastes every region of the page in the caller's order (painter's order, as marconet_hip_ordered.h states it for cells).
 * Plain C, like marconet_hip.h; same rules — the caller owns every buffer, a call only enqueues work on the given stream, returns 0 or a negative
 * MNET_E_*, message via mnet_last_error().  ctypes binding: marconet_amd/_lib.py, MIXED_SYMBOLS.  The definition is the host's, byte for byte:
 * marconet_amd/regions.py (compose_regions_host). */
#ifndef MARCONET_HIP_MIXED_H
#define MARCONET_HIP_MIXED_H

#include "marconet_hip_ordered.h"
#include "marconet_hip_quad.h"
#include "marconet_hip_curve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MNET_ITEM_CELL 0
#define MNET_ITEM_QUAD 1
#define MNET_ITEM_CURVE 2

/* One thing to paste: entry `index` of the table of its `kind`.  The rectangle is what the HOST bins by (its field names are those pages.bin_tiles reads):
 * the cell's rectangle, or the region's bounding box clipped to the page.  The kernel itself decides by the descriptor's own rectangle. */
typedef struct {
    int32_t kind;               /* 0: cells[index], 1: quads[index], 2: curves[index]                            */
    int32_t index;
    int32_t x0, y0, rw, rh;     /* the item's rectangle in the page                                             */
} mnet_page_item;               /* 24 bytes */

/* lines / page as mnet_paste_ordered_u8 takes them.  atlas: uint8 RGB [atlas_h][atlas_w][3], the upright foregrounds of ALL quadrilateral and curved
 * regions (what ONE mnet_paste_u8 launch with feather 0 makes of their lines), as mnet_quad_paste_u8 and mnet_curve_paste_u8 read it.  Four DEVICE tables,
 * 8-byte aligned, each of which may be absent (NULL) with count 0: cells (a plain region is a cell, see marconet_hip_ordered.h), quads, curves with their
 * segs.  `items`: a DEVICE table of n_items records, 4-byte aligned; a column's cells are consecutive items.  spans / order: over the ITEMS, exactly as
 * mnet_paste_ordered_u8's are over cells — one span per 64 x 16 tile of the page, row-major from the page's origin, and int32 indices into `items`.
 * Tile t keeps its pixels in registers, composites the items order[first .. first + count) in that sequence — a cell by mnet_column_paste_u8's
 * arithmetic, a quadrilateral by mnet_quad_paste_u8's, a curved region by mnet_curve_paste_u8's (its segments tried in order, the first claim wins), each
 * blending into what the pixel holds at that moment — and stores, once, exactly the pixels some followed item claimed.  One workgroup owns a tile and one
 * thread does all blends of a pixel, so the order is defined.
 * Bounds and skipping.  No table can take the kernel out of any buffer.  Skipped, each on its own, while the neighbours in the sequence stand: a span that
 * cannot be followed (first < 0, count < 0 or first + count > n_order: the tile keeps its pixels); an entry outside [0, n_items); a kind outside 0..2; an
 * index outside its kind's table; a descriptor that fails its kind's own list (mnet_column_paste_u8's, mnet_quad_paste_u8's, mnet_curve_paste_u8's with
 * its segments'); an item listed in a tile that its descriptor's rectangle does not touch.
 * MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null page, items, spans or order; a null table, lines or atlas where the count that
 * reads it is nonzero (lines: n_cells; atlas: n_quads + n_curves; segs: n_curves); a negative count; n_items, n_order, page_h or page_w < 1; n_lines, rows
 * or line_w < 1 with cells; atlas_h or atlas_w < 1 with quads or curves; n_segs < 1 with curves; 2^24 tiles or more; n_spans other than the page's tile
 * count.  MNET_E_ALIGN for cells, quads, curves or segs that are not 8-byte aligned, items, spans or order not 4-byte aligned. */
int mnet_paste_mixed_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const uint8_t* atlas, int32_t atlas_h, int32_t atlas_w,
                        const mnet_column_paste* cells, int32_t n_cells, const mnet_quad_region* quads, int32_t n_quads,
                        const mnet_curve_region* curves, int32_t n_curves, const mnet_curve_seg* segs, int32_t n_segs, const mnet_page_item* items,
                        int32_t n_items, const mnet_tile_span* spans, int32_t n_spans, const int32_t* order, int32_t n_order, uint8_t* page,
                        int32_t page_h, int32_t page_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_MIXED_H */
