// The page-tile compositor: ONE kernel, paste_tiles_kernel, in two instantiations.  <false> pastes regions of EVERY kind (mnet_paste_mixed_u8,
// include/marconet_hip_mixed.h): lines and column cells, quadrilaterals and curved strips, overlapping one another, in the caller's order in ONE
// launch; the definition is the host's, byte for byte — marconet_amd/regions.py::compose_regions_host: pages.paste_host, columns.paste_column_host,
// quads.warp_paste_host and curves.warp_paste_host applied one after another in list order.  <true> pastes cells alone (mnet_paste_ordered_u8,
// include/marconet_hip_ordered.h: pages.paste_host / columns.paste_column_host in the table's order): an order entry is a cell's index, there is no
// item table, and the other kinds' branches and the curve's LDS are compiled out.
//
// The workgroup owns tile blockIdx.x of the PAGE (64 x 16, row-major from the page's origin), keeps the tile's pixels in registers, walks the items
// order[first .. first + count) of its span in sequence and stores, once, exactly the pixels some followed item claimed: the work follows the
// covered area.  The item's kind is uniform over the workgroup; per kind the per-pixel arithmetic is the per-descriptor kernels' own, stated once: a
// cell by cell_foreground / cell_blend (cell_paste.h), a quadrilateral by quad_paste_pixel, a curved region by curve_paste_pixel (warp_paste.h) —
// each blending into the register pixel.  -ffp-contract=off (build.sh), for the reasons of lq_taps.h, quad_map.h and curve_map.h.
// A cell's tile origin counted from the cell's corner may be negative or beyond the rectangle: lq_cubic_taps clamps every index for any coordinate,
// and those lanes' taps are not used.
// LDS: the cell's taps (PtTaps, 2560 bytes) and, in <false>, the curve's segments (CurveSegL[32], 3584 bytes) side by side; ONE barrier before either
// stage is overwritten, so that every lane has finished reading the previous item's; pt_stage_taps' own barrier, or the curve's vote, after.
// Every condition that skips a span or an item is uniform over the workgroup, and after the first barrier no lane returns before the last: a lane
// outside an item is predicated (the per-descriptor kernels let such lanes return).
// Bounds: a descriptor is followed only if it passes its kind's list — cell_followed, quad_region_followed, curve_region_followed with curve_stage
// and curve_seg_in_region over its segments, voted — so every index the shared bodies form lies where their own headers say; an order entry is used
// only inside [0, n_items) (<true>: [0, n_cells)), an item's index only inside its kind's table; the page is read and written at the thread's own
// pixel only, inside the page: a claimed pixel lies inside a followed descriptor's rectangle, which lies inside the page.
#include "common.h"
#include "../../include/marconet_hip_ordered.h"
#include "../../include/marconet_hip_mixed.h"
#include "cell_paste.h"
#include "warp_paste.h"

namespace {

static_assert(sizeof(mnet_page_item) == 24 && sizeof(mnet_tile_span) == 8, "descriptor layout");
static_assert(CURVE_MAX_SEGS == MNET_CURVE_MAX_SEGS, "curve_map.h and marconet_hip_curve.h disagree");

struct MixedArgs {
    const unsigned char* lines; int n_lines, rows, line_w;
    const unsigned char* atlas; int atlas_h, atlas_w;
    const mnet_column_paste* cells; int n_cells;
    const mnet_quad_region* quads; int n_quads;
    const mnet_curve_region* curves; int n_curves;
    const mnet_curve_seg* segs; int n_segs;
    const mnet_page_item* items; int n_items;
    const mnet_tile_span* spans; const int* order; int n_order;
    int tiles_x; unsigned char* page; int page_h, page_w;
};

// a rectangle inside the page (so its ends fit an int) shares a pixel with the tile at (X0, Y0)
__device__ __forceinline__ bool touches_tile(int x0, int y0, int w, int h, int X0, int Y0) {
    return !(x0 - X0 >= PT_TX || x0 + w <= X0 || y0 - Y0 >= PT_TY || y0 + h <= Y0);
}

template <bool CELLS_ONLY>
__global__ void __launch_bounds__(256) paste_tiles_kernel(const MixedArgs A) {
    __shared__ PtTaps s;
    __shared__ CurveSegL S[CURVE_MAX_SEGS];                                       // <true> never names it: no LDS is allotted to it there
    const mnet_tile_span sp = A.spans[blockIdx.x];                                // the launcher has checked: one record per workgroup
    if (sp.count <= 0 || sp.first < 0 || (long long)sp.first + sp.count > A.n_order) return;     // uniform; nothing loaded, no barrier met
    const int page_h = A.page_h, page_w = A.page_w;
    const int X0 = (int)(blockIdx.x % (unsigned)A.tiles_x) * PT_TX, Y0 = (int)(blockIdx.x / (unsigned)A.tiles_x) * PT_TY;
    const int t = (int)threadIdx.x, tx = t & (PT_TX - 1), ty = t / PT_TX;
    const bool in_x = tx < page_w - X0;                                           // X0 + tx itself could pass 2^31 in a page's last tile
    unsigned char pix[PT_TY / 4][3] = {};
    unsigned covered = 0u;                                                        // bit i: row ty + 4 i of the tile was claimed by a followed item
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        if (in_x && ty + 4 * i < page_h - Y0) {
            const unsigned char* d = A.page + ((size_t)(Y0 + ty + 4 * i) * page_w + (size_t)(X0 + tx)) * 3;
            pix[i][0] = d[0]; pix[i][1] = d[1]; pix[i][2] = d[2];
        }
    }
    for (int e = 0; e < sp.count; ++e) {
        int kind = MNET_ITEM_CELL, c = A.order[sp.first + e];                     // <true>: the order lists cells
        if constexpr (!CELLS_ONLY) {
            if (c < 0 || c >= A.n_items) continue;                                // uniform, as every `continue` of this loop
            kind = A.items[c].kind;
            c = A.items[c].index;
        }
        if (kind == MNET_ITEM_CELL) {
            if (c < 0 || c >= A.n_cells) continue;
            const mnet_column_paste R = A.cells[c];
            if (!cell_followed(R, A.n_lines, A.rows, A.line_w, page_h, page_w) || !touches_tile(R.x0, R.y0, R.rw, R.rh, X0, Y0)) continue;
            const int k = R.k;
            const PtTile T = {X0 - R.x0, Y0 - R.y0, c};
            __syncthreads();                                                      // every lane has read the last cell's taps
            pt_stage_taps(s, T, (R.src_w + k - 1) / k, R.scale_x, A.rows / k, R.scale_y, 0, 1, 0);
            const int u = T.x0 + tx;
            if (in_x && u >= 0 && u < R.rw) {
                const CellView V = cell_view(R, A.lines, A.rows, A.line_w);
                const unsigned fa = V.F ? page_feather_axis(V.fu0 + (unsigned)u, (unsigned)R.fw, V.F) : 0u;
                const PtI4 ci = s.ci[tx], ct = s.ct[tx];
#pragma unroll
                for (int i = 0; i < PT_TY / 4; ++i) {
                    const int r = ty + 4 * i, v = T.y0 + r;
                    if (v >= 0 && v < R.rh) {
                        int acc[3];
                        cell_foreground(V.line, V.row_bytes, k, R.src_w, ci, ct, s.ri[r], s.rt[r], acc);
                        const unsigned fb = V.F ? page_feather_axis(V.fv0 + (unsigned)v, (unsigned)R.fh, V.F) : 0u;
                        cell_blend(pix[i], acc, fa, fb, V.F);
                        covered |= 1u << i;
                    }
                }
            }
        }
        if constexpr (!CELLS_ONLY) {
            const size_t atlas_row = (size_t)A.atlas_w * 3;
            if (kind == MNET_ITEM_QUAD) {
                if (c < 0 || c >= A.n_quads) continue;
                const mnet_quad_region R = A.quads[c];
                if (!quad_region_followed(R, A.atlas_h, A.atlas_w, page_h, page_w) || !touches_tile(R.bx0, R.by0, R.bw, R.bh, X0, Y0)) continue;
                const int i0 = X0 - R.bx0 + tx;                                   // the pixel's column in the bounding box
                if (in_x && i0 >= 0 && i0 < R.bw) {
                    const double x = LQ_DADD((double)(X0 + tx), 0.5);
                    const unsigned char* fg0 = A.atlas + ((size_t)R.ay0 * A.atlas_w + (size_t)R.ax0) * 3;
#pragma unroll 1
                    for (int i = 0; i < PT_TY / 4; ++i) {                         // the rows one after the other, as for a curve: 4 waves, not 3
                        const int Y = Y0 + ty + 4 * i, j = Y - R.by0;
                        if (j < 0 || j >= R.bh) continue;
                        unsigned char d[3] = {0, 0, 0};
#pragma unroll
                        for (int q = 0; q < PT_TY / 4; ++q)                       // a register array is indexed by constants only
                            if (q == i) { d[0] = pix[q][0]; d[1] = pix[q][1]; d[2] = pix[q][2]; }
                        if (quad_paste_pixel(R.n, R.rw, R.rh, (unsigned)R.feather, fg0, atlas_row, x, LQ_DADD((double)Y, 0.5), d)) {
#pragma unroll
                            for (int q = 0; q < PT_TY / 4; ++q)
                                if (q == i) { pix[q][0] = d[0]; pix[q][1] = d[1]; pix[q][2] = d[2]; }
                            covered |= 1u << i;
                        }
                    }
                }
            } else if (kind == MNET_ITEM_CURVE) {
                if (c < 0 || c >= A.n_curves) continue;
                const mnet_curve_region R = A.curves[c];
                if (!curve_region_followed(R, A.atlas_h, A.atlas_w, page_h, page_w, A.n_segs) || !touches_tile(R.bx0, R.by0, R.bw, R.bh, X0, Y0)) continue;
                const int nseg = R.nseg;
                __syncthreads();                                                  // every lane has read the last curve's segments
                bool good = true, hit = false;
                if (t < nseg) {
                    mnet_curve_seg g;
                    good = curve_stage(S, A.segs, R.seg0, t, g) && curve_seg_in_region(g, R);
                    hit = curve_seg_hits(g, X0, Y0, PT_TX, PT_TY);
                }
                if (!__syncthreads_and(good ? 1 : 0)) continue;                   // the vote is the barrier: S is visible, and the decision is uniform
                if ((long long)S[nseg - 1].u0 + S[nseg - 1].w != R.rw) continue;
                if (!__syncthreads_or(hit ? 1 : 0)) continue;                     // the tile meets no segment's box
                if (in_x) {
                    const int X = X0 + tx;
                    const double x = LQ_DADD((double)X, 0.5);
                    const unsigned char* fg0 = A.atlas + ((size_t)R.ay0 * A.atlas_w + (size_t)R.ax0) * 3;
#pragma unroll 1
                    for (int i = 0; i < PT_TY / 4; ++i) {                         // the rows one after the other: the fp64 body is stated once in the code
                        const int Y = Y0 + ty + 4 * i;
                        if (Y >= page_h) break;
                        unsigned char d[3] = {0, 0, 0};
#pragma unroll
                        for (int q = 0; q < PT_TY / 4; ++q)                       // a register array is indexed by constants only
                            if (q == i) { d[0] = pix[q][0]; d[1] = pix[q][1]; d[2] = pix[q][2]; }
                        if (curve_paste_pixel(S, nseg, R.rw, R.rh, (unsigned)R.feather, fg0, atlas_row, X, Y, x, LQ_DADD((double)Y, 0.5), d)) {
#pragma unroll
                            for (int q = 0; q < PT_TY / 4; ++q)
                                if (q == i) { pix[q][0] = d[0]; pix[q][1] = d[1]; pix[q][2] = d[2]; }
                            covered |= 1u << i;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PT_TY / 4; ++i) {
        if (covered & (1u << i)) {
            unsigned char* d = A.page + ((size_t)(Y0 + ty + 4 * i) * page_w + (size_t)(X0 + tx)) * 3;
            d[0] = pix[i][0]; d[1] = pix[i][1]; d[2] = pix[i][2];
        }
    }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what the two entry points check alike, in the words of `who`, and the launch: one workgroup per tile of the page.  A holds the caller's tables;
// the page's size and the tile count are filled in here.
template <bool CELLS_ONLY>
int tiles_launch(const char* who, MixedArgs A, int32_t n_spans, void* stream) {
    MNET_CHECK_ALIGN(aligned_to(A.items, 4) && aligned_to(A.spans, 4) && aligned_to(A.order, 4), "%s: %s must be 4-byte aligned", who,
                     CELLS_ONLY ? "spans and order" : "items, spans and order");
    const PtGrid g = pt_grid(1, A.page_w, A.page_h);
    MNET_CHECK_ARG(g.blocks <= PT_MAX_BLOCKS, "%s: page too large (%lld tiles)", who, g.blocks);
    // a launch of more than 2^32 - 1 threads runs only a part of its workgroups, without an error: refuse it (2^24 tiles are 17 gigapixels)
    MNET_CHECK_ARG(g.blocks * 256 <= 0xffffffffll, "%s: page too large (%lld tiles of 256 threads are 2^32 threads or more)", who, g.blocks);
    MNET_CHECK_ARG((long long)n_spans == g.blocks, "%s: %d spans for a page of %lld tiles (%d x %d)", who, n_spans, g.blocks, A.page_w, A.page_h);
    A.tiles_x = (int)g.tiles_x;
    hipLaunchKernelGGL(paste_tiles_kernel<CELLS_ONLY>, dim3((unsigned)g.blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), A);
    MNET_LAUNCH_CHECK(who);
    return MNET_OK;
}

}  // namespace

extern "C" int mnet_paste_ordered_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_column_paste* cells, int32_t n_cells,
                                     const mnet_tile_span* spans, int32_t n_spans, const int32_t* order, int32_t n_order, uint8_t* page, int32_t page_h,
                                     int32_t page_w, void* stream) {
    const char* who = "paste_ordered_u8";
    MNET_CHECK_ARG(lines && cells && spans && order && page, "%s: null pointer", who);
    MNET_CHECK_ARG(n_lines >= 1 && rows >= 1 && line_w >= 1 && n_cells >= 1 && n_order >= 1 && page_h >= 1 && page_w >= 1,
                   "%s: bad shape (n_lines=%d, rows=%d, line_w=%d, n_cells=%d, n_order=%d, page_h=%d, page_w=%d)", who, n_lines, rows, line_w, n_cells,
                   n_order, page_h, page_w);
    MNET_CHECK_ALIGN(aligned_to(cells, 8), "%s: cells must be 8-byte aligned", who);
    return tiles_launch<true>(who, {lines, n_lines, rows, line_w, nullptr, 0, 0, cells, n_cells, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, spans, order,
                                    n_order, 0, page, page_h, page_w}, n_spans, stream);
}

extern "C" int mnet_paste_mixed_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const uint8_t* atlas, int32_t atlas_h, int32_t atlas_w,
                                   const mnet_column_paste* cells, int32_t n_cells, const mnet_quad_region* quads, int32_t n_quads,
                                   const mnet_curve_region* curves, int32_t n_curves, const mnet_curve_seg* segs, int32_t n_segs,
                                   const mnet_page_item* items, int32_t n_items, const mnet_tile_span* spans, int32_t n_spans, const int32_t* order,
                                   int32_t n_order, uint8_t* page, int32_t page_h, int32_t page_w, void* stream) {
    const char* who = "paste_mixed_u8";
    MNET_CHECK_ARG(n_cells >= 0 && n_quads >= 0 && n_curves >= 0 && n_segs >= 0 && n_items >= 1 && n_order >= 1 && page_h >= 1 && page_w >= 1,
                   "%s: bad shape (n_cells=%d, n_quads=%d, n_curves=%d, n_segs=%d, n_items=%d, n_order=%d, page_h=%d, page_w=%d)", who, n_cells, n_quads,
                   n_curves, n_segs, n_items, n_order, page_h, page_w);
    MNET_CHECK_ARG(items && spans && order && page, "%s: null pointer", who);
    MNET_CHECK_ARG((cells || !n_cells) && (quads || !n_quads) && (curves || !n_curves) && (segs || !n_curves) && (lines || !n_cells) &&
                   (atlas || !(n_quads || n_curves)), "%s: null pointer for a table, the lines or the atlas that a nonzero count reads", who);
    MNET_CHECK_ARG(!n_cells || (n_lines >= 1 && rows >= 1 && line_w >= 1), "%s: bad shape (n_lines=%d, rows=%d, line_w=%d with %d cells)", who, n_lines,
                   rows, line_w, n_cells);
    MNET_CHECK_ARG(!(n_quads || n_curves) || (atlas_h >= 1 && atlas_w >= 1), "%s: bad shape (atlas_h=%d, atlas_w=%d with %d quads and %d curves)", who,
                   atlas_h, atlas_w, n_quads, n_curves);
    MNET_CHECK_ARG(!n_curves || n_segs >= 1, "%s: bad shape (n_segs=%d with %d curves)", who, n_segs, n_curves);
    MNET_CHECK_ALIGN(aligned_to(cells, 8) && aligned_to(quads, 8) && aligned_to(curves, 8) && aligned_to(segs, 8),
                     "%s: cells, quads, curves and segs must be 8-byte aligned", who);
    return tiles_launch<false>(who, {lines, n_lines, rows, line_w, atlas, atlas_h, atlas_w, cells, n_cells, quads, n_quads, curves, n_curves, segs, n_segs,
                                     items, n_items, spans, order, n_order, 0, page, page_h, page_w}, n_spans, stream);
}
