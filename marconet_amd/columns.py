"""Vertical text columns of a page: upright characters stacked top to bottom, as on shop signs, couplets, book spines and in traditional
typesetting.  ``quads`` can only turn such a column by 90 degrees, which feeds the networks characters lying on their side; this module lays the
column's character cells side by side as the horizontal strip the encoder expects, and brings each restored character back to its own cell.  The
networks see an ordinary line.  Everything is stated in integers, with arithmetic the project already has (``pages.resize_cubic_to``,
``pages.line_to_rect``, ``pages.box_factor``, ``pages.feather_blend``, ``long_lines.plan_windows``), and the device returns the same bytes:

    cell_cuts, cell_widths            the cells: cuts t_0 = y1 < t_1 < ... < t_n = y2 tile the column, cell j is page[t_j:t_j+1, x1:x2]
    virtual_strip, virtual_boxes      each cell resized on its own to w_j x 32 (taps clamped at the CELL's border) and stacked horizontally: the
                                      virtual strip V [32, Wv, 3], with the character boxes [o_j, 0, o_j+1, 32] — from here an ordinary line
    paste_column_host                 cell j's foreground is ``pages.line_to_rect`` of its slice [4 o_j, 4 o_j+1) of the restored line; the column's
                                      is their vstack, blended by ONE ``pages.feather_blend`` over the whole column: no ramp between cells
    check_columns                     the refusals
    compose_columns_host              the pure-host definition of a page that mixes columns and horizontal lines
    gather_table, paste_table,        the same bytes on the device: one ``mnet_column_gather_u8`` launch makes every window of every column, one
    gather_columns, paste_columns     ``mnet_column_paste_u8`` launch pastes every cell

A column is an integer axis-aligned box [x1, y1, x2, y2] in page pixels (``pages.round_box`` rounds a detector's box outward) whose text is read top
to bottom.  ``MarconetPipeline.restore_page_columns`` ties it to the networks.  Out of scope: vertical columns that are rotated or in perspective,
right-to-left ordering of the columns (the caller's), curved vertical columns (curved horizontal text: ``curves``), detection and recognition, several pages per launch.
"""
import numpy as np
import torch

from . import _lib, lq_device, lq_io, ops, pages

LQ_H = lq_device.LQ_H         # the height of the virtual strip: the encoder's own, so that it reaches the encoder unchanged
ROW_H = pages.ROW_H           # the height of a restored line
UP = ROW_H // LQ_H            # a column of the virtual strip is UP columns of the restored line


def _who(region, char=None):
    return ("" if region is None else "region %d: " % region) + ("" if char is None else "character %d: " % char)


# --------------------------------------------------------------------------------------------------------------------------- the cells
def cell_cuts(box, n, char_boxes=None, region=None):
    """the n + 1 cuts of a column of n characters → list of ints, t_0 = y1 and t_n = y2.  Without character boxes t_j = y1 + (2 j ch + n) // (2 n):
    j ch / n rounded half up.  With ``char_boxes`` ([x1, y1, x2, y2] in page pixels, top to bottom) the cut between characters j − 1 and j lies in the
    middle of their gap, (floor(cb[j−1].y2) + floor(cb[j].y1)) // 2, clamped into [y1, y2]: ``long_lines.plan_windows``' own rule, turned by 90
    degrees.  ValueError naming ``region`` (and the character) for a column without a character, a count of character boxes other than n, and cuts
    that do not increase strictly (an empty cell)."""
    x1, y1, x2, y2 = (int(v) for v in box)
    n, ch = int(n), y2 - y1
    if n < 1:
        raise ValueError("%sa column without a character has no cells" % _who(region))
    if char_boxes is None:
        cuts = [y1 + (2 * j * ch + n) // (2 * n) for j in range(n + 1)]
    else:
        cb = np.asarray(char_boxes, dtype=np.float64).reshape(-1, 4)
        if cb.shape[0] != n:
            raise ValueError("%s%d character boxes for %d characters" % (_who(region), cb.shape[0], n))
        top, bottom = np.floor(cb[:, 1]).astype(np.int64), np.floor(cb[:, 3]).astype(np.int64)
        cuts = [y1] + [min(max(int(bottom[j - 1] + top[j]) // 2, y1), y2) for j in range(1, n)] + [y2]
    _strictly_increasing(cuts, region)
    return cuts


def _strictly_increasing(cuts, region):
    for j in range(len(cuts) - 1):
        if cuts[j + 1] <= cuts[j]:
            raise ValueError("%sits cell is empty (rows %d..%d of the page): the cuts must increase strictly" % (_who(region, j), cuts[j], cuts[j + 1]))


def cell_widths(box, cuts):
    """w_j = max(1, rint(cw · 32 / h_j)): the width of cell j at height 32, its aspect kept (round half to even, as ``lq_io.resize_cubic`` sizes)"""
    cw = int(box[2]) - int(box[0])
    return [max(1, int(np.rint(cw * LQ_H / (int(cuts[j + 1]) - int(cuts[j]))))) for j in range(len(cuts) - 1)]


def virtual_strip(page, box, cuts):
    """→ (V, widths): V = np.hstack of ``pages.resize_cubic_to(page[t_j:t_j+1, x1:x2], w_j, 32)`` over the cells, uint8 RGB [32, Σ w_j, 3]; each
    cell is resized on its own, so the taps clamp at the cell's border, not the page's"""
    page = pages._page_array(page)
    x1, x2 = int(box[0]), int(box[2])
    widths = cell_widths(box, cuts)
    cells = [pages.resize_cubic_to(page[int(cuts[j]):int(cuts[j + 1]), x1:x2], w, LQ_H) for j, w in enumerate(widths)]
    return np.ascontiguousarray(np.hstack(cells)), widths


def cell_offsets(widths):
    """o_0 = 0, o_j+1 = o_j + w_j: the cells' first columns in the virtual strip"""
    return [0] + [int(v) for v in np.cumsum([int(w) for w in widths])]


def virtual_boxes(widths):
    """the virtual strip's character boxes [o_j, 0, o_j+1, 32]: they tile the strip, so every window cut of ``plan_windows`` falls on a cell boundary"""
    o = cell_offsets(widths)
    return [[o[j], 0, o[j + 1], LQ_H] for j in range(len(widths))]


# --------------------------------------------------------------------------------------------------------------------------- the paste
def _column_scale(rect, cuts):
    rw, rh, ch = int(rect[2]), int(rect[3]), int(cuts[-1]) - int(cuts[0])
    if ch < 1 or rh % ch:
        raise ValueError("the column's rectangle is %d rows high, no multiple of its %d page rows" % (rh, ch))
    return rh // ch


def column_foreground(line_bgr, rect, cuts, widths):
    """the column's foreground, uint8 RGB [rh, rw, 3]: the vstack over the cells of ``pages.line_to_rect(L[:, UP o_j : UP o_j+1], rw, s h_j)`` — every
    cell with its own ``pages.box_factor(s h_j)``"""
    line_bgr = np.asarray(line_bgr)
    s, o, up = _column_scale(rect, cuts), cell_offsets(widths), line_bgr.shape[0] // LQ_H
    if len(widths) != len(cuts) - 1 or line_bgr.shape[1] != up * o[-1]:
        raise ValueError("a line of %d columns expected for cells of widths %s, got %d" % (up * o[-1], list(widths), line_bgr.shape[1]))
    return np.vstack([pages.line_to_rect(line_bgr[:, up * o[j]:up * o[j + 1]], int(rect[2]), s * (int(cuts[j + 1]) - int(cuts[j]))) for j in range(len(widths))])


def paste_column_host(page_up, line_bgr, rect, cuts, widths, feather):
    """the definition of one column: ``page_up`` (uint8 RGB [PH, PW, 3], the enlarged page) is changed IN PLACE inside ``rect`` = (x0, y0, rw, rh), the
    column's rectangle there, and returned; ``line_bgr``: the restored line of its virtual strip, uint8 BGR [rows, UP · Σ w_j, 3]; ``cuts`` in page
    pixels.  ONE ``pages.feather_blend`` over the whole rectangle: the ramp follows the column's outer edge, there is none between cells."""
    x0, y0, rw, rh = (int(v) for v in rect)
    if page_up.dtype != np.uint8 or page_up.ndim != 3 or page_up.shape[2] != 3:
        raise TypeError("paste_column_host: uint8 RGB HxWx3 page expected")
    if rw < 1 or rh < 1 or x0 < 0 or y0 < 0 or x0 + rw > page_up.shape[1] or y0 + rh > page_up.shape[0]:
        raise ValueError("paste_column_host: rectangle %s outside the %d x %d page" % ((x0, y0, rw, rh), page_up.shape[1], page_up.shape[0]))
    view = page_up[y0:y0 + rh, x0:x0 + rw]
    view[...] = pages.feather_blend(view, column_foreground(line_bgr, rect, cuts, widths), feather)
    return page_up


# ------------------------------------------------------------------------------------------------------------------------- the refusals
def check_columns(page_h, page_w, boxes, restored, cuts_per_region, scale, feather, rows=ROW_H, overlap="refuse"):
    """the refusals, all ValueError naming the region (and the character where there is one), and the regions' rectangles (x0, y0, rw, rh) in the
    enlarged page.  ``cuts_per_region[i]``: the cuts of region i where it is a column, None where it is a horizontal line.  Refused: everything
    ``pages.region_rects`` refuses (scale, feather, a box that is empty or outside the page, a rectangle under rows / 16 rows, two restored regions
    that overlap — across both kinds of region, unless ``overlap="order"``: ``pages``' head); for a restored column, cuts that do not run from y1 to y2 or do not increase strictly, and a cell
    under rows / 16 output rows (16 s h_j < rows: the box reduction stops at 8)."""
    if len(cuts_per_region) != len(boxes):
        raise ValueError("one list of cuts (or None) per box expected (%d boxes, %d lists)" % (len(boxes), len(cuts_per_region)))
    rects = pages.region_rects(page_h, page_w, boxes, restored, scale, feather, rows, overlap)
    s = int(scale)
    for i, cuts in enumerate(cuts_per_region):
        if cuts is None or not restored[i]:
            continue
        cuts = [int(c) for c in cuts]
        if len(cuts) < 2 or cuts[0] != int(boxes[i][1]) or cuts[-1] != int(boxes[i][3]):
            raise ValueError("region %d: its cuts %s do not run from y1 = %d to y2 = %d" % (i, cuts, int(boxes[i][1]), int(boxes[i][3])))
        _strictly_increasing(cuts, i)
        for j in range(len(cuts) - 1):
            if s * (cuts[j + 1] - cuts[j]) * pages.MIN_RECT_H_DIV < rows:
                raise ValueError("region %d: character %d: its cell is %d rows high at scale %d, under the %d a %d-row line can be reduced to"
                                 % (i, j, s * (cuts[j + 1] - cuts[j]), s, rows // pages.MIN_RECT_H_DIV, rows))
    return rects


# ------------------------------------------------------------------------------------------------------------------- the definition
def compose_columns_host(page, lines, boxes, cuts_per_region, scale=4, feather=8, overlap="refuse"):
    """the definition of a page: ``page`` uint8 RGB [H, W, 3]; ``boxes[i]`` region i's integer box; ``cuts_per_region[i]`` its cuts where it is a
    column (``cell_cuts``), None where it is a horizontal line; ``lines[i]``: its restored line, uint8 BGR [rows, w, 3] — for a column
    ``MarconetPipeline.restore_lines`` of ``virtual_strip(page, box, cuts)`` with ``virtual_boxes``, for a line that of the crop — or None for a
    region that keeps the background → uint8 RGB [s·H, s·W, 3]: ``lq_io.resize_cubic(page, s, s)`` with ``paste_column_host`` of every column and
    ``pages.paste_host`` of every line, in list order — which only shows where ``overlap="order"`` lets regions overlap (``pages``' head)."""
    page = pages._page_array(page)
    rows = next((int(np.shape(l)[0]) for l in lines if l is not None), ROW_H)
    rects = check_columns(page.shape[0], page.shape[1], boxes, [l is not None for l in lines], cuts_per_region, scale, feather, rows, overlap)
    out = lq_io.resize_cubic(page, int(scale), int(scale))
    for line, rect, box, cuts in zip(lines, rects, boxes, cuts_per_region):
        if line is None:
            continue
        if cuts is None:
            pages.paste_host(out, line, rect, int(feather))
        else:
            paste_column_host(out, line, rect, cuts, cell_widths(box, cuts), int(feather))
    return out


# ------------------------------------------------------------------------------------------------------------------- the device path
def gather_table(columns, base=0, dst_h=LQ_H):
    """``columns[c]`` = (box, cuts, widths, plan): a column and the ``plan_windows`` result of its virtual strip → (numpy record array of
    ``mnet_column_cell``, one per (window, cell) in the plans' order; per window its (h, w); per window its byte offset; the flat buffer's size): the
    window images are packed tightly from byte ``base``.  ValueError for a window cut that does not fall on a cell boundary."""
    recs, shapes, offsets, off = [], [], [], int(base)
    for box, cuts, widths, plan in columns:
        x1, x2 = int(box[0]), int(box[2])
        o = cell_offsets(widths)
        for p in plan:
            if p.c0 != o[p.g0] or p.c1 != o[p.g1]:
                raise ValueError("the window of characters %d..%d spans columns %d..%d of the virtual strip, not its cells' %d..%d" % (p.g0, p.g1, p.c0, p.c1, o[p.g0], o[p.g1]))
            for j in range(p.g0, p.g1):
                sh = int(cuts[j + 1]) - int(cuts[j])
                recs.append((off, p.c1 - p.c0, o[j] - p.c0, int(widths[j]), x1, int(cuts[j]), x2 - x1, sh, 0,
                             pages.axis_scale(widths[j], x2 - x1), pages.axis_scale(dst_h, sh)))
            shapes.append((int(dst_h), p.c1 - p.c0))
            offsets.append(off)
            off += 3 * int(dst_h) * (p.c1 - p.c0)
    tab = np.zeros((len(recs),), dtype=np.dtype(_lib.ColumnCell))
    for k, r in enumerate(recs):
        tab[k] = r
    return tab, shapes, offsets, off


def paste_table(columns, line_index, rects, feather, rows=ROW_H):
    """→ numpy record array of ``mnet_column_paste``, one per cell: column c (``columns[c]`` as ``gather_table`` takes it; its plan is not read) reads
    line ``line_index[c]`` into ``rects[c]``, its rectangle in the enlarged page, which is every cell's feather rectangle"""
    recs, up = [], int(rows) // LQ_H
    for (box, cuts, widths, _), l, rect in zip(columns, line_index, rects):
        x0, y0, rw, rh = (int(v) for v in rect)
        s, o = _column_scale(rect, cuts), cell_offsets(widths)
        for j, w in enumerate(widths):
            ch = s * (int(cuts[j + 1]) - int(cuts[j]))
            k = pages.box_factor(ch, rows)
            recs.append((int(l), up * o[j], up * int(w), x0, y0 + s * (int(cuts[j]) - int(cuts[0])), rw, ch, int(feather), k, x0, y0, rw, rh, 0,
                         pages.axis_scale(rw, -(-up * int(w) // k)), pages.axis_scale(ch, int(rows) // k)))
    tab = np.zeros((len(recs),), dtype=np.dtype(_lib.ColumnPaste))
    for n, r in enumerate(recs):
        tab[n] = r
    return tab


def gather_columns(page_d, columns, base=0):
    """``page_d`` uint8 RGB [H, W, 3] on the device → (uint8 [bytes] on the device: from byte ``base`` the windows of every column's virtual strip —
    ``virtual_strip(page, box, cuts)[0][:, c0:c1]`` —, packed tightly in order, the first ``base`` bytes left to the caller; per window its (h, w);
    per window its offset): one copy of the table, one launch.  The result is the ragged batch ``lq_device.prepare_packed`` accepts."""
    tab, shapes, offsets, nbytes = gather_table(columns, base)
    dst = torch.empty((nbytes,), dtype=torch.uint8, device=page_d.device)
    with ops.on_device(page_d):
        ops.column_gather_u8(page_d, ops.table_to_device(tab, page_d.device), int(tab["dw"].max()), LQ_H, dst)
    return dst, shapes, offsets


def paste_columns(out, joined, line_index, columns, rects, feather):
    """``out``: the enlarged page on the device, changed IN PLACE; ``joined``: uint8 BGR [L, rows, line_w, 3] on the device
    (``long_lines.compose_lines``); column c reads line ``line_index[c]`` into ``rects[c]``: ``paste_column_host``'s bytes.  One copy of the table, one
    launch for all cells of all columns."""
    if not columns:
        return out
    rows = int(joined.shape[1])
    _check_lines("paste_columns", joined, line_index, columns)
    tab = paste_table(columns, line_index, rects, feather, rows)
    with ops.on_device(out):
        ops.column_paste_u8(joined, ops.table_to_device(tab, out.device), out)
    return out


def _check_lines(who, joined, line_index, columns):
    rows = int(joined.shape[1])
    for c, (_, _, widths, _) in enumerate(columns):
        if not 0 <= int(line_index[c]) < joined.shape[0] or (rows // LQ_H) * cell_offsets(widths)[-1] > joined.shape[2]:
            raise ValueError("%s: column %d: line %d of %d columns does not lie inside the lines %s" % (who, c, int(line_index[c]), (rows // LQ_H) * cell_offsets(widths)[-1], list(joined.shape)))


def mixed_table(joined, regions, feather):
    """one table for ``pages.paste_ordered``: ``regions`` in paste order, region r = (its line's index in ``joined``, its rectangle in the enlarged
    page, the width of its line — a horizontal line — or its column as ``gather_table`` takes it) → record array of ``mnet_column_paste``: a line as
    ``pages.as_cell`` of ``pages.build_table``'s record, a column as ``paste_table``'s cells, consecutive.  ``paste_columns``' refusals."""
    for l, rect, what in regions:
        if isinstance(what, tuple):
            _check_lines("mixed_table", joined, [l], [what])
    parts = [region_cells(l, rect, what, feather, int(joined.shape[1])) for l, rect, what in regions]
    return np.concatenate(parts) if parts else np.zeros((0,), dtype=np.dtype(_lib.ColumnPaste))


def region_cells(l, rect, what, feather, rows=ROW_H):
    """the ``mnet_column_paste`` records of ONE region of ``mixed_table``, which reads line ``l`` into ``rect``: ``what`` is the width of a horizontal
    line (→ one record, ``pages.as_cell`` of ``pages.build_table``'s) or a column as ``gather_table`` takes it (→ ``paste_table``'s cells)"""
    if isinstance(what, tuple):
        return paste_table([what], [l], [rect], feather, rows)
    return pages.as_cell(pages.build_table([rect], [int(what)], feather, rows, [l]))
