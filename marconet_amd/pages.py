"""A page and its text regions: the enlarged page with every restored text line pasted back in place.  The script restores strips and stops there;
its user has a scanned page or a photo and a detector's text-line boxes.  This module states what "in place" means, in integers, and returns the
same bytes from the device:

    box_factor, box_reduce    a restored line (height ``ROW_H`` = 128) is first averaged over k x k blocks, so that the cubic below never skips a pixel
    resize_cubic_to           ``lq_io.resize_cubic``'s arithmetic to a GIVEN size: the intermediate → exactly the region's rectangle
    feather_blend             the integer blend of the line into the background near the rectangle's edge
    paste_host, compose_host  the pure-host definition of one region and of a page
    build_table, paste_rects, the same bytes with one kernel launch (``mnet_paste_u8``) from the joined lines ``long_lines.compose_lines`` leaves on
    enlarge, compose_page     the device and the background ``ops.lq_from_u8(preview=True)`` makes of the page: ``lq_io.resize_cubic(page, s, s)``
    check_request,            what ``quads`` and ``columns`` share with this module: the refusals of scale and feather, and the intake of a host or
    page_to_device            device page with its joined lines
    as_cell, bin_tiles,       overlapping regions in the caller's order: one table of cells, the cells of every 64 x 16 tile of the page, and ONE
    paste_ordered             ``mnet_paste_ordered_u8`` launch whose workgroups own page tiles

Overlap.  Two regions that share a pixel are refused by default (``overlap="refuse"``): the per-descriptor kernels blend in place, so an overlap has
no order there.  ``overlap="order"`` is painter's order, and this is its one statement: the regions are pasted one after another in list order by
``paste_host`` (a column by ``columns.paste_column_host``); a later region is blended, under its own feather ramp, into what the page holds at that
moment, earlier regions included.  The loops of ``compose_host`` and ``columns.compose_columns_host`` do exactly that; ``"order"`` only drops the
pairwise refusal, every other refusal stands, and the crops the networks read are taken from the original page, so they do not depend on the order.
The device reproduces it byte for byte (``mnet_paste_ordered_u8``: one thread does all blends of a pixel, in that order).  The same order holds
across kinds of region — a quadrilateral by ``quads.warp_paste_host``, a curve by ``curves.warp_paste_host``, in their place of the list:
``regions.compose_regions_host``, ``mnet_paste_mixed_u8``.

``MarconetPipeline.restore_page`` ties them to the networks.  A region is an axis-aligned integer box [x1, y1, x2, y2] in page pixels: the reference
handles regular layouts without perspective only; rotated and quadrilateral regions are ``quads``' (``MarconetPipeline.restore_page_quads``).  Out of
scope: vertical columns that are rotated or in perspective (upright columns of stacked characters are ``columns``': ``MarconetPipeline.
restore_page_columns``; a page that mixes boxes, columns, quadrilaterals and curves, overlapping or not, is ``regions``':
``MarconetPipeline.restore_page_regions``), any blend of overlapping regions other than painter's order, detection beyond horizontal lines in columns on plain paper
(``layout``: ``MarconetPipeline.find_lines`` / ``restore_page_auto`` find those from ink profiles; every other box is the caller's) and
recognition beyond the encoder's own reading (``blind``), and several pages in one launch.
"""
import math

import numpy as np
import torch

from . import _lib, lq_device, lq_io, ops

ROW_H = lq_device.SHOW_H      # the height of a restored line (``restore_lines``)
MAX_SCALE, MAX_FEATHER, MAX_K = 8, 1024, 8
MIN_RECT_H_DIV = 16           # a rectangle under ROW_H / 16 = 8 rows is refused: the box reduction stops at 8, the cubic would skip rows
TILE_W, TILE_H = 64, 16       # csrc/page_tile.h's tile, which mnet_paste_ordered_u8 counts from the page's origin
MAX_TILES = 2 ** 31 - 1       # PT_MAX_BLOCKS; the span's fields are int32 too
OVERLAP_MODES = ("refuse", "order")


def check_overlap(overlap):
    """``overlap`` is "refuse" or "order" (ValueError otherwise) → whether overlapping regions are pasted in list order"""
    if overlap not in OVERLAP_MODES:
        raise ValueError('overlap must be "refuse" or "order", got %r' % (overlap,))
    return overlap == "order"


def box_factor(rh, rows=ROW_H):
    """the largest power of two k with k·rh ≤ rows, at most 8; 1 for a rectangle that is not lower than the line"""
    k = 1
    while k < MAX_K and 2 * k * int(rh) <= int(rows):
        k *= 2
    return k


def box_reduce(line, k):
    """uint8 [rows, w, c] → uint8 [rows / k, ceil(w / k), c]: every k x k block (k x c', c' < k, at a ragged right edge) replaced per channel by
    its mean rounded half up, (2·sum + cnt) // (2·cnt) — csrc/page_blend.h's page_box_avg"""
    line, k = np.asarray(line), int(k)
    if line.dtype != np.uint8 or line.ndim != 3:
        raise TypeError("box_reduce: uint8 HxWxC image expected")
    rows, w, c = line.shape
    if k not in (1, 2, 4, 8) or rows % k or w < 1:
        raise ValueError("box_reduce: k in {1, 2, 4, 8} dividing the %d rows, and at least one column, expected (k = %d, w = %d)" % (rows, k, w))
    nx = -(-w // k)
    pad = np.zeros((rows, nx * k, c), dtype=np.int64)
    pad[:, :w] = line
    s = pad.reshape(rows // k, k, nx, k, c).sum(axis=(1, 3))
    cnt = (k * np.minimum(k, w - k * np.arange(nx)))[None, :, None]
    return ((2 * s + cnt) // (2 * cnt)).astype(np.uint8)


def axis_scale(n_dst, n_src):
    """the sampling step of one axis as ``lq_io._cubic_taps(n_dst, n_src, n_dst / n_src)`` computes it — the double the device table carries"""
    return 1.0 / (int(n_dst) / int(n_src))


def resize_cubic_to(img, dst_w, dst_h):
    """``cv2.resize(img, (dst_w, dst_h), interpolation=cv2.INTER_CUBIC)`` for a uint8 HxWxC image: ``lq_io.resize_cubic``'s integer passes and its
    single rounding shift by 22 bits, with the taps ``lq_io._cubic_taps(n_dst, n_src, n_dst / n_src)`` of the two sizes themselves, per axis"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise TypeError("resize_cubic_to: uint8 HxWxC image expected")
    h, w, _ = img.shape
    dst_w, dst_h = int(dst_w), int(dst_h)
    if dst_w < 1 or dst_h < 1 or h < 1 or w < 1:
        raise ValueError("resize_cubic_to: empty image or output")
    xi, xt = lq_io._cubic_taps(dst_w, w, dst_w / w)
    yi, yt = lq_io._cubic_taps(dst_h, h, dst_h / h)
    src = img.astype(np.int64)
    hor = (src[:, xi, :] * xt[None, :, :, None]).sum(axis=2)                 # [h, dst_w, c]
    ver = (hor[yi, :, :] * yt[:, :, None, None]).sum(axis=1)                 # [dst_h, dst_w, c]
    return np.clip((ver + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def feather_axis(n, feather):
    """csrc/page_blend.h's page_feather_axis for every coordinate of an axis of n pixels: min(2·min(u, n−1−u) + 1, 2F)"""
    u = np.arange(int(n), dtype=np.int64)
    return np.minimum(2 * np.minimum(u, int(n) - 1 - u) + 1, 2 * int(feather))


def feather_blend(bg, fg, feather):
    """bg, fg: uint8 [RH, RW, c] → the rectangle's bytes.  F = 0: fg.  Else at (u, v): m = a·b with a = ``feather_axis(RW, F)[u]``, b the same on
    (v, RH); D = 4F²; (bg·(D − m) + fg·m + D // 2) // D — csrc/page_blend.h's page_feather.  The line's weight m / D is symmetric, at most 1 / (2F) at
    the edge and exactly 1 from F pixels inside, on both axes."""
    bg, fg, F = np.asarray(bg), np.asarray(fg), int(feather)
    if bg.shape != fg.shape or bg.dtype != np.uint8 or fg.dtype != np.uint8 or bg.ndim != 3:
        raise ValueError("feather_blend: two uint8 images of one shape expected")
    if not 0 <= F <= MAX_FEATHER:
        raise ValueError("feather_blend: feather %d outside [0, %d]" % (F, MAX_FEATHER))
    if F == 0:
        return fg.copy()
    m = (feather_axis(bg.shape[0], F)[:, None] * feather_axis(bg.shape[1], F)[None, :])[:, :, None]
    D = 4 * F * F
    return ((bg.astype(np.int64) * (D - m) + fg.astype(np.int64) * m + D // 2) // D).astype(np.uint8)


def line_to_rect(line_bgr, rw, rh):
    """a restored line, uint8 BGR [rows, src_w, 3] → the rectangle's foreground, uint8 RGB [rh, rw, 3]: box reduction, cubic, channel flip"""
    line_bgr = np.asarray(line_bgr)
    return np.ascontiguousarray(resize_cubic_to(box_reduce(line_bgr, box_factor(rh, line_bgr.shape[0])), rw, rh)[:, :, ::-1])


def paste_host(page_up, line_bgr, rect, feather):
    """the definition of one region: ``page_up`` (uint8 RGB [PH, PW, 3], the enlarged page) is changed IN PLACE inside ``rect`` = (x0, y0, rw, rh)
    and returned; ``line_bgr``: the region's restored line, uint8 BGR [rows, src_w, 3]"""
    x0, y0, rw, rh = (int(v) for v in rect)
    if page_up.dtype != np.uint8 or page_up.ndim != 3 or page_up.shape[2] != 3:
        raise TypeError("paste_host: uint8 RGB HxWx3 page expected")
    if rw < 1 or rh < 1 or x0 < 0 or y0 < 0 or x0 + rw > page_up.shape[1] or y0 + rh > page_up.shape[0]:
        raise ValueError("paste_host: rectangle %s outside the %d x %d page" % ((x0, y0, rw, rh), page_up.shape[1], page_up.shape[0]))
    view = page_up[y0:y0 + rh, x0:x0 + rw]
    view[...] = feather_blend(view, line_to_rect(line_bgr, rw, rh), feather)
    return page_up


def round_box(box, page_h, page_w):
    """a detector's box [x1, y1, x2, y2] (any numbers) → integers, rounded outward and clamped into the page"""
    x1, y1, x2, y2 = (float(v) for v in box)
    return [min(max(int(math.floor(x1)), 0), int(page_w)), min(max(int(math.floor(y1)), 0), int(page_h)),
            min(max(int(math.ceil(x2)), 0), int(page_w)), min(max(int(math.ceil(y2)), 0), int(page_h))]


def check_request(scale, feather, n_regions, n_lines, unit, units):
    """the refusals every kind of region shares (ValueError): ``scale`` outside [1, 8] or ``feather`` outside [0, 1024] (integers), and a count of
    lines other than that of the regions, which the message calls ``unit`` / ``units``"""
    if int(scale) != scale or not 1 <= int(scale) <= MAX_SCALE:
        raise ValueError("scale must be an integer in [1, %d], got %r" % (MAX_SCALE, scale))
    if int(feather) != feather or not 0 <= int(feather) <= MAX_FEATHER:
        raise ValueError("feather must be an integer in [0, %d], got %r" % (MAX_FEATHER, feather))
    if n_lines != n_regions:
        raise ValueError("one line (or None) per %s expected (%d %s, %d lines)" % (unit, n_regions, units, n_lines))


def region_rects(page_h, page_w, boxes, restored, scale, feather, rows=ROW_H, overlap="refuse"):
    """the refusals, all ValueError naming the region, and the regions' rectangles (x0, y0, rw, rh) in the enlarged page.  ``restored[i]``: region i
    has a line to paste (the others keep the background: only their box is checked).  Refused: ``scale`` outside [1, 8] or ``feather`` outside
    [0, 1024] (integers); a box that is not four integers with 0 ≤ x1 < x2 ≤ W and 0 ≤ y1 < y2 ≤ H; a restored region's rectangle under rows / 16
    rows; two restored regions whose rectangles overlap, unless ``overlap="order"`` (the head of this module: list order is paste order)."""
    ordered = check_overlap(overlap)
    check_request(scale, feather, len(boxes), len(restored), "box", "boxes")
    s, rects = int(scale), []
    for i, b in enumerate(boxes):
        if len(b) != 4 or any(int(v) != v for v in b):
            raise ValueError("region %d: an integer box [x1, y1, x2, y2] expected, got %r (round_box rounds a detector's box outward)" % (i, list(b)))
        x1, y1, x2, y2 = (int(v) for v in b)
        if not (0 <= x1 < x2 <= page_w and 0 <= y1 < y2 <= page_h):
            raise ValueError("region %d: box %s is empty or lies outside the %d x %d page" % (i, [x1, y1, x2, y2], page_w, page_h))
        rects.append((s * x1, s * y1, s * (x2 - x1), s * (y2 - y1)))
        if restored[i] and rects[i][3] * MIN_RECT_H_DIV < rows:
            raise ValueError("region %d: its rectangle is %d rows high at scale %d, under the %d a %d-row line can be reduced to"
                             % (i, rects[i][3], s, rows // MIN_RECT_H_DIV, rows))
    live = [] if ordered else [i for i in range(len(boxes)) if restored[i]]
    for n, i in enumerate(live):
        for j in live[:n]:
            a, b = rects[i], rects[j]
            if a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]:
                raise ValueError("regions %d and %d overlap: the paste blends in place, so an overlap has no defined order" % (j, i))
    return rects


def _page_array(page):
    page = np.asarray(page)
    if page.dtype != np.uint8 or page.ndim != 3 or page.shape[2] != 3 or page.shape[0] < 1 or page.shape[1] < 1:
        raise TypeError("uint8 RGB HxWx3 page expected")
    return page


def compose_host(page, lines, boxes, scale=4, feather=8, overlap="refuse"):
    """the definition of a page: ``page`` uint8 RGB [H, W, 3]; ``lines[i]``: region i's restored line, uint8 BGR [rows, src_w, 3]
    (``MarconetPipeline.restore_lines`` of the crop ``page[y1:y2, x1:x2]``), or None for a region that keeps the background; ``boxes[i]`` its
    integer box → uint8 RGB [s·H, s·W, 3]: ``lq_io.resize_cubic(page, s, s)`` with ``paste_host`` of every line in its rectangle
    (s·x1, s·y1, s·(x2 − x1), s·(y2 − y1)), in list order — which only shows where ``overlap="order"`` lets rectangles overlap."""
    page = _page_array(page)
    rows = next((int(np.shape(l)[0]) for l in lines if l is not None), ROW_H)
    rects = region_rects(page.shape[0], page.shape[1], boxes, [l is not None for l in lines], scale, feather, rows, overlap)
    out = lq_io.resize_cubic(page, int(scale), int(scale))
    for line, rect in zip(lines, rects):
        if line is not None:
            paste_host(out, line, rect, int(feather))
    return out


def build_table(rects, out_ws, feather, rows=ROW_H, line_index=None):
    """→ numpy record array of ``mnet_paste_region``, one per region with a line (``out_ws[i]`` is not None), in order: the l-th such region reads
    line ``line_index[l]`` (default l: the count of such regions before it), ``out_ws[i]`` columns wide, into ``rects[i]``"""
    live = [i for i, w in enumerate(out_ws) if w is not None]
    tab = np.zeros((len(live),), dtype=np.dtype(_lib.PasteRegion))
    for l, i in enumerate(live):
        x0, y0, rw, rh = rects[i]
        k = box_factor(rh, rows)
        tab[l] = (l if line_index is None else int(line_index[l]), int(out_ws[i]), x0, y0, rw, rh, int(feather), k,
                  axis_scale(rw, -(-int(out_ws[i]) // k)), axis_scale(rh, rows // k))
    return tab


def paste_rects(out, joined, rects, out_ws, feather, line_index=None):
    """``out``: the enlarged page on the device, changed IN PLACE; ``joined``: uint8 BGR [L, rows, line_w, 3] on the device; the regions of
    ``build_table(rects, out_ws, feather, rows, line_index)``: ``paste_host``'s bytes.  One copy of the table, one launch for all regions."""
    if any(w is not None for w in out_ws):
        with ops.on_device(out):
            ops.paste_u8(joined, ops.table_to_device(build_table(rects, out_ws, feather, int(joined.shape[1]), line_index), out.device), out)
    return out


def atlas_layout(sizes):
    """the atlas of upright foregrounds that quadrilaterals and curved regions are pasted from: ``sizes[i]`` = (rw, rh), or None for a region without
    one → (per region its rectangle (0, y, rw, rh), the rectangles stacked vertically in order, None where there is none; the atlas' (Σ rh, max rw))"""
    rects, y = [None] * len(sizes), 0
    for i, size in enumerate(sizes):
        if size is not None:
            rects[i] = (0, y, int(size[0]), int(size[1]))
            y += int(size[1])
    return rects, (y, max((r[2] for r in rects if r is not None), default=0))


def fill_atlas(joined, fg, atlas_hw):
    """→ the atlas on ``joined``'s device, uint8 RGB [Σ rh, max rw, 3], zeroed, with every line of ``joined`` brought to its upright foreground —
    ``line_to_rect``'s bytes — by ONE ``mnet_paste_u8`` launch; ``fg``: ``build_table`` of ``atlas_layout``'s rectangles at feather 0"""
    atlas = torch.zeros(tuple(atlas_hw) + (3,), dtype=torch.uint8, device=joined.device)
    with ops.on_device(joined):
        return ops.paste_u8(joined, ops.table_to_device(fg, joined.device), atlas)


def crop_buffer(who, dst, nbytes, device):
    """the flat buffer ``quads.crop_quads`` / ``curves.crop_curves`` write ``nbytes`` of: ``dst`` as given (ValueError naming ``who`` where it cannot
    hold them), or a new one on ``device`` for None"""
    if dst is None:
        return torch.empty((nbytes,), dtype=torch.uint8, device=device)
    if dst.dtype != torch.uint8 or dst.dim() != 1 or dst.numel() < nbytes:
        raise ValueError("%s: a flat uint8 buffer of at least %d bytes expected" % (who, nbytes))
    return dst


def as_cell(regions):
    """record array of ``mnet_paste_region`` → the same regions as ``mnet_column_paste`` records: the slice starts at column 0 and the feather
    rectangle is the region's own (csrc/page_kernels.hip's as_cell), so that one table holds lines and column cells together"""
    regions = np.asarray(regions)
    if regions.dtype != np.dtype(_lib.PasteRegion):
        raise TypeError("as_cell: a record array of mnet_paste_region expected")
    cells = np.zeros(regions.shape, dtype=np.dtype(_lib.ColumnPaste))
    for name in ("line_index", "src_w", "x0", "y0", "rw", "rh", "feather", "k", "scale_x", "scale_y"):
        cells[name] = regions[name]
    for name, src in (("fx0", "x0"), ("fy0", "y0"), ("fw", "rw"), ("fh", "rh")):
        cells[name] = regions[src]
    return cells


def bin_tiles(cells, page_h, page_w):
    """the cells of every 64 x 16 tile of a ``page_w`` x ``page_h`` page (tiles row-major from the page's origin) → (spans, order): ``spans`` a
    record array of ``mnet_tile_span``, one per tile; ``order`` int32, for tile t at ``order[first : first + count]`` the indices of the cells
    whose rectangle (x0, y0, rw, rh) intersects it, ascending — the table's order is the paste order; ``first`` is the exclusive prefix sum of
    ``count``.  An empty rectangle touches no tile; a rectangle is clipped to the page.  ValueError for a page of more than 2^31 − 1 tiles and for
    an order longer than that.  The (tile, cell) pairs are generated cell by cell and sorted by tile with a stable sort: no loop over tiles."""
    cells = np.asarray(cells)
    page_h, page_w = int(page_h), int(page_w)
    if page_h < 1 or page_w < 1:
        raise ValueError("bin_tiles: empty page (%d x %d)" % (page_w, page_h))
    tiles_x, tiles_y = -(-page_w // TILE_W), -(-page_h // TILE_H)
    n_tiles = tiles_x * tiles_y
    if n_tiles > MAX_TILES:
        raise ValueError("bin_tiles: a %d x %d page has %d tiles, more than %d" % (page_w, page_h, n_tiles, MAX_TILES))
    x0, y0 = cells["x0"].astype(np.int64), cells["y0"].astype(np.int64)
    x1, y1 = np.minimum(x0 + cells["rw"], page_w), np.minimum(y0 + cells["rh"], page_h)
    x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
    tx0, ty0, tx1, ty1 = x0 // TILE_W, y0 // TILE_H, -(-x1 // TILE_W), -(-y1 // TILE_H)       # the tiles [tx0, tx1) x [ty0, ty1)
    per_cell = np.where((x1 > x0) & (y1 > y0), (tx1 - tx0) * (ty1 - ty0), 0)
    total = int(per_cell.sum())
    if total > MAX_TILES:
        raise ValueError("bin_tiles: the cells touch %d tiles in all, an order longer than %d" % (total, MAX_TILES))
    tiles = [(np.arange(ty0[c], ty1[c])[:, None] * tiles_x + np.arange(tx0[c], tx1[c])[None, :]).reshape(-1) for c in np.flatnonzero(per_cell)]
    tile = np.concatenate(tiles) if tiles else np.zeros((0,), np.int64)
    cell = np.repeat(np.arange(len(cells), dtype=np.int32), per_cell)                             # the pairs, in cell order
    order = np.ascontiguousarray(cell[np.argsort(tile, kind="stable")])
    count = np.bincount(tile, minlength=n_tiles)
    spans = np.zeros((n_tiles,), dtype=np.dtype(_lib.TileSpan))
    spans["count"] = count
    spans["first"] = np.cumsum(count) - count
    return spans, order


def paste_ordered(out, joined, cells):
    """``out``: the enlarged page on the device, changed IN PLACE; ``joined``: uint8 BGR [L, rows, line_w, 3] on the device; ``cells``: a record
    array of ``mnet_column_paste`` (``as_cell`` of ``build_table``'s regions, ``columns.paste_table``'s cells), pasted in the table's order wherever
    they overlap: the bytes of ``paste_host`` / ``columns.paste_column_host`` applied one after another.  One copy each of the table, the spans and
    the order, and ONE launch whose workgroups are the page's tiles."""
    if len(cells):
        spans, order = bin_tiles(cells, int(out.shape[0]), int(out.shape[1]))
        with ops.on_device(out):
            ops.paste_ordered_u8(joined, ops.table_to_device(cells, out.device), ops.table_to_device(spans, out.device),
                                 torch.from_numpy(order).to(out.device), out)
    return out


def enlarge(page_d, s):
    """``lq_io.resize_cubic(page, s, s)`` of a page on the device, bit for bit (``mnet_lq_from_u8``'s preview form) → uint8 RGB [s·H, s·W, 3]: one copy
    of the descriptor, one launch"""
    H, W = int(page_d.shape[0]), int(page_d.shape[1])
    desc = np.zeros((1,), dtype=np.dtype(_lib.LqImage))
    desc[0] = (0, H, W, s * W, 0, 1.0 / s)
    with ops.on_device(page_d):
        return ops.lq_from_u8(page_d.reshape(-1), ops.table_to_device(desc, page_d.device), s * H, s * W, preview=True)[0]


def page_to_device(who, page, joined, out_ws, device, check):
    """the intake of ``compose_page`` and ``quads.compose_page_quads``, which ``who`` names in the messages.  ``page``: uint8 RGB [H, W, 3], a host
    array (copied once) or a device tensor (TypeError otherwise); ``joined`` / ``out_ws`` as ``compose_page`` takes them; ``check(H, W, rows)``: the
    caller's own refusals → (its records of the regions, their heights in the enlarged page).  ValueError for lines that do not match the widths, a
    width outside its line, rows the region's box factor does not divide, and a host page without lines or device — every refusal before anything
    is copied.  → (the page on the device, rows, the records)"""
    host = not torch.is_tensor(page)
    if host:
        page = torch.from_numpy(np.ascontiguousarray(_page_array(page)))
    elif page.dtype != torch.uint8 or page.dim() != 3 or page.shape[2] != 3 or page.numel() == 0:
        raise TypeError("uint8 RGB HxWx3 page expected")
    n_live = sum(w is not None for w in out_ws)
    if n_live and (joined is None or joined.dim() != 4 or joined.shape[0] != n_live or joined.dtype != torch.uint8):
        raise ValueError("%s: one joined line per region with a width expected (%d widths, lines %s)"
                         % (who, n_live, None if joined is None else list(joined.shape)))
    rows = int(joined.shape[1]) if n_live else ROW_H
    records, heights = check(int(page.shape[0]), int(page.shape[1]), rows)
    for i, w in enumerate(out_ws):
        if w is not None and not 1 <= int(w) <= joined.shape[2]:
            raise ValueError("%s: region %d: line width %d outside [1, %d]" % (who, i, int(w), joined.shape[2]))
        if w is not None and rows % box_factor(heights[i], rows):
            raise ValueError("%s: region %d: lines of %d rows cannot be box-reduced by %d" % (who, i, rows, box_factor(heights[i], rows)))
    if host:
        device = torch.device(device) if device is not None else joined.device if n_live else None
        if device is None:
            raise ValueError("%s: a device is needed for a host page without lines" % who)
        page = page.to(device)                                                             # the one copy of the pixels
    return page, rows, records


def compose_page(page, joined, out_ws, boxes, scale=4, feather=8, device=None, overlap="refuse"):
    """the device path of ``compose_host``.  ``page``: uint8 RGB [H, W, 3], a host array (copied once) or a device tensor; ``joined``: uint8 BGR
    [L, rows, line_w, 3] on the device, the lines of the regions that have one, in the regions' order (``long_lines.compose_lines``), or None where
    no region has one; ``out_ws[i]``: the width of region i's line, None for a region that keeps the background; ``boxes[i]``: its integer box.
    → uint8 RGB [s·H, s·W, 3] on the device.  Every refusal of ``compose_host`` is raised before anything is copied or launched; then one copy of
    the page and one of each small table (the background's descriptor, the regions), one launch for the background and one for all regions.
    ``overlap="order"``: overlapping regions are pasted in list order, by one ``mnet_paste_ordered_u8`` launch over the same regions as cells
    (``paste_ordered``) — overlap-free pages too, so that the mode has one path."""
    ordered = check_overlap(overlap)

    def check(H, W, rows):
        rects = region_rects(H, W, boxes, [w is not None for w in out_ws], scale, feather, rows, overlap)
        return rects, [r[3] for r in rects]
    page, rows, rects = page_to_device("compose_page", page, joined, out_ws, device, check)
    if ordered:
        return paste_ordered(enlarge(page, int(scale)), joined, as_cell(build_table(rects, out_ws, feather, rows)))
    return paste_rects(enlarge(page, int(scale)), joined, rects, out_ws, feather)
