"""A page whose text regions are of ANY kind and may lie over one another: a seal stamped over the text lines, a slanted stamp across a table, a
sign's column beside a rotated line.  ``pages``, ``columns``, ``quads`` and ``curves`` each state one kind of region; this module states a page
that mixes them, with nothing new per pixel, and returns the same bytes from the device:

    region_kind, normalize_regions    a region is a dict with exactly one of "box" ([x1, y1, x2, y2], optionally "vertical": True), "quad" (four
                                      points) and "polygon" (2K points); every kind's own refusals, then ONE cross-kind overlap rule
    compose_regions_host              the pure-host definition of a page: the existing host paste of each region's kind, in list order
    mixed_tables, bin_items,          the same bytes on the device: one table per kind, one item per thing to paste, the items of every 64 x 16
    paste_regions                     tile of the page, one ``mnet_paste_u8`` launch (feather 0) for the upright foregrounds of all quadrilaterals
                                      and curves, and ONE ``mnet_paste_mixed_u8`` launch whose workgroups own page tiles

Overlap is ``pages``' (its head states painter's order, for every kind).  The cross-kind rule of ``overlap="refuse"``: every region is a list of
convex polygons — a box or a quadrilateral is one, a curve is its chain's quadrilaterals — and two restored regions overlap where their
(unclipped) bounding boxes intersect and some pair of their pieces is not separated by an edge (``curves._boxes_apart``, ``quads._separated``:
regions that only touch do not overlap).  ``MarconetPipeline.restore_page_regions`` ties it to the networks.  Out of scope: any blend of
overlapping regions other than painter's order, vertical columns that are rotated or curved, detection and recognition, several pages per launch.
"""
import numpy as np
import torch

from . import _lib, columns, curves, lq_io, ops, pages, quads

ROW_H = pages.ROW_H
SHAPE_KEYS = ("box", "quad", "polygon")


def region_kind(region, i):
    """``region``: a dict with exactly one of "box", "quad", "polygon" → "line", "column" (a box with a true "vertical"), "quad" or "curve";
    ValueError naming region ``i`` otherwise, and for "vertical" beside a quadrilateral or a polygon"""
    keys = [k for k in SHAPE_KEYS if isinstance(region, dict) and k in region]
    if len(keys) != 1:
        raise ValueError('region %d: exactly one of "box", "quad" and "polygon" expected, got %s' % (i, keys if keys else repr(region)))
    if keys[0] != "box" and region.get("vertical"):
        raise ValueError('region %d: "vertical" applies to a "box" only (a column is an upright box), not to a "%s"' % (i, keys[0]))
    return {"box": "column" if region.get("vertical") else "line", "quad": "quad", "polygon": "curve"}[keys[0]]


def _renamed(i, fn, *args, **kw):
    """``fn`` checks ONE region, which it calls region 0: its refusal names region ``i``"""
    try:
        return fn(*args, **kw)
    except ValueError as e:
        msg = str(e)
        raise ValueError("region %d:%s" % (i, msg[len("region 0:"):]) if msg.startswith("region 0:") else msg) from None


def normalize_regions(page_h, page_w, regions, restored, texts=None, char_boxes=None, scale=4, feather=8, overlap="refuse", rows=ROW_H, cuts=None):
    """the refusals, all ValueError naming the region, and per region a record (a dict with ``kind`` and ``pieces``, its convex polygons in page
    pixels).  Every kind is checked by its own module, one region at a time, so that none of their pairwise tests runs:
        "line"     ``box`` (``pages.round_box``), ``rect`` (``pages.region_rects``)
        "column"   the same and, where it is restored, ``cuts`` (``cuts[i]`` if given, else ``columns.cell_cuts`` for ``len(texts[i])`` characters
                   and ``char_boxes[i]``) and ``widths`` (``columns.cell_widths``), checked by ``columns.check_columns``
        "quad"     ``quads.check_quads``' record
        "curve"    ``curves.check_curves``' record
    ``restored[i]``: region i has a line to paste.  Then the cross-kind rule of this module's head: with ``overlap="refuse"`` two restored regions
    whose interiors intersect are refused, both named; with ``"order"`` nothing is refused pairwise and every other refusal stands."""
    ordered = pages.check_overlap(overlap)
    pages.check_request(scale, feather, len(regions), len(restored), "region", "regions")
    page_h, page_w, out = int(page_h), int(page_w), []
    for i, region in enumerate(regions):
        kind, live = region_kind(region, i), bool(restored[i])
        if kind in ("line", "column"):
            try:
                box = pages.round_box(region["box"], page_h, page_w)
            except (TypeError, ValueError):
                raise ValueError("region %d: a box [x1, y1, x2, y2] expected, got %r" % (i, region["box"])) from None
            rec = dict(kind=kind, box=box, pieces=[[(float(x), float(y)) for x, y in quads.box_quad(box)]])
            rec["rect"] = _renamed(i, pages.region_rects, page_h, page_w, [box], [live], scale, feather, rows, "order")[0]
            if kind == "column" and live:
                if cuts is not None and cuts[i] is not None:
                    rec["cuts"] = [int(c) for c in cuts[i]]
                else:
                    if texts is None:
                        raise ValueError("region %d: a column's cells need its text (one cell per character) or its cuts" % i)
                    rec["cuts"] = columns.cell_cuts(box, len(texts[i]), None if char_boxes is None else char_boxes[i], region=i)
                _renamed(i, columns.check_columns, page_h, page_w, [box], [True], [rec["cuts"]], scale, feather, rows, "order")
                rec["widths"] = columns.cell_widths(box, rec["cuts"])
        elif kind == "quad":
            rec = dict(_renamed(i, quads.check_quads, page_h, page_w, [region["quad"]], [live], scale, feather, rows)[0], kind=kind)
            rec["pieces"] = [rec["quad"]]
        else:
            rec = dict(_renamed(i, curves.check_curves, page_h, page_w, [region["polygon"]], [live], scale, feather, rows)[0], kind=kind)
            rec["pieces"] = rec["quads"]
        out.append(rec)
    alive = [] if ordered else [i for i in range(len(regions)) if restored[i]]
    points = {i: [p for piece in out[i]["pieces"] for p in piece] for i in alive}
    for n, i in enumerate(alive):
        for j in alive[:n]:
            if not curves._boxes_apart(points[i], points[j]) and any(not quads._separated(p, q) for p in out[i]["pieces"] for q in out[j]["pieces"]):
                raise ValueError('regions %d and %d overlap (a %s and a %s): overlap="order" pastes them in list order' % (j, i, out[j]["kind"], out[i]["kind"]))
    return out


def paste_region_host(page_up, line_bgr, rec, feather):
    """the existing host paste of the record's kind, unchanged: ``page_up`` is changed IN PLACE and returned"""
    kind, F = rec["kind"], int(feather)
    if kind == "line":
        return pages.paste_host(page_up, line_bgr, rec["rect"], F)
    if kind == "column":
        return columns.paste_column_host(page_up, line_bgr, rec["rect"], rec["cuts"], rec["widths"], F)
    fg = pages.line_to_rect(line_bgr, rec["rw"], rec["rh"])
    if kind == "quad":
        return quads.warp_paste_host(page_up, fg, quads.inverse_map(quads.quad_map(rec["out_quad"], rec["rw"], rec["rh"])), rec["rw"], rec["rh"], F)
    return curves.warp_paste_host(page_up, fg, rec["out_segs"], rec["rw"], rec["rh"], F)


def compose_regions_host(page, lines, regions, texts=None, char_boxes=None, scale=4, feather=8, overlap="refuse", cuts=None):
    """the definition of a page: ``page`` uint8 RGB [H, W, 3]; ``regions[i]`` a region dict; ``lines[i]``: its restored line, uint8 BGR
    [rows, w, 3] — ``MarconetPipeline.restore_lines`` of the crop its kind defines — or None for a region that keeps the background; a column's
    cells come from ``cuts[i]`` or from ``texts[i]`` / ``char_boxes[i]`` (``normalize_regions``) → uint8 RGB [s·H, s·W, 3]:
    ``lq_io.resize_cubic(page, s, s)``, then in list order ``pages.paste_host``, ``columns.paste_column_host``, ``quads.warp_paste_host`` or
    ``curves.warp_paste_host`` of every line, the last two with ``pages.line_to_rect`` of the line as their foreground.  A page of one kind without
    overlaps gives the bytes of that kind's own ``compose_*_host``."""
    page = pages._page_array(page)
    rows = next((int(np.shape(l)[0]) for l in lines if l is not None), ROW_H)
    recs = normalize_regions(page.shape[0], page.shape[1], regions, [l is not None for l in lines], texts, char_boxes, scale, feather, overlap, rows, cuts)
    out = lq_io.resize_cubic(page, int(scale), int(scale))
    for line, rec in zip(lines, recs):
        if line is not None:
            paste_region_host(out, line, rec, feather)
    return out


# ------------------------------------------------------------------------------------------------------------------- the device path
def mixed_tables(recs, out_ws, feather, rows=ROW_H, line_index=None):
    """``recs``: ``normalize_regions``' records; ``out_ws[i]``: the width of region i's joined line, None where it keeps the background; the l-th
    region with a line reads line ``line_index[l]`` (default l) → a dict of numpy record arrays and the atlas' layout:
        ``cells``     ``mnet_column_paste``: a line as ``pages.as_cell`` of ``pages.build_table``'s record, a column as ``columns.paste_table``'s cells
        ``quads``     ``quads.paste_table`` of the quadrilaterals          ``curves``, ``segs``    ``curves.paste_table`` of the curved regions
        ``items``     ``mnet_page_item``, in paste order: one per line, quadrilateral and curve, one per cell of a column (consecutive); the rectangle
                      is the cell's, or the region's clipped bounding box
        ``entries``, ``entry_item``   what ``bin_items`` bins: per item its rectangle, per curve instead one rectangle per segment box that is not
                      empty (a seal's ring leaves most of its bounding box empty), with the item each belongs to
        ``fg``        ``mnet_paste_region`` (``pages.build_table``, feather 0): the upright foregrounds of the quadrilaterals and curves, stacked
                      vertically in ONE atlas of ``atlas_hw`` = (Σ rh, max rw); None where there is none"""
    live = [i for i, w in enumerate(out_ws) if w is not None]
    line_of = {i: (l if line_index is None else int(line_index[l])) for l, i in enumerate(live)}
    warped = [i for i in live if recs[i]["kind"] in ("quad", "curve")]
    fg_rects, atlas_hw = pages.atlas_layout([(r["rw"], r["rh"]) if i in warped else None for i, r in enumerate(recs)])
    qs, cs = [i for i in warped if recs[i]["kind"] == "quad"], [i for i in warped if recs[i]["kind"] == "curve"]
    quad_tab = quads.paste_table([recs[i] for i in qs], feather, [fg_rects[i][:2] for i in qs])
    curve_tab, seg_tab = curves.paste_table([recs[i] for i in cs], feather, [fg_rects[i][:2] for i in cs])
    cell_parts, items, entries, entry_item, n_cells = [], [], [], [], 0
    for i in live:
        r, kind = recs[i], recs[i]["kind"]
        if kind in ("line", "column"):
            part = columns.region_cells(line_of[i], r["rect"], out_ws[i] if kind == "line" else (r["box"], r["cuts"], r["widths"], None), feather, rows)
            for c in part:
                rect = (int(c["x0"]), int(c["y0"]), int(c["rw"]), int(c["rh"]))
                entries.append(rect)
                entry_item.append(len(items))
                items.append((_lib.ITEM_CELL, n_cells) + rect)
                n_cells += 1
            cell_parts.append(part)
        elif kind == "quad":
            entries.append(tuple(r["bbox"]))
            entry_item.append(len(items))
            items.append((_lib.ITEM_QUAD, qs.index(i)) + tuple(r["bbox"]))
        else:
            boxes = [s["box"] for s in r["out_segs"] if s["box"][2] > 0 and s["box"][3] > 0]
            entries.extend(tuple(int(v) for v in b) for b in boxes)
            entry_item.extend([len(items)] * len(boxes))
            items.append((_lib.ITEM_CURVE, cs.index(i)) + tuple(r["bbox"]))
    item_dt = np.dtype(_lib.PageItem)
    item_tab, entry_tab = np.zeros((len(items),), dtype=item_dt), np.zeros((len(entries),), dtype=item_dt)
    for n, it in enumerate(items):
        item_tab[n] = it
    for n, e in enumerate(entries):
        entry_tab[n] = (0, 0) + e
    fg = None
    if warped:
        fg = pages.build_table(fg_rects, [out_ws[i] if i in warped else None for i in range(len(recs))], 0, rows, [line_of[i] for i in warped])
    return dict(cells=np.concatenate(cell_parts) if cell_parts else np.zeros((0,), dtype=np.dtype(_lib.ColumnPaste)), quads=quad_tab, curves=curve_tab,
                segs=seg_tab, items=item_tab, entries=entry_tab, entry_item=np.asarray(entry_item, dtype=np.int32), fg=fg,
                atlas_hw=atlas_hw)


def bin_items(entries, entry_item, page_h, page_w):
    """the items of every 64 x 16 tile of the page → (spans, order) as ``pages.bin_tiles`` gives them for cells: ``entries`` (a record array with
    ``x0``, ``y0``, ``rw``, ``rh``) are binned by ``pages.bin_tiles`` as they are; entry n stands for item ``entry_item[n]`` (ascending, an item's
    entries consecutive), and an item that several of its entries bring to one tile is listed there once.  No loop over tiles."""
    spans, order = pages.bin_tiles(entries, page_h, page_w)
    entry_item = np.asarray(entry_item, dtype=np.int32)
    if len(entry_item) != len(entries) or (len(entry_item) > 1 and (np.diff(entry_item) < 0).any()):
        raise ValueError("bin_items: one item per entry, ascending, expected")
    item = entry_item[order]
    tile = np.repeat(np.arange(len(spans), dtype=np.int64), spans["count"])
    keep = np.ones((len(item),), bool)
    keep[1:] = (item[1:] != item[:-1]) | (tile[1:] != tile[:-1])                 # within a tile the entries ascend, so an item's duplicates are neighbours
    count = np.bincount(tile[keep], minlength=len(spans))
    spans = np.zeros((len(spans),), dtype=np.dtype(_lib.TileSpan))
    spans["count"] = count
    spans["first"] = np.cumsum(count) - count
    return spans, np.ascontiguousarray(item[keep].astype(np.int32))


def paste_tables(out, joined, tabs):
    """``out``: the enlarged page on the device, changed IN PLACE; ``joined``: uint8 BGR [L, rows, line_w, 3] on the device; ``tabs``:
    ``mixed_tables``' result.  One copy of each table that is not empty, one ``mnet_paste_u8`` launch (feather 0) for the atlas where a
    quadrilateral or a curve is live, and ONE ``mnet_paste_mixed_u8`` launch."""
    if not len(tabs["items"]):
        return out
    spans, order = bin_items(tabs["entries"], tabs["entry_item"], int(out.shape[0]), int(out.shape[1]))
    if not len(order):
        return out
    dev = out.device
    up = lambda t: ops.table_to_device(t, dev) if len(t) else None
    with ops.on_device(out):
        atlas = None if tabs["fg"] is None else pages.fill_atlas(joined, tabs["fg"], tabs["atlas_hw"])
        ops.paste_mixed_u8(joined if len(tabs["cells"]) else None, atlas, up(tabs["cells"]), up(tabs["quads"]), up(tabs["curves"]), up(tabs["segs"]),
                           ops.table_to_device(tabs["items"], dev), ops.table_to_device(spans, dev), torch.from_numpy(order).to(dev), out)
    return out


def paste_regions(out, joined, out_ws, recs, feather, line_index=None):
    """``paste_tables`` of ``mixed_tables(recs, out_ws, feather, rows of joined, line_index)``: ``paste_region_host``'s bytes, region after region"""
    if all(w is None for w in out_ws):
        return out
    return paste_tables(out, joined, mixed_tables(recs, out_ws, feather, int(joined.shape[1]), line_index))


def compose_page_regions(page, joined, out_ws, regions, texts=None, char_boxes=None, scale=4, feather=8, device=None, overlap="refuse", cuts=None):
    """the device path of ``compose_regions_host``; the arguments are ``pages.compose_page``'s, with region dicts in the place of the boxes.
    → uint8 RGB [s·H, s·W, 3] on the device.  Every refusal of ``compose_regions_host`` is raised before anything is copied or launched; both
    overlap modes compose through ``mnet_paste_mixed_u8``, so the mode has one path."""
    def check(H, W, rows):
        recs = normalize_regions(H, W, regions, [w is not None for w in out_ws], texts, char_boxes, scale, feather, overlap, rows, cuts)
        hs = []
        for r in recs:                          # the height the box factor is taken of; a column's cells each have their own: the lowest decides
            if "cuts" in r:
                hs.append(min(int(scale) * (b - a) for a, b in zip(r["cuts"][:-1], r["cuts"][1:])))
            else:
                hs.append(r["rect"][3] if "rect" in r else r["rh"])
        return recs, hs
    page, rows, recs = pages.page_to_device("compose_page_regions", page, joined, out_ws, device, check)
    return paste_regions(pages.enlarge(page, int(scale)), joined, out_ws, recs, int(feather))
