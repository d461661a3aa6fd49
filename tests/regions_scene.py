"""The small scene the tests of the mixed page compositor share (tests/test_regions.py for the binning, tests/test_regions_gpu.py for the kernel):
a 150 x 70 page — 3 x 5 tiles of 64 x 16 —, five lines of 16 rows x 96 columns, and things of every kind laid over one another, each with its own
feather.  Every thing knows its descriptors (built by the modules' own table builders; a column's cells by hand, because ``columns`` needs lines
of at least 32 rows) and its host paste, which is the existing host paste of its kind."""
import math

import numpy as np

from marconet_amd import _lib, curves, pages, quads

PAGE_H, PAGE_W, ROWS, N_LINES, LINE_W = 70, 150, 16, 5, 96


def arc(cx, cy, r_in, r_out, deg0, deg1, K):
    a = [math.radians(d) for d in np.linspace(deg0, deg1, K)]
    top = [(cx + r_out * math.cos(t), cy - r_out * math.sin(t)) for t in a]
    bot = [(cx + r_in * math.cos(t), cy - r_in * math.sin(t)) for t in a]
    return top + bot[::-1]


# tests/test_curves_gpu.py's tapered chain (a1 changes sign inside its first segment), moved into this page
TAPERED = [(x - 60.0, y - 48.0) for x, y in [(163.5, 85.75), (169.35, 86.35), (177.5, 88.0), (187.5, 108.0), (172.25, 110.0), (158.5, 116.0)]]
TWIN = [(5, 50), (40, 48), (41, 62), (6, 64)]


def line(rect, li, src_w, F, page_h=PAGE_H, page_w=PAGE_W):
    return dict(kind="line", rect=tuple(rect), li=li, src_w=src_w, F=F)


def column(rect, heights, slices, li, F):
    assert sum(heights) == rect[3] and len(heights) == len(slices)
    return dict(kind="column", rect=tuple(rect), heights=list(heights), slices=list(slices), li=li, F=F)


def quad(points, li, src_w, F, page_h=PAGE_H, page_w=PAGE_W):
    return dict(kind="quad", rec=quads.check_quads(page_h, page_w, [points], [True], 1, F, ROWS)[0], li=li, src_w=src_w, F=F)


def curve(points, li, src_w, F, page_h=PAGE_H, page_w=PAGE_W):
    return dict(kind="curve", rec=curves.check_curves(page_h, page_w, [points], [True], 1, F, ROWS)[0], li=li, src_w=src_w, F=F)


def scene():
    """the things in paste order: see the comments"""
    return [
        line((10, 5, 100, 40), 0, 96, 40),                                         # 0 a large line across the tile column 63|64 and the tile row 15|16
        quad([(30, 12), (95, 20), (92, 36), (27, 28)], 1, 80, 1),                  # 1 a rotated quad over it
        curve(arc(64.0, 60.0, 22.0, 38.0, 160.0, 20.0, 7), 2, 96, 3),              # 2 a 6-segment arc over both: three kinds, three deep in tile (0, 1)
        curve(arc(118.0, 66.0, 8.0, 20.0, 170.0, 10.0, 33), 3, 90, 0),             # 3 a 32-segment arc
        quad([(135, 4), (160, 8), (158, 20), (133, 16)], 4, 70, 3),                # 4 clipped by the page's right edge
        column((88, 40, 12, 28), (9, 10, 9), ((0, 30), (30, 61), (61, 96)), 0, 1),  # 5 a column of three cells under the arc's end
        line((50, 14, 1, 20), 1, 40, 0),                                           # 6 a 1-pixel-wide cell over the quad
        quad(TWIN, 2, 96, 3),                                                      # 7, 8 two identical quads, the second with feather 0
        quad(TWIN, 3, 77, 0),
        curve(TAPERED, 4, 96, 3),                                                  # 9 the tapered chain
    ]


def data(seed=11):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8), rng.integers(0, 256, (N_LINES, ROWS, LINE_W, 3), dtype=np.uint8)


def paste_host(out, lines, t):
    """the existing host paste of the thing's kind; ``out`` is changed in place"""
    src = lines[t["li"]]
    if t["kind"] == "line":
        return pages.paste_host(out, src[:, :t["src_w"]], t["rect"], t["F"])
    if t["kind"] == "column":                                # columns.paste_column_host's definition: the cells' foregrounds stacked, ONE blend over the column
        x0, y0, rw, rh = t["rect"]
        fg = np.vstack([pages.line_to_rect(src[:, a:b], rw, h) for h, (a, b) in zip(t["heights"], t["slices"])])
        view = out[y0:y0 + rh, x0:x0 + rw]
        view[...] = pages.feather_blend(view, fg, t["F"])
        return out
    r = t["rec"]
    fg = pages.line_to_rect(src[:, :t["src_w"]], r["rw"], r["rh"])
    if t["kind"] == "quad":
        return quads.warp_paste_host(out, fg, quads.inverse_map(quads.quad_map(r["out_quad"], r["rw"], r["rh"])), r["rw"], r["rh"], t["F"])
    return curves.warp_paste_host(out, fg, r["out_segs"], r["rw"], r["rh"], t["F"])


def host(page, lines, things):
    out = page.copy()
    for t in things:
        paste_host(out, lines, t)
    return out


def column_cells(t):
    x0, y0, rw, rh = t["rect"]
    tab = np.zeros((len(t["heights"]),), dtype=np.dtype(_lib.ColumnPaste))
    y = y0
    for j, (h, (a, b)) in enumerate(zip(t["heights"], t["slices"])):
        k = pages.box_factor(h, ROWS)
        tab[j] = (t["li"], a, b - a, x0, y, rw, h, t["F"], k, x0, y0, rw, rh, 0, pages.axis_scale(rw, -(-(b - a) // k)), pages.axis_scale(h, ROWS // k))
        y += h
    return tab


def tables(things):
    """→ the dict ``regions.mixed_tables`` gives, for things with their own feathers"""
    cells, quad_tabs, curve_tabs, seg_tabs, items, entries, entry_item, fg_rects, fg_ws, fg_li = [], [], [], [], [], [], [], [], [], []
    n_cells = n_quads = n_curves = n_segs = y = 0
    for t in things:
        if t["kind"] in ("line", "column"):
            part = column_cells(t) if t["kind"] == "column" else pages.as_cell(pages.build_table([t["rect"]], [t["src_w"]], t["F"], ROWS, [t["li"]]))
            for c in part:
                rect = (int(c["x0"]), int(c["y0"]), int(c["rw"]), int(c["rh"]))
                entries.append(rect)
                entry_item.append(len(items))
                items.append((_lib.ITEM_CELL, n_cells) + rect)
                n_cells += 1
            cells.append(part)
            continue
        r = t["rec"]
        fg_rects.append((0, y, r["rw"], r["rh"]))
        fg_ws.append(t["src_w"])
        fg_li.append(t["li"])
        if t["kind"] == "quad":
            quad_tabs.append(quads.paste_table([r], t["F"], [(0, y)]))
            entries.append(tuple(r["bbox"]))
            entry_item.append(len(items))
            items.append((_lib.ITEM_QUAD, n_quads) + tuple(r["bbox"]))
            n_quads += 1
        else:
            tab, segs = curves.paste_table([r], t["F"], [(0, y)])
            tab["seg0"] += n_segs
            curve_tabs.append(tab)
            seg_tabs.append(segs)
            boxes = [tuple(int(v) for v in s["box"]) for s in r["out_segs"] if s["box"][2] > 0 and s["box"][3] > 0]
            entries.extend(boxes)
            entry_item.extend([len(items)] * len(boxes))
            items.append((_lib.ITEM_CURVE, n_curves) + tuple(r["bbox"]))
            n_curves += 1
            n_segs += len(segs)
        y += r["rh"]

    def cat(parts, struct):
        return np.concatenate(parts) if parts else np.zeros((0,), dtype=np.dtype(struct))
    item_dt = np.dtype(_lib.PageItem)
    item_tab, entry_tab = np.zeros((len(items),), dtype=item_dt), np.zeros((len(entries),), dtype=item_dt)
    for n, it in enumerate(items):
        item_tab[n] = it
    for n, e in enumerate(entries):
        entry_tab[n] = (0, 0) + e
    return dict(cells=cat(cells, _lib.ColumnPaste), quads=cat(quad_tabs, _lib.QuadRegion), curves=cat(curve_tabs, _lib.CurveRegion),
                segs=cat(seg_tabs, _lib.CurveSeg), items=item_tab, entries=entry_tab, entry_item=np.asarray(entry_item, dtype=np.int32),
                fg=pages.build_table(fg_rects, fg_ws, 0, ROWS, fg_li) if fg_rects else None, atlas_hw=(y, max([r[2] for r in fg_rects], default=0)))
