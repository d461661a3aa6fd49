"""Finding a page's text lines: a recursive XY-cut over ink profiles.  The page entry points take their regions from the caller; for a scan of
horizontal lines in one or more columns on plain paper the boxes can be measured from the pixels without a model — a box is cut where its row
profile, then its column profile, has a blank run, and the pieces are cut again until nothing changes.  This module is the pure-host definition,
numpy and integers only; ``MarconetPipeline.find_lines`` is the device path — the profiles of every pass from ONE ``mnet_box_ink_u8`` launch — and
returns exactly this (tests/test_layout_gpu.py compares the two with ``==``).  It never raises on any uint8 RGB page.

The rules:

    box_ink           ``ink.box_ink`` (``ink``'s head defines Y, d and e): rows[r] = Σ_{x = 0 .. w − 2} e(x, r);  cols[x] = Σ_{r = 0 .. h − 1} e(x, r)
                      for x <= w − 2, cols[w − 1] = 0: a pair is filed under its LEFT pixel.  Exact integers: ``mnet_box_ink_u8`` returns both
                      with ==.  With floor <= 1 ``rows`` is ``blind_columns.row_ink``.
    cut               an entry of a profile is blank iff it is 0.  The blank ends are trimmed; the rest is split at every inner blank run of
                      ``min_gap`` entries or more → half-open segments [a, b); an all-blank profile → [].  For the Y axis the profile is ``rows``.
                      For the X axis it is the PIXEL profile c[x] = cols[x − 1] + cols[x] (cols[−1] = 0): an edge keeps both of its pixels, so a
                      found box includes the background pixel on either side of its outermost vertical edges — and a pair that straddles a
                      box's side is blank over the box's rows.
    xy_cut            from the page as one box, passes alternate: Y with gap_y = max(1, text_h // 8) — between two lines any blank row cuts —,
                      then X with gap_x = 2 text_h — a gutter cuts, the space between two words does not.  In a pass every box is replaced,
                      in place in the list, by its segments; an all-blank box vanishes.  It stops after two consecutive passes that change
                      nothing (one of each axis) or after ``max_passes``.  List order is reading order, depth first: bands top to bottom, blocks
                      left to right inside a band, lines top to bottom inside a block.
    allowances        every box carries four, (left, top, right, bottom): the count of blank pixels outside that side that belong to the box
                      alone.  Two siblings separated by a blank run of L get L // 2 each; an outermost child gets what was trimmed on that side
                      plus its parent's allowance there; across the cut axis a child inherits its parent's; the page has 0.  A box grown by at
                      most its allowances stays inside the page and can never meet another.
    find_lines_host   text_h = max(8, page_h // 100) (a prior, as ``blind_columns``' square cell is one); min_h = max(2, text_h // 4), min_w =
                      max(2, text_h // 2), max_h = 4 text_h, pad = text_h // 4.  After the cut the boxes under min_h or min_w are dropped (specks,
                      rules), the boxes taller than max_h go to ``skipped`` with the reason (a figure, or lines the cut could not part), and
                      every side of the others grows by min(pad, allowance).

Limits, stated and not solved here: the defaults are design choices, not measurements, and no claim of detection QUALITY is made.  Out of scope:
vertical columns, rotated or curved text, tables with vertical rules (every row has ink), text on textured backgrounds, real scans.  A page skewed
as a whole by up to about 7 degrees is ``skew``'s: the same cut in the coordinates of a sheared frame (``MarconetPipeline.find_lines_skewed``)."""
import numpy as np

from . import pages
from .ink import MAX_LAUNCH_BOXES, MAX_LAUNCH_TILES, box_ink, box_table as ink_table, launch_chunks, luma             # noqa: F401  (the profiles: ``ink``'s)

DEFAULT_FLOOR = 24
AXIS_Y, AXIS_X = 0, 1


# --------------------------------------------------------------------------------------------------------------------------- the profiles
def pixel_profile(cols):
    """c[x] = cols[x − 1] + cols[x]: the X axis' profile per PIXEL of a profile per pair"""
    cols = np.asarray(cols).astype(np.int64)
    c = cols.copy()
    c[1:] += cols[:-1]
    return c


# -------------------------------------------------------------------------------------------------------------------------------- the cut
def cut(profile, min_gap):
    """``profile``: non-negative integers, blank where 0 → the half-open segments [(a, b)] between its blank ends, split at every inner blank run
    of at least ``min_gap`` entries; [] for an all-blank (or empty) profile"""
    ink = np.flatnonzero(np.asarray(profile) != 0)
    if ink.size == 0:
        return []
    min_gap = max(1, int(min_gap))
    breaks = np.flatnonzero(np.diff(ink) - 1 >= min_gap)                   # ink[k] and ink[k + 1] lie a blank run of >= min_gap apart
    firsts = [int(ink[0])] + [int(ink[k + 1]) for k in breaks]
    lasts = [int(ink[k]) for k in breaks] + [int(ink[-1])]
    return [(a, b + 1) for a, b in zip(firsts, lasts)]


def _children(box, allow, segs, axis):
    """the boxes and allowances of the segments ``segs`` of ``box`` along ``axis`` (the module's head: allowances)"""
    lo, hi = (box[1], box[3]) if axis == AXIS_Y else (box[0], box[2])
    near, far = (1, 3) if axis == AXIS_Y else (0, 2)
    out = []
    for k, (a, b) in enumerate(segs):
        child, al = list(box), list(allow)
        child[near], child[far] = lo + a, lo + b
        al[near] = a + allow[near] if k == 0 else (a - segs[k - 1][1]) // 2
        al[far] = (hi - lo - b) + allow[far] if k == len(segs) - 1 else (segs[k + 1][0] - b) // 2
        out.append((child, al))
    return out


def xy_cut(profiles, page_h, page_w, text_h, max_passes=8, start=None):
    """the recursive XY-cut (the module's head states it).  ``profiles(boxes, axis)``: per box of ``boxes`` its ``rows`` (``axis`` 0) or its ``cols``
    (``axis`` 1) as ``box_ink`` defines them — the one thing the host and the device paths do not share; it is not called with an empty list.
    → (boxes [[x1, y1, x2, y2]] in reading order, their allowances [[left, top, right, bottom]], the passes that ran).  ``start``: (boxes,
    allowances) to start from instead of the page — the result of an earlier call comes back unchanged after 2 passes."""
    text_h = max(1, int(text_h))
    gaps = (max(1, text_h // 8), 2 * text_h)
    if start is None:
        boxes, allows = ([[0, 0, int(page_w), int(page_h)]], [[0, 0, 0, 0]]) if page_h >= 1 and page_w >= 1 else ([], [])
    else:
        boxes, allows = [list(b) for b in start[0]], [list(a) for a in start[1]]
    passes, unchanged = 0, 0
    while passes < int(max_passes) and unchanged < 2:
        axis = passes % 2
        profs = profiles(boxes, axis) if boxes else []
        new_boxes, new_allows = [], []
        for box, allow, prof in zip(boxes, allows, profs):
            for child, al in _children(box, allow, cut(prof if axis == AXIS_Y else pixel_profile(prof), gaps[axis]), axis):
                new_boxes.append(child)
                new_allows.append(al)
        unchanged = unchanged + 1 if new_boxes == boxes else 0
        boxes, allows, passes = new_boxes, new_allows, passes + 1
    return boxes, allows, passes


# ------------------------------------------------------------------------------------------------------------------------------ the lines
def line_params(page_h, text_h=None, floor=DEFAULT_FLOOR, pad=None, min_h=None, min_w=None, max_h=None):
    """the arguments of ``find_lines_host`` with their defaults filled in (the module's head) → dict; ValueError for a ``floor`` outside 0..255,
    a ``text_h`` under 1 and a negative ``pad``, ``min_h``, ``min_w`` or ``max_h`` — the only refusals of the finding, raised before any pixel is read"""
    text_h = max(8, int(page_h) // 100) if text_h is None else text_h
    if int(text_h) != text_h or text_h < 1:
        raise ValueError("text_h must be an integer >= 1, got %r" % (text_h,))
    if int(floor) != floor or not 0 <= floor <= 255:
        raise ValueError("floor must be an integer in [0, 255], got %r" % (floor,))
    text_h = int(text_h)
    p = dict(text_h=text_h, floor=int(floor), pad=text_h // 4 if pad is None else pad, min_h=max(2, text_h // 4) if min_h is None else min_h,
             min_w=max(2, text_h // 2) if min_w is None else min_w, max_h=4 * text_h if max_h is None else max_h)
    for name in ("pad", "min_h", "min_w", "max_h"):
        if int(p[name]) != p[name] or p[name] < 0:
            raise ValueError("%s must be an integer >= 0, got %r" % (name, p[name]))
        p[name] = int(p[name])
    return p


def lines_from_profiles(profiles, page_h, page_w, params, frame=None):
    """``find_lines_host`` from ``xy_cut`` on: what the host and the device paths share.  ``params``: ``line_params``' dict.  ``frame``: the box the
    cut starts from instead of the page — ``skew``'s frame box, whose coordinates are the frame's; a box then grows by min(pad, allowance − 1),
    one pixel less a side (``skew``'s head says why)"""
    cut_boxes, allows, passes = xy_cut(profiles, page_h, page_w, params["text_h"], start=None if frame is None else ([list(frame)], [[0, 0, 0, 0]]))
    boxes, tight, skipped = [], [], []
    for b, al in zip(cut_boxes, allows):
        h, w = b[3] - b[1], b[2] - b[0]
        if h < params["min_h"] or w < params["min_w"]:
            continue
        if h > params["max_h"]:
            skipped.append(dict(box=list(b), reason="%d rows high, over max_h = %d: a figure, or lines the cut could not part" % (h, params["max_h"])))
            continue
        g = [min(params["pad"], a if frame is None else max(a - 1, 0)) for a in al]
        tight.append(list(b))
        boxes.append([b[0] - g[0], b[1] - g[1], b[2] + g[2], b[3] + g[3]])
    return dict(boxes=boxes, tight=tight, skipped=skipped, passes=passes)


def find_lines_host(page, text_h=None, floor=DEFAULT_FLOOR, pad=None, min_h=None, min_w=None, max_h=None):
    """the text lines of ``page`` (uint8 RGB [H, W, 3]) → dict(boxes: integer [x1, y1, x2, y2] in reading order, each grown by min(pad,
    allowance) a side; tight: the same boxes as cut; skipped: [dict(box, reason)], the boxes taller than ``max_h``; passes: the passes ``xy_cut``
    ran) — the definition of ``MarconetPipeline.find_lines`` (the module's head states the rules and the defaults)"""
    page = pages._page_array(page)
    params = line_params(page.shape[0], text_h, floor, pad, min_h, min_w, max_h)
    return lines_from_profiles(lambda boxes, axis: [box_ink(page, b, params["floor"])[axis] for b in boxes], int(page.shape[0]), int(page.shape[1]), params)
