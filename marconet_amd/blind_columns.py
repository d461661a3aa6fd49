"""Reading a vertical column blind: the text and the character boxes of a column of upright characters whose text is unknown.  ``columns`` cuts a
column's cells from its text, one per character; without a text the cells are measured from the column's pixels — the rows where its ink profile
dips — and the virtual strip of those first-pass cells (``columns.virtual_strip``) is an ordinary line 32 px high that the encoder reads through
probes of whole cells, as ``blind`` reads a wide line.  This module is the pure-host definition of that reading, fp64 and integers only;
``MarconetPipeline.read_columns`` is the device path and returns exactly this (tests/test_blind_columns_gpu.py compares the two with ``==``).

The rules:

    row_ink           ``ink.row_ink``: per row of the box its total horizontal variation of integer luma (``ink``'s head defines it).  An exact
                      integer: ``mnet_row_ink_u8`` returns it with ==.
    first_cuts        n = max(1, (2 ch + cw) // (2 cw)) cells, about square.  The cuts are found top to bottom, each relative to the one before
                      (a global grid drifts): with ``left`` cells to cut from the ``rem`` rows below c_{j−1}, the nominal cut is t = c_{j−1} +
                      rem / left rounded half up, and c_j is the row r within R = rem // (4 left) of t — and such that every cell above and below
                      keeps a row — whose two flanking rows hold the least ink, ink[r − 1] + ink[r]; ties go to the smallest |r − t|, then to
                      the smaller r.  A glyph's inner blank band lies more than a quarter pitch from where a cut is expected and cannot attract it.
    plan_cell_probes  A probe is a run of WHOLE cells (what ``columns.gather_table`` gathers): from cell g0 the longest run with Σ w_j <=
                      ``probe_width`` and at most ``probe_width // 32`` cells (12 square cells at the default: room in the encoder's 16 slots);
                      the next probe starts max(1, len // 2) cells later; the last one is the longest run that ends at the last cell.  A probe
                      OWNS the columns of the virtual strip up to the middle of its overlap with each neighbour, (c0_{k+1} + c1_k) // 2, as in
                      ``blind.plan_probes``.
    reading           ``blind.read_probe(..., probe=(c0, c1, own_lo, own_hi), h=32)`` per probe and ``blind.merge(32, Wv, reads)``, unchanged.
    strip_to_rows     a column x of the virtual strip → the page row t_j + (x − o_j) h_j / w_j of the cell j that holds it (x = Wv: the last
                      cell); a read character [xa, xb] becomes the box [x1, row(xa), x2, row(xb)] in page pixels.
    settle            makes the reading one the GIVEN path accepts: while ``columns.cell_cuts(box, n, char_boxes)`` has an empty cell or one
                      under rows / 16 output rows (16 s h_j < rows), the character whose cell is shortest is dropped (ties: the later one).
                      Total: it never raises.  An empty result skips the column.

Limits, stated and not solved here: the count n comes from the square-cell prior — with cell heights within ±5 % of the column's width every cut of
300 synthetic columns fell into the right gap; at ±12 % the cuts still snap but n is wrong for about 3 % of the columns —, so columns whose cells
are far from square are out of scope, as are rotated or curved columns and the QUALITY of the segmentation and of the reading (the checkpoint's).
"""
import math

import numpy as np
import torch

from . import blind, columns, lq_device, lq_io, pages
from .ink import luma, row_ink, row_table as ink_table                                # noqa: F401  (the profile: ``ink``'s)
from .long_lines import Window

LQ_H = columns.LQ_H
ROW_H = columns.ROW_H


def cell_count(box):
    """n = max(1, (2 ch + cw) // (2 cw)): ch / cw rounded half up — the square-cell prior"""
    x1, y1, x2, y2 = (int(v) for v in box)
    cw, ch = x2 - x1, y2 - y1
    if cw < 1 or ch < 1:
        raise ValueError("an empty column (%d x %d) has no cells" % (cw, ch))
    return max(1, (2 * ch + cw) // (2 * cw))


def first_cuts(box, ink):
    """the first-pass cells of a column of unknown text → n + 1 integer cuts from y1 to y2, strictly increasing (the module's head states the rule);
    ``ink``: the column's ``row_ink``, one value per row"""
    x1, y1, x2, y2 = (int(v) for v in box)
    n = cell_count(box)
    ink = [int(v) for v in ink]
    if len(ink) != y2 - y1:
        raise ValueError("a profile of %d rows expected for the column's %d..%d, got %d" % (y2 - y1, y1, y2, len(ink)))
    cuts = [y1]
    for j in range(1, n):
        left, rem = n - j + 1, y2 - cuts[-1]
        t = cuts[-1] + (2 * rem + left) // (2 * left)
        R = rem // (4 * left)
        lo, hi = max(t - R, cuts[-1] + 1), min(t + R, y2 - (n - j))
        best = None
        for r in range(lo, hi + 1):
            key = (ink[r - 1 - y1] + ink[r - y1], abs(r - t), r)
            if best is None or key < best:
                best = key
        cuts.append(best[2] if best is not None else min(max(t, cuts[-1] + 1), y2 - (n - j)))
    cuts.append(y2)
    return cuts


# --------------------------------------------------------------------------------------------------------------------------- the probes
def plan_cell_probes(widths, probe_width=384, region=None):
    """the probes of a virtual strip whose cells are ``widths`` wide → list of (g0, g1, c0, c1, own_lo, own_hi): cells [g0, g1), columns [c0, c1)
    of the strip, of which [own_lo, own_hi) are the probe's own (the module's head states the rules).  ValueError naming ``region`` for a single
    cell wider than ``probe_width``; ``blind.check_probe_width``'s for the width itself."""
    probe_width = blind.check_probe_width(probe_width)
    widths = [int(w) for w in widths]
    n, o, cap = len(widths), columns.cell_offsets(widths), probe_width // LQ_H
    if n < 1:
        raise ValueError("%sa column without a cell has no probes" % columns._who(region))
    for j, w in enumerate(widths):
        if w > probe_width or w < 1:
            raise ValueError("%sits cell is %d px wide at height %d: a probe of %d px cannot hold it" % (columns._who(region, j), w, LQ_H, probe_width))

    def run_from(g0):                                                      # the longest run of whole cells that starts at g0
        g1 = g0 + 1
        while g1 < n and g1 - g0 < cap and o[g1 + 1] - o[g0] <= probe_width:
            g1 += 1
        return g1

    runs, g0 = [], 0
    while run_from(g0) < n:
        runs.append((g0, run_from(g0)))
        g0 += max(1, (runs[-1][1] - g0) // 2)
    g0 = n - 1                                                             # the last probe: the longest run that ends at cell n
    while g0 > 0 and n - (g0 - 1) <= cap and o[n] - o[g0 - 1] <= probe_width:
        g0 -= 1
    runs.append((g0, n))
    own = [0] + [(o[runs[k + 1][0]] + o[runs[k][1]]) // 2 for k in range(len(runs) - 1)] + [o[n]]
    return [(a, b, o[a], o[b], own[k], own[k + 1]) for k, (a, b) in enumerate(runs)]


def probe_windows(probes):
    """the probes as the windows ``columns.gather_table`` takes (``long_lines.Window``: its c0, c1, g0, g1 are read)"""
    return [Window(p[2], p[3], p[0], p[1], 0, 0) for p in probes]


# --------------------------------------------------------------------------------------------------------------------------- the way back
def strip_to_rows(x, cuts, widths):
    """a column ``x`` of the virtual strip (a number, or a sequence of them → a list) → the page row t_j + (x − o_j) · h_j / w_j, fp64, of the cell j
    with o_j <= x < o_j+1; x = Wv belongs to the last cell, and what lies outside [0, Wv] is taken by the first and the last cell"""
    if np.ndim(x):
        return [strip_to_rows(v, cuts, widths) for v in x]
    o, x = columns.cell_offsets(widths), float(x)
    j = 0
    while j < len(widths) - 1 and x >= o[j + 1]:
        j += 1
    return int(cuts[j]) + (x - o[j]) * (int(cuts[j + 1]) - int(cuts[j])) / int(widths[j])


def _given_cuts(box, char_boxes):
    """``columns.cell_cuts(box, n, char_boxes)``'s cuts, by its arithmetic, without its refusal of an empty cell"""
    y1, y2 = int(box[1]), int(box[3])
    top = [int(math.floor(b[1])) for b in char_boxes]
    bottom = [int(math.floor(b[3])) for b in char_boxes]
    return [y1] + [min(max((bottom[j - 1] + top[j]) // 2, y1), y2) for j in range(1, len(char_boxes))] + [y2]


def settle(box, labels, char_boxes, scale, rows=ROW_H):
    """a reading → the reading the given path accepts, (labels, char_boxes) (the module's head states the rule): ``columns.cell_cuts`` of the
    result has no empty cell and none under ``rows`` / 16 output rows at ``scale``.  Never raises; the result may be empty."""
    keep = [(int(l), [float(v) for v in b]) for l, b in zip(labels, char_boxes) if len(b) == 4 and all(math.isfinite(float(v)) for v in b)]
    try:
        s = int(scale)
    except (TypeError, ValueError):
        s = 0
    while keep:
        cuts = _given_cuts(box, [b for _, b in keep])
        heights = [cuts[j + 1] - cuts[j] for j in range(len(keep))]
        worst = min(heights)
        if worst >= 1 and pages.MIN_RECT_H_DIV * s * worst >= int(rows):
            break
        del keep[max(j for j, h in enumerate(heights) if h == worst)]
    return [l for l, _ in keep], [b for _, b in keep]


# --------------------------------------------------------------------------------------------------------------------------- the reading
def plan_columns(boxes, inks, probe_width=384, regions=None):
    """per column its first-pass cells and probes, which need its profile only: → list of dict(box, first_cuts, widths, probes); a refusal names
    column k as region ``regions[k]`` (k itself without)"""
    out = []
    for k, (box, ink) in enumerate(zip(boxes, inks)):
        box = [int(v) for v in box]
        cuts = first_cuts(box, ink)
        widths = columns.cell_widths(box, cuts)
        out.append(dict(box=box, first_cuts=cuts, widths=widths, probes=plan_cell_probes(widths, probe_width, region=k if regions is None else regions[k])))
    return out


def decode(plans, rows, locs, scale=4):
    """the host half of a reading, shared by ``read_columns_host`` and ``MarconetPipeline.read_columns``: ``plans``: ``plan_columns``' result;
    ``rows`` / ``locs``: the argmax indices [ΣP, 64] and the fp32 (left, right) pairs [ΣP, 32] of all probes in column order (``blind.encode``)
    → per column dict(text, labels, char_boxes, cuts, first_cuts, probes, overflow), None for a reading that ``settle`` leaves empty"""
    out, j = [], 0
    for p in plans:
        box, cuts, widths, probes = p["box"], p["first_cuts"], p["widths"], p["probes"]
        reads = [blind.read_probe(rows[j + k], locs[j + k], pr[2:], LQ_H) for k, pr in enumerate(probes)]
        j += len(probes)
        labels, strip_boxes = blind.merge(LQ_H, sum(widths), reads)
        char_boxes = [[float(box[0]), strip_to_rows(b[0], cuts, widths), float(box[2]), strip_to_rows(b[2], cuts, widths)] for b in strip_boxes]
        labels, char_boxes = settle(box, labels, char_boxes, scale)
        out.append(dict(text=lq_io.text_from_labels(labels), labels=labels, char_boxes=char_boxes,
                        cuts=columns.cell_cuts(box, len(labels), char_boxes), first_cuts=list(cuts), probes=list(probes),
                        overflow=any(r[2] for r in reads)) if labels else None)
    return out


def check_boxes(page_h, page_w, boxes, scale):
    """the columns' boxes rounded outward (``pages.round_box``); ``pages.region_rects``' refusals of the scale and of a box that is empty or outside
    the page, naming the column"""
    boxes = [pages.round_box(b, int(page_h), int(page_w)) for b in boxes]
    pages.region_rects(int(page_h), int(page_w), boxes, [False] * len(boxes), scale, 0)
    return boxes


@torch.no_grad()
def read_columns_host(pipe, image, boxes, scale=4, probe_width=384):
    """the definition of ``MarconetPipeline.read_columns``: ``row_ink`` and ``first_cuts`` per column, the virtual strips of the first-pass cells
    (``columns.virtual_strip``), the probes' crops taken on the host and resized by ``lq_device.prepare_strips`` (one batch in probe order), the
    encoder on that batch (``blind.encode``), ``decode`` → what ``read_columns`` returns, to be compared with ``==``"""
    image = pages._page_array(image)
    boxes = check_boxes(image.shape[0], image.shape[1], boxes, scale)
    plans = plan_columns(boxes, [row_ink(image, b) for b in boxes], probe_width)
    if not plans:
        return []
    crops = []
    for p in plans:
        strip, _ = columns.virtual_strip(image, p["box"], p["first_cuts"])
        crops += [np.ascontiguousarray(strip[:, pr[2]:pr[3]]) for pr in p["probes"]]
    prep = lq_device.prepare_strips(crops, next(pipe.sr.parameters()).device)
    rows, locs = blind.encode(pipe, prep.lq)
    return decode(plans, rows, locs, scale)
