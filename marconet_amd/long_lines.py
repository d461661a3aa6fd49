"""Text lines wider than the reference's limit.  The script refuses a strip wider than 512 px at height 32 and tells its user to "crop it into
shorter segments" (test_sr.py:108-110); this module does the cropping and the joining:

    plan_windows    cuts a line into overlapping windows of whole characters, each narrow enough for ``lq_device.strip_geometry``
    stitch_host     the pure-host definition of the join: a column of one window is that window's byte, a column of two is an integer cross-fade
    compose_lines   the same bytes for a whole batch of lines with one kernel launch (``mnet_stitch_u8``) from the uint8 SR result on the device

``MarconetPipeline.restore_lines`` ties them together: every window of every line goes through the three networks as one batch.  How a window
itself is restored does not change; a line that fits one window gives ``restore_images``' bytes.
"""
import collections

import numpy as np

from . import _lib, lq_device, ops
from .lq_io import StripTooWide

ROW_H = lq_device.SHOW_H      # the joined line has the height of ShowSR (test_sr.py:198-201)

Window = collections.namedtuple("Window", "c0 c1 g0 g1 offset show_w")


def crop_geometry(h, cw):
    """``lq_device.strip_geometry`` of an h x cw crop (its own arithmetic, on a view that holds no pixels); None where it refuses the crop as too wide"""
    try:
        return lq_device.shape_geometry(h, cw)
    except StripTooWide:
        return None


def too_wide(h, w):
    """True for a strip ``restore_images`` skips for its width"""
    return crop_geometry(h, w) is None


def cover_fault(offsets, widths, out_w):
    """the join's conditions on one line's windows, in the kernel's order → index of the first window that breaks one, ``len(offsets)`` where the
    line's last columns are not covered, None for a line that can be followed: offsets ≥ 0 and strictly increasing, widths ≥ 1, every column of
    [0, out_w) in one window or in two"""
    prev, m1, m2 = -1, 0, 0
    for k, (off, sw) in enumerate(zip(offsets, widths)):
        off, sw = int(off), int(sw)
        if sw < 1 or off < 0 or off <= prev:
            return k
        if (off > m1 and m1 < out_w) or (off < m2 and off < out_w):
            return k
        prev, end = off, off + sw
        if end > m1:
            m1, m2 = end, m1
        elif end > m2:
            m2 = end
    return len(offsets) if m1 < out_w else None


def plan_out_w(plan):
    """width of the joined line at height 128"""
    return max(w.offset + w.show_w for w in plan)


def plan_windows(h, w, boxes, max_glyphs=16, overlap_glyphs=2):
    """h, w: the line's size in source pixels; boxes: its character boxes [x1,y1,x2,y2] in source pixels, left to right (``lq_io.evenly_spaced_boxes``
    where the caller has none) → list of ``Window``:

        g0, g1     the window holds the whole characters [g0, g1)
        c0, c1     and the source columns [c0, c1): c0 = 0 for the first window, c1 = w for the last; between characters g - 1 and g the cut
                   lies in the middle of their gap, (boxes[g-1].x2 + boxes[g].x1) // 2, clamped into [0, w)
        offset     the window's first column in the joined line (height 128): (256 c0 + h) // (2 h) — 128 c0 / h rounded half up, in integers
        show_w     its width there: what ``lq_device.strip_geometry`` returns for the crop

    Greedy: a window takes as many characters as fit — at most ``max_glyphs``, and the crop accepted by ``strip_geometry`` (≤ 512 px at height
    32) — and the next one starts ``overlap_glyphs`` characters before it ended.  The plan guarantees that every window advances, that every column
    of [0, ``plan_out_w``) lies in one window or in two, and that consecutive windows share at least one column; ValueError naming the character
    where the boxes do not allow it (a character wider than a window, an overlap as large as the window).  A line that fits one window gets
    the one-window plan (0, w, 0, n, 0, show_w)."""
    h, w = int(h), int(w)
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    n = int(b.shape[0])
    max_glyphs, overlap_glyphs = int(max_glyphs), int(overlap_glyphs)
    if n < 1:
        raise ValueError("plan_windows: a line without a character has no windows")
    if h < 1 or w < 1:
        raise ValueError("plan_windows: empty line (%d x %d)" % (h, w))
    if max_glyphs < 1 or not 0 <= overlap_glyphs < max_glyphs:
        raise ValueError("plan_windows: max_glyphs >= 1 and 0 <= overlap_glyphs < max_glyphs expected (got %d, %d)" % (max_glyphs, overlap_glyphs))
    x1, x2 = np.floor(b[:, 0]).astype(np.int64), np.floor(b[:, 2]).astype(np.int64)

    def cut(g):                       # the source column between characters g - 1 and g
        return 0 if g <= 0 else w if g >= n else min(max(int(x2[g - 1] + x1[g]) // 2, 0), w - 1)

    def fit(g0, g1):                  # the geometry of the crop that holds characters [g0, g1), None where strip_geometry refuses it or it is empty
        return crop_geometry(h, cut(g1) - cut(g0)) if cut(g1) > cut(g0) else None

    def no_fit(g):
        return ValueError("plan_windows: character %d does not fit a window (columns %d..%d of a line %d px high: wider than %d px at height %d, "
                          "or empty)" % (g, cut(g), cut(g + 1), h, lq_device.LQ_W, lq_device.LQ_H))

    plan, g0 = [], 0
    while True:
        for g1 in range(min(g0 + max_glyphs, n), g0, -1):
            geom = fit(g0, g1)
            if geom is not None:
                break
        else:
            raise no_fit(g0)
        plan.append(Window(cut(g0), cut(g1), g0, g1, (256 * cut(g0) + h) // (2 * h), int(geom.show_w)))
        if g1 >= n:
            break
        if g1 - overlap_glyphs <= g0:
            if fit(g1, g1 + 1) is None:
                raise no_fit(g1)
            raise ValueError("plan_windows: the window at character %d holds %d character(s), no more than the overlap of %d: the plan cannot advance"
                             % (g0, g1 - g0, overlap_glyphs))
        g0 = g1 - overlap_glyphs
    bad = cover_fault([p.offset for p in plan], [p.show_w for p in plan], plan_out_w(plan))
    for k in range(1, len(plan)):
        if bad is None and plan[k].offset >= plan[k - 1].offset + plan[k - 1].show_w:
            bad = k                   # the windows touch without sharing a column: nothing to cross-fade over
    if bad is not None:
        raise ValueError("plan_windows: the window at character %d cannot be joined to its neighbours (an output column in three windows or in none, or "
                         "no shared column)" % plan[min(bad, len(plan) - 1)].g0)
    return plan


def blend(a, b, t, D):
    """csrc/stitch_blend.h in numpy / Python integers: the byte of column A + t of a D-column overlap, a from the left window, b from the right"""
    return (a * (2 * D - 2 * t - 1) + b * (2 * t + 1) + D) // (2 * D)


def stitch_host(windows_u8, plan):
    """windows_u8[k]: window k's ``ShowSR``, uint8 [rows, show_w_k, 3] → the joined line, uint8 [rows, plan_out_w, 3].  A column in one window is
    that window's byte; a column x in windows k and k + 1 is, per channel, ``blend(a, b, x - A, B - A)`` over the overlap
    [A, B) = [offset_{k+1}, offset_k + show_w_k) — integers only, exact, and the same whichever window is called the left one."""
    if len(windows_u8) != len(plan) or not plan:
        raise ValueError("stitch_host: one image per window expected")
    out_w = plan_out_w(plan)
    if cover_fault([p.offset for p in plan], [p.show_w for p in plan], out_w) is not None:
        raise ValueError("stitch_host: the plan does not cover every column once or twice")
    wins = [np.asarray(v) for v in windows_u8]
    rows = wins[0].shape[0]
    for v, p in zip(wins, plan):
        if v.dtype != np.uint8 or v.shape != (rows, p.show_w, 3):
            raise ValueError("stitch_host: uint8 [%d, %d, 3] expected for the window at character %d, got %s %s" % (rows, p.show_w, p.g0, v.dtype, v.shape))
    out = np.zeros((rows, out_w, 3), dtype=np.uint8)
    x = np.arange(out_w)
    inside = [(x >= p.offset) & (x < p.offset + p.show_w) for p in plan]
    count = np.sum(inside, axis=0)                                    # 1 or 2 everywhere: cover_fault
    for k, p in enumerate(plan):
        alone = inside[k] & (count == 1)
        out[:, alone] = wins[k][:, x[alone] - p.offset]
        for j in range(k + 1, len(plan)):
            both = inside[k] & inside[j]
            if both.any():
                A, D = plan[j].offset, p.offset + p.show_w - plan[j].offset
                a, b = wins[k][:, x[both] - p.offset].astype(np.int64), wins[j][:, x[both] - A].astype(np.int64)
                out[:, both] = blend(a, b, (x[both] - A)[None, :, None], D).astype(np.uint8)
    return out


def build_tables(plans, sr_index=None):
    """→ (record array of ``mnet_stitch_line`` [L], record array of ``mnet_stitch_window`` [ΣW]); window j of the batch (the plans' windows in order)
    shows SR image ``sr_index[j]`` (default: j)"""
    lines = np.zeros((len(plans),), dtype=np.dtype(_lib.StitchLine))
    wins = np.zeros((sum(len(p) for p in plans),), dtype=np.dtype(_lib.StitchWindow))
    j = 0
    for l, plan in enumerate(plans):
        lines[l] = (plan_out_w(plan), j, len(plan), 0)
        for p in plan:
            wins[j] = (j if sr_index is None else int(sr_index[j]), p.offset, p.show_w, 0)
            j += 1
    return lines, wins


def compose_lines(sr_u8, plans):
    """sr_u8: uint8 [ΣW,128,2048,3] BGR on the device (``forward_batch(output="u8_bgr")``), the windows of all lines in the plans' order;
    plans: one ``plan_windows`` result per line → uint8 [L,128,max out_w,3] on the device: ``stitch_host`` of line l at [l, :, :plan_out_w(plans[l])],
    0 beyond.  One copy of each of the two small tables, one launch.  ValueError (before anything is copied or launched) for plans that do not fit
    the tensor or cannot be followed."""
    if not plans or any(not p for p in plans):
        raise ValueError("compose_lines: at least one line, and at least one window per line, expected")
    if sr_u8.dim() != 4 or sum(len(p) for p in plans) != sr_u8.shape[0]:
        raise ValueError("compose_lines: one SR image per window expected (%d windows, SR tensor %s)" % (sum(len(p) for p in plans), list(sr_u8.shape)))
    for l, plan in enumerate(plans):
        if any(p.show_w > sr_u8.shape[2] for p in plan) or cover_fault([p.offset for p in plan], [p.show_w for p in plan], plan_out_w(plan)) is not None:
            raise ValueError("compose_lines: the plan of line %d cannot be followed (a window wider than the %d-px SR image, or a column in three "
                             "windows or in none)" % (l, sr_u8.shape[2]))
    lines, wins = build_tables(plans)
    lines_d, wins_d = ops.table_to_device(lines, sr_u8.device), ops.table_to_device(wins, sr_u8.device)      # one copy of each table
    with ops.on_device(sr_u8):
        return ops.stitch_u8(sr_u8, lines_d, wins_d, out_w=max(plan_out_w(p) for p in plans))
