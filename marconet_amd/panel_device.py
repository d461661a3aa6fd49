"""The output side of the script's driver glue on the GPU: the panel test_sr.py:203-232 saves per strip — preview | preview
with box marks | SR | structure images — composed for a whole batch with one kernel launch (``mnet_panel_u8``) from what is on the device
already: the preview of ``lq_device.prepare_strips(preview=True)``, the uint8 BGR SR output and the generator's structure images.  The host
computes per strip only scalars (the resize step, the mark intervals) and makes one copy of each of the two small tables.

``lq_io`` stays the pure-host definition: the device path returns the bytes of ``lq_io.panel_rgb_u8(lq_io.panel(...))``
(tests/test_panel_device_gpu.py).
"""
import numpy as np
import torch

from . import _lib, ops

ROW_H = 128                   # every row block of the panel (test_sr.py:99,207)
IMG_MAX_WIDTH = 16 * 128      # lq_io.draw_locs: the locs are fractions of the 2048-px SR canvas


def mark_intervals(locs_row, n, show_w):
    """``lq_io.draw_locs``' column intervals for one strip → int32 [n,4] = (a, b, r, t) per character: red on columns [a, b) of the upper half,
    blue on [r, t) of the lower half.  The scalar statement is the script's (test_sr.py:214-231: edges = int(centre·2048) ∓ int(half-width·2048),
    the two products truncated separately; pads 2 and 1; max(0, ·) / min(·, 2048)); each pair is then resolved as numpy resolves the slice
    ``a:b`` on an axis of ``show_w`` columns — a left edge below −2 gives a NEGATIVE stop, which counts from the right end, so the mark then
    runs from column 0 to ``show_w + b``.  An empty interval has b <= a."""
    loc = np.asarray(locs_row, dtype=np.float32).reshape(-1)
    out = np.zeros((int(n), 4), dtype=np.int32)
    pad, padr = 2, 1
    for c in range(int(n)):
        centre, width = int(float(loc[2 * c]) * IMG_MAX_WIDTH), int(float(loc[2 * c + 1]) * IMG_MAX_WIDTH)
        x, y = centre - width, centre + width
        a, b = max(0, x - pad), min(x + pad, IMG_MAX_WIDTH)
        r, t = max(0, y - padr), min(y + padr, IMG_MAX_WIDTH)
        out[c, 0:2] = slice(a, b).indices(int(show_w))[:2]
        out[c, 2:4] = slice(r, t).indices(int(show_w))[:2]
    return out


def build_tables(preview_index, show_w, counts, locs):
    """→ (record array of ``mnet_panel_strip`` [n], int32 marks [ΣN,4]); ``locs[k]``: strip k's ``preds_locs`` row (≥ 2·counts[k] values)"""
    n = len(show_w)
    tab = np.zeros((n,), dtype=np.dtype(_lib.PanelStrip))
    marks, g0 = [], 0
    for k in range(n):
        c, w = int(counts[k]), int(show_w[k])
        tab[k] = (w, int(preview_index[k]), g0, c, ROW_H * c / w)            # step: resize_linear's n_src / n_dst, a Python float
        marks.append(mark_intervals(locs[k], c, w))
        g0 += c
    return tab, np.concatenate(marks, axis=0)


def compose_panels(preview, preview_index, show_w, sr_u8, prior_nhwc4, counts, locs):
    """preview     uint8 [P,128,W,3] on the device (``prepare_strips(preview=True)``), ``preview_index[k]`` strip k's image in it
    show_w      the n strips' widths at height 128
    sr_u8       uint8 [n,128,2048,3] BGR (``forward_batch(output="u8_bgr")``), prior_nhwc4 fp32 [ΣN,128,128,4]: ``_core``'s ``prior_images``
    counts      characters per strip (≥ 1), ``locs[k]`` strip k's ``preds_locs`` row
    → uint8 [n,512,max(show_w),3] on the device: ``lq_io.panel_rgb_u8(lq_io.panel(...))`` of strip k at [k, :, :show_w[k]], 0 beyond.
    ValueError (before anything is copied or launched) for a strip wider than the SR image — ``lq_io.panel`` raises there too, from
    ``np.vstack`` — for a strip without a character, and for tables that do not fit the tensors."""
    n = len(show_w)
    if not (len(preview_index) == len(counts) == len(locs) == n == sr_u8.shape[0]) or n < 1:
        raise ValueError("compose_panels: one preview index, width, count, locs row and SR image per strip expected")
    for k in range(n):
        w, c = int(show_w[k]), int(counts[k])
        if w > sr_u8.shape[2]:
            raise ValueError("compose_panels: strip %d is %d px wide at height %d, wider than the %d-px SR image: its panel rows cannot be stacked"
                             % (k, w, ROW_H, sr_u8.shape[2]))
        if w < 1 or w > preview.shape[2] or not 0 <= int(preview_index[k]) < preview.shape[0]:
            raise ValueError("compose_panels: strip %d (width %d, preview %d) lies outside the preview tensor %s" % (k, w, int(preview_index[k]), list(preview.shape)))
        if c < 1:
            raise ValueError("compose_panels: strip %d has no character (the script skips such strips, test_sr.py:168-170)" % k)
    if sum(int(c) for c in counts) != prior_nhwc4.shape[0]:
        raise ValueError("compose_panels: %d structure images for %d characters" % (prior_nhwc4.shape[0], sum(int(c) for c in counts)))
    tab, marks = build_tables(preview_index, show_w, counts, locs)
    dev = preview.device
    strips_d = ops.table_to_device(tab, dev)                                                     # the one copy of the descriptor table
    marks_d = torch.from_numpy(marks).to(dev)                                                    # the one copy of the marks table
    with ops.on_device(preview):
        return ops.panel_u8(preview, sr_u8, prior_nhwc4, strips_d, marks_d, out_w=max(int(w) for w in show_w))
